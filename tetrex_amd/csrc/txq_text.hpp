// What the kernels over record text share (txq_edit.hip, txq_regex.hip, txq_translate.hip; DESIGN.md §3 "Text kernels: units
// and clipped loads"): the text side of a (something, group) pair, the two binary searches, the unit arithmetic and the
// clipped 16-byte load.  Plain functions, no HIP: tests/native/text_units_dump.cpp runs them on the CPU under sanitizers.
#pragma once
#include "txq_records.hpp"

#define TXQ_TEXT_FN TXQ_HOST_DEVICE inline __attribute__((always_inline))

namespace txq {

// Records text[rec[r] .. rec[r + 1]) back to back, group g = records grp[g] .. grp[g + 1] - 1: what a pair's group index names.
struct TextGroups {
    const uint8_t* text;
    const uint64_t* rec;
    uint64_t n_rec, text_bytes;
    const uint64_t* grp;
    uint64_t n_grp;
};

// Group g as the kernels work on it: records [r0, r1), bytes [gs, ge) of the text.  ok = false: an index or an offset outside
// its array (nothing behind the failed check is read).
struct GroupView {
    bool ok;
    uint64_t r0, r1, gs, ge;
};
TXQ_TEXT_FN GroupView view_group(const TextGroups& t, uint32_t g) {
    GroupView v{};
    if (g >= t.n_grp) return v;
    v.r0 = t.grp[g], v.r1 = t.grp[g + 1];
    if (v.r0 > v.r1 || v.r1 > t.n_rec) return v;
    v.gs = t.rec[v.r0], v.ge = t.rec[v.r1];
    v.ok = v.gs <= v.ge && v.ge <= t.text_bytes;
    return v;
}

// the pair that owns unit u: the first i with pref[i + 1] > u (u < pref[n]; a pair of no units owns none)
TXQ_TEXT_FN uint64_t pair_of_unit(const uint64_t* pref, uint64_t n, uint64_t u) {
    uint64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (pref[mid + 1] > u) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// the record of [r0, r1) that holds byte x (rec[r0] <= x < rec[r1]): the last r with rec[r] <= x
TXQ_TEXT_FN uint64_t record_of(const uint64_t* rec, uint64_t r0, uint64_t r1, uint64_t x) {
    uint64_t lo = r0 + 1, hi = r1;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (rec[mid] > x) hi = mid;
        else lo = mid + 1;
    }
    return lo - 1;
}

// units of `lanes` chunks of `chunk` bytes that a text of `bytes` bytes is cut into
TXQ_TEXT_FN uint64_t units_of(uint64_t bytes, uint32_t lanes, uint32_t chunk) {
    const uint64_t per_unit = (uint64_t)lanes * chunk;
    return (bytes + per_unit - 1) / per_unit;
}

// the bytes [ca, cb) of the text [gs, ge) that lane `lane` of the group's unit `slice` owns (ca >= ge: none)
struct ChunkBounds {
    uint64_t ca, cb;
};
TXQ_TEXT_FN ChunkBounds chunk_bounds(uint64_t gs, uint64_t ge, uint64_t slice, uint32_t lanes, uint32_t lane, uint32_t chunk) {
    const uint64_t ca = gs + (slice * lanes + lane) * (uint64_t)chunk;
    return {ca, ca + chunk < ge ? ca + chunk : ge};
}

typedef uint32_t text4 __attribute__((vector_size(16), may_alias));

// The 16-byte block at address blk (a multiple of 16) of a text that lies at [lo, hi): one 16-byte load where the block is
// inside (`whole`), else byte loads of what is inside and `fill` for the rest, so nothing outside [lo, hi) is read.
// t0 is the first byte's index in the text, byte i of the block being byte t0 + i.  Where the block begins below lo (the text
// is not 16-byte aligned), blk - lo is -k in unsigned arithmetic, k = 1..15: the bytes below lo get an index of 2^64 - k + i,
// beyond any text, and a caller that keeps its indices below a bound skips them; the bytes at and above lo wrap back to their
// true index i - k.  The kernels' record-boundary handling relies on these indices being exact.
struct TextBlock {
    text4 w;
    uint64_t t0;
    bool whole;
};
TXQ_TEXT_FN TextBlock load_block(uintptr_t blk, uintptr_t lo, uintptr_t hi, uint8_t fill) {
    TextBlock b;
    b.t0 = (uint64_t)(blk - lo);
    b.whole = blk >= lo && blk + 16 <= hi;
    if (b.whole) b.w = *reinterpret_cast<const text4*>(blk);
    else {
        // (a byte that is inside replaces the fill: for fill = 0 this folds to q |= byte << shift.  Selecting between byte and
        // fill before one unconditional OR costs regex_kernel 8 VGPRs and a wave per SIMD.)
        const uint32_t f = fill * 0x01010101u;
        uint32_t q[4] = {f, f, f, f};
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (blk + i >= lo && blk + i < hi)
                q[i >> 2] = (q[i >> 2] & ~(0xFFu << (8 * (i & 3)))) | (uint32_t)*reinterpret_cast<const uint8_t*>(blk + i) << (8 * (i & 3));
        b.w = text4{q[0], q[1], q[2], q[3]};
    }
    return b;
}

}  // namespace txq
