// What the two edit-distance kernels share (txq_edit.hip: the pattern in one lane, m <= 512; txq_edit_long.hip: the pattern
// over the lanes of a group, m <= 4096): the 64-bit result key, and under hipcc the arguments, the view of a
// pair with its checks, the finish kernel that turns keys into (d, r, j), and the host-buffer call around a _device call.
// The key functions are plain C++: tests/native/edit_long_sim.cpp runs them on the CPU.
#pragma once
#include "txq_text.hpp"

namespace txq {

// A result is one 64-bit key: distance << 48 | position, the position of end j of record r being (bytes of the group before
// r) + (records of the group before r) + j, so records and ends are ordered as the contract orders them and j = 0 of a record
// differs from the end of the record before.  The least key of a pair is its answer.
constexpr uint64_t kNoKey = ~0ULL;
constexpr uint64_t kBadPair = ~0ULL - 1;  // a pair the plan kernel refused
constexpr uint32_t kPosBits = 48;

// the key of distance `score` at byte t of the text (the match ends behind it: j = t + 1 - record start), t in record r of a
// group that begins with record r0 at byte gs
TXQ_TEXT_FN uint64_t edit_key(uint32_t score, uint64_t t, uint64_t gs, uint64_t r, uint64_t r0) {
    return (uint64_t)score << kPosBits | (t - gs + 1 + (r - r0));
}

// (d, r, j) of a key that is neither kNoKey nor kBadPair
struct EditAnswer {
    uint32_t d, r, j;
};
TXQ_TEXT_FN EditAnswer edit_answer(uint64_t key, const uint64_t* rec, uint64_t r0, uint64_t r1, uint64_t gs) {
    const uint64_t pos = key & ((1ULL << kPosBits) - 1);
    // the last record of the group whose end 0 is at or before pos: position of (r, 0) = rec[r] - gs + (r - r0)
    uint64_t lo = r0 + 1, hi = r1;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (rec[mid] - gs + (mid - r0) > pos) hi = mid;
        else lo = mid + 1;
    }
    const uint64_t rr = lo - 1;
    return {(uint32_t)(key >> kPosBits), (uint32_t)rr, (uint32_t)(pos - (rec[rr] - gs + (rr - r0)))};
}

}  // namespace txq

#if defined(__HIPCC__)
#include "../../include/txq.h"
#include "txq_internal.hpp"

namespace txq {
namespace {

struct EdArgs {
    const uint8_t* pat;
    const uint64_t* pat_off;
    uint64_t n_pat, pat_bytes;
    TextGroups t;
    const uint32_t* pairs;
    uint64_t n_pairs;
    const uint8_t* codes;
    uint32_t* out;
    uint64_t* keys;  // n_pairs
    uint64_t* pref;  // n_pairs + 1: pref[0] = 0, pref[i + 1] = units of pairs 0 .. i
    uint32_t chunk;  // bytes of text per lane (txq_edit.hip) or per lane group (txq_edit_long.hip)
};

// What a pair works on; ok = false: an index or an offset outside its array, m = 0 or m > kMax.
struct PairView {
    bool ok;
    uint32_t m, e;
    uint64_t p0, r0, r1, gs, ge;
};

template <uint32_t kMax>
__device__ __forceinline__ PairView view_pair(const EdArgs& a, uint64_t i) {
    PairView v{};
    const uint32_t p = a.pairs[3 * i], g = a.pairs[3 * i + 1];
    v.e = a.pairs[3 * i + 2];
    if (p >= a.n_pat) return v;
    const uint64_t p0 = a.pat_off[p], p1 = a.pat_off[p + 1];
    if (p1 > a.pat_bytes || p0 >= p1 || p1 - p0 > kMax) return v;
    const GroupView gv = view_group(a.t, g);
    v.ok = gv.ok;
    v.m = (uint32_t)(p1 - p0);
    v.p0 = p0, v.r0 = gv.r0, v.r1 = gv.r1, v.gs = gv.gs, v.ge = gv.ge;
    return v;
}

template <uint32_t kMax>
__global__ __launch_bounds__(256) void edit_finish_kernel(EdArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_pairs) return;
    const uint64_t key = a.keys[i];
    uint32_t d = 0xFFFFFFFFu, r = 0xFFFFFFFFu, j = 0xFFFFFFFFu;
    if (key == kBadPair) r = j = 0xFFFFFFFEu;
    else if (key != kNoKey) {
        const PairView v = view_pair<kMax>(a, i);
        const EditAnswer ans = edit_answer(key, a.t.rec, v.r0, v.r1, v.gs);
        d = ans.d, r = ans.r, j = ans.j;
    }
    a.out[3 * i] = d;
    a.out[3 * i + 1] = r;
    a.out[3 * i + 2] = j;
}

inline int edit_args(const void* pat_off, const void* rec, const void* grp, const void* pairs, size_t n_pairs, size_t n_records, size_t text_bytes,
                     const void* codes, const void* out) {
    if (!pat_off || !rec || !grp || !codes || (n_pairs && (!pairs || !out))) return fail(TXQ_ERR_ARG, "null argument");
    if (n_pairs > 0x7FFFFFFFull || n_records >= 0xFFFFFFFEull) return fail(TXQ_ERR_ARG, "at most 2^31 pairs and 2^32 - 2 records per call");
    if ((uint64_t)text_bytes + n_records >= 1ULL << kPosBits) return fail(TXQ_ERR_ARG, "text too large for one call");
    return TXQ_OK;
}

// what a _device entry point can see of its arguments before it launches
inline int edit_device_args(const uint8_t* d_patterns, const uint64_t* d_pat_offsets, size_t pattern_bytes, const uint8_t* d_text,
                            const uint64_t* d_rec_offsets, size_t n_records, size_t text_bytes, const uint64_t* d_group_offsets,
                            const uint32_t* d_pairs, size_t n_pairs, const uint8_t* d_codes, uint32_t* d_out, void* d_workspace) {
    if (int rc = edit_args(d_pat_offsets, d_rec_offsets, d_group_offsets, d_pairs, n_pairs, n_records, text_bytes, d_codes, d_out)) return rc;
    if (n_pairs && (!d_workspace || ((uintptr_t)d_workspace & 7))) return fail(TXQ_ERR_ARG, "the workspace must be an 8-byte aligned device pointer");
    if ((pattern_bytes && !d_patterns) || (text_bytes && !d_text)) return fail(TXQ_ERR_ARG, "null argument");
    return require_init();
}

using EditDeviceFn = int (*)(const uint8_t*, const uint64_t*, size_t, size_t, const uint8_t*, const uint64_t*, size_t, size_t, const uint64_t*, size_t,
                             const uint32_t*, size_t, const uint8_t*, uint32_t*, void*, void*);

// The host-buffer form of a _device call: the buffers checked (patterns of 1 .. max_pattern bytes), staged, `device` run on
// them with `workspace` bytes, the results copied back.
inline int edit_search_staged(const uint8_t* patterns, const uint64_t* pat_offsets, size_t n_patterns, const uint8_t* text, const uint64_t* rec_offsets,
                              size_t n_records, const uint64_t* group_offsets, size_t n_groups, const uint32_t* pairs, size_t n_pairs,
                              const uint8_t* codes, uint32_t* out, uint32_t max_pattern, size_t workspace, EditDeviceFn device, const char* who) {
    if (!pat_offsets || !rec_offsets || !group_offsets) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = check_ascending(pat_offsets, n_patterns, "pattern")) return rc;
    if (int rc = check_ascending(rec_offsets, n_records, "record")) return rc;
    if (int rc = check_ascending(group_offsets, n_groups, "group", "records", n_records)) return rc;
    const uint64_t pat0 = pat_offsets[0], pat_bytes = pat_offsets[n_patterns] - pat0;
    const uint64_t text0 = rec_offsets[0], text_bytes = rec_offsets[n_records] - text0;
    if (int rc = edit_args(pat_offsets, rec_offsets, group_offsets, pairs, n_pairs, n_records, text_bytes, codes, out)) return rc;
    if ((pat_bytes && !patterns) || (text_bytes && !text)) return fail(TXQ_ERR_ARG, "null argument");
    for (size_t i = 0; i < n_pairs; ++i) {
        const uint32_t p = pairs[3 * i], g = pairs[3 * i + 1];
        if (p >= n_patterns || g >= n_groups) return fail(TXQ_ERR_ARG, "pair %zu names pattern %u of %zu, group %u of %zu", i, p, n_patterns, g, n_groups);
        const uint64_t m = pat_offsets[p + 1] - pat_offsets[p];
        if (m < 1 || m > max_pattern) return fail(TXQ_ERR_ARG, "pair %zu: a pattern of %llu bytes (1..%u run on the device)", i, (unsigned long long)m, max_pattern);
    }
    if (int rc = require_init()) return rc;
    if (n_pairs == 0) return TXQ_OK;
    DeviceStage d;  // (+16: the kernels' 16-byte loads of patterns and text end inside the slice)
    const size_t s_pat = d.add(pat_bytes + 16), s_po = d.add((n_patterns + 1) * 8), s_text = d.add(text_bytes + 16), s_rec = d.add((n_records + 1) * 8),
                 s_grp = d.add((n_groups + 1) * 8), s_pairs = d.add(n_pairs * 12), s_codes = d.add(256), s_out = d.add(n_pairs * 12),
                 s_work = d.add(workspace);
    if (const hipError_t e = d.alloc(); e != hipSuccess) return fail_hip(e, "hipMalloc");
    const std::vector<uint64_t> po = rebased(pat_offsets, n_patterns), ro = rebased(rec_offsets, n_records);
    d.upload(s_pat, patterns + pat0, pat_bytes);
    d.upload(s_po, po.data(), po.size() * 8);
    d.upload(s_text, text + text0, text_bytes);
    d.upload(s_rec, ro.data(), ro.size() * 8);
    d.upload(s_grp, group_offsets, (n_groups + 1) * 8);
    d.upload(s_pairs, pairs, n_pairs * 12);
    d.upload(s_codes, codes, 256);
    int rc = TXQ_OK;
    if (d.error() == hipSuccess)
        rc = device(d.at<uint8_t>(s_pat), d.at<uint64_t>(s_po), n_patterns, pat_bytes, d.at<uint8_t>(s_text), d.at<uint64_t>(s_rec), n_records, text_bytes,
                    d.at<uint64_t>(s_grp), n_groups, d.at<uint32_t>(s_pairs), n_pairs, d.at<uint8_t>(s_codes), d.at<uint32_t>(s_out), d.at<void>(s_work),
                    nullptr);
    if (rc == TXQ_OK) d.download(out, s_out, n_pairs * 12);  // (waits for the kernels)
    if (d.error() != hipSuccess) return fail_hip(d.error(), who);
    return rc;
}

}  // namespace
}  // namespace txq
#endif
