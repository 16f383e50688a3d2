// Which records of a bin does a regular expression match?  (automaton, bin) pairs on gfx950 (txq_regex_filter /
// txq_regex_filter_device; `tetrex query --gpu-verify`).  The reference has no counterpart.  The contract is in
// include/txq.h, the automaton and what "matches" means in include/txq_regex.h: the kernel steps through txq_regex_step, the
// same function the host twin (txh_regex_filter) and the CPU tests run.
//
// Mapping to the machine (units, prefix and clipped loads: see txq_text.hpp):
//   * a pair's text is the bytes of its group's records, back to back.  regex_plan_kernel checks the pair, writes its status and
//     cuts the text into units of 256 lane chunks of `chunk` bytes (TXQ_REGEX_CHUNK); scan_kernel (txq_scan.hpp) turns the unit
//     counts into a prefix; the grid of regex_kernel is persistent: a workgroup of four waves takes units u = block, block +
//     grid, ... and finds (pair, slice) by a binary search in the prefix.  The prefix lives in the caller's workspace: the call
//     allocates nothing, reads nothing back and waits for nothing;
//   * per unit the workgroup copies the pair's blob into LDS with 16-byte loads (a unit of the default chunk is 64 KiB of
//     text; the median motif's blob is below 1 KiB) and opens it there: class table, transitions and flags are LDS reads.
//     Three instances of one template: blobs up to 8 KiB (many workgroups per CU), blobs up to 64 KiB (two per CU), and
//     blobs above that, which stay in the arena and are read through L2.  A unit of another tier is skipped;
//   * a lane owns the bytes [a, b) of the text.  Text comes in 16-byte loads (byte loads only where the 16 bytes would leave
//     the buffer); at a record's start the state is start_begin, at its end the "accepts at the end" flag is tested; since the
//     accept state is absorbing it is looked for once per 16 bytes, and a record that matched is left at once;
//   * a BOUNDED automaton (lmax finite): the lane starts in start_mid at max(record start, a - (lmax - 1)).  A match whose last
//     byte is in [a, b) starts no earlier than that, and the unanchored automaton started later than the record's start only
//     loses matches that start before the scan does — so every match is found by the lane that owns its last byte, and a
//     record of any length is spread over lanes;
//   * an UNBOUNDED automaton: the lane that owns a record's first byte scans all of it, up to TXQ_REGEX_MAX_SERIAL bytes; a
//     longer record is flagged unseen (the caller looks at flagged records anyway).  Other lanes skip to the record's end;
//   * records of no bytes belong to no lane: the workgroup of a pair's first unit walks the group's offsets for them;
//   * a record's bit is set with a vector atomicOr on the bitmap's word.
#include "../../include/txq.h"
#include "../../include/txq_regex.h"
#include "txq_internal.hpp"
#include "txq_scan.hpp"
#include "txq_text.hpp"

namespace txq {
namespace {

constexpr uint32_t kDefaultChunk = 256, kMinChunk = 16, kMaxChunk = 1u << 20;
constexpr uint32_t kDefaultSerial = 65536;
constexpr uint32_t kBlock = 256;                    // lanes of a workgroup: a unit is kBlock chunks
constexpr uint32_t kSmallLds = 8192, kLargeLds = 65536;
constexpr uint32_t kCus = 256;

typedef uint32_t rx4 __attribute__((ext_vector_type(4)));

struct RxArgs {
    const uint8_t* arena;
    const uint64_t* aoff;
    uint64_t n_auto, arena_bytes;
    TextGroups t;
    const uint32_t* pairs;
    uint64_t n_pairs;
    const uint64_t* out_off;
    uint32_t* out;
    uint64_t out_words;
    uint32_t* status;
    uint64_t* pref;  // n_pairs + 1: pref[0] = 0, pref[i + 1] = units of pairs 0 .. i
    uint32_t chunk, max_serial;
};

// What a pair works on; ok = false: an index or an offset outside its array, a malformed blob, a bitmap outside d_out.
struct PairView {
    bool ok;
    txq_regex_view rx;  // (tables not bound)
    uint64_t a0, r0, r1, gs, ge, o;
};

__device__ __forceinline__ PairView view_pair(const RxArgs& a, uint64_t i) {
    PairView v{};
    const uint32_t p = a.pairs[2 * i], g = a.pairs[2 * i + 1];
    if (p >= a.n_auto) return v;
    const uint64_t a0 = a.aoff[p], a1 = a.aoff[p + 1];
    if (a0 > a1 || a1 > a.arena_bytes || (a0 & 15) || a1 - a0 < TXQ_REGEX_TABLES) return v;
    const uint32_t* hw = reinterpret_cast<const uint32_t*>(a.arena + a0);
    const uint32_t h[8] = {hw[0], hw[1], hw[2], hw[3], hw[4], hw[5], hw[6], hw[7]};
    if (!txq_regex_header(h, (size_t)(a1 - a0), &v.rx)) return v;
    const GroupView gv = view_group(a.t, g);
    if (!gv.ok) return v;
    const uint64_t o = a.out_off[i], words = (gv.r1 - gv.r0 + 31) / 32;
    v.ok = o <= a.out_words && words <= a.out_words - o;
    v.a0 = a0, v.r0 = gv.r0, v.r1 = gv.r1, v.gs = gv.gs, v.ge = gv.ge, v.o = o;
    return v;
}

__device__ __forceinline__ uint32_t tier_of(uint32_t blob_bytes) { return blob_bytes <= kSmallLds ? 0u : blob_bytes <= kLargeLds ? 1u : 2u; }

__global__ __launch_bounds__(256) void regex_plan_kernel(RxArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) a.pref[0] = 0;
    if (i >= a.n_pairs) return;
    const PairView v = view_pair(a, i);
    uint64_t units = 0;
    if (v.ok && v.r1 > v.r0) {
        units = units_of(v.ge - v.gs, kBlock, a.chunk);
        if (units == 0) units = 1;  // records of no bytes still want their answer
    }
    a.pref[i + 1] = units;
    a.status[i] = v.ok ? 0u : TXQ_REGEX_REFUSED;
}

// The automaton over text[p0, p1) from state s (p1 <= text_bytes): 16-byte loads, the state looked at once per load.
__device__ __forceinline__ uint32_t scan_bytes(const txq_regex_view& v, uintptr_t text_lo, uintptr_t text_hi, uint64_t p0, uint64_t p1, uint32_t s) {
    const uintptr_t first = (text_lo + p0) & ~(uintptr_t)15, last = text_lo + p1;
    for (uintptr_t blk = first; blk < last && s > TXQ_REGEX_ACCEPT; blk += 16) {
        const TextBlock raw = load_block(blk, text_lo, text_hi, 0);
        if (raw.whole && raw.t0 >= p0 && raw.t0 + 16 <= p1) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int b = 0; b < 4; ++b) s = txq_regex_step(v, s, (uint8_t)(raw.w[q] >> (8 * b)));
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t word = raw.w[q];
#pragma nounroll
                for (uint32_t b = 0; b < 4; ++b) {
                    const uint64_t t = raw.t0 + 4u * q + b;  // (bytes below text_lo: an index >= p1, see load_block)
                    if (t >= p0 && t < p1) s = txq_regex_step(v, s, (uint8_t)(word >> (8 * b)));
                }
            }
        }
    }
    return s;
}

template <uint32_t kLds>
__global__ __launch_bounds__(256) void regex_kernel(RxArgs a) {
    __shared__ rx4 table[kLds ? kLds / 16 : 1];
    constexpr uint32_t kTier = kLds == kSmallLds ? 0u : kLds == kLargeLds ? 1u : 2u;
    const uint32_t tid = threadIdx.x;
    const uint64_t total = a.pref[a.n_pairs];
    const uintptr_t text_lo = (uintptr_t)a.t.text, text_hi = text_lo + a.t.text_bytes;
    for (uint64_t u = blockIdx.x; u < total; u += gridDim.x) {
        const uint64_t pair = pair_of_unit(a.pref, a.n_pairs, u);
        const PairView v = view_pair(a, pair);
        if (!v.ok || tier_of(v.rx.total_bytes) != kTier) continue;  // (uniform over the workgroup)
        const uint64_t slice = u - a.pref[pair];
        txq_regex_view rx = v.rx;
        if (kLds) {
            __syncthreads();  // the unit before is done with the table
            const rx4* src = reinterpret_cast<const rx4*>(a.arena + v.a0);
            for (uint32_t i = tid; i < rx.total_bytes / 16; i += kBlock) table[i] = src[i];
            __syncthreads();
            txq_regex_bind(&rx, reinterpret_cast<const uint8_t*>(table));
        } else {
            txq_regex_bind(&rx, a.arena + v.a0);
        }
        uint32_t* bits = a.out + v.o;
        const auto flag = [&](uint64_t r) { atomicOr(bits + ((r - v.r0) >> 5), 1u << ((r - v.r0) & 31)); };
        // a record offset as the kernel uses it: inside the group's bytes whatever the array holds
        const auto at = [&](uint64_t r) {
            const uint64_t x = a.t.rec[r];
            return x < v.gs ? v.gs : x > v.ge ? v.ge : x;
        };
        if (slice == 0 && txq_regex_accepts_at_end(rx, rx.start_begin))  // the records of no bytes
            for (uint64_t r = v.r0 + tid; r < v.r1; r += kBlock)
                if (at(r + 1) <= at(r)) flag(r);

        const auto [ca, cb] = chunk_bounds(v.gs, v.ge, slice, kBlock, tid, a.chunk);
        if (ca >= v.ge) continue;
        uint64_t r = record_of(a.t.rec, v.r0, v.r1, ca);
        if (rx.lmax != TXQ_REGEX_UNBOUNDED) {
            const uint64_t lead = rx.lmax ? rx.lmax - 1 : 0;
            uint64_t pos = ca;
            while (pos < cb && r < v.r1) {
                uint64_t rs = at(r);
                const uint64_t re = at(r + 1);
                if (re <= pos) { ++r; continue; }
                if (rs > pos) rs = pos;  // (offsets that do not ascend)
                const uint64_t start = pos - rs > lead ? pos - lead : rs;
                const uint64_t end = re < cb ? re : cb;
                const uint32_t s = scan_bytes(rx, text_lo, text_hi, start, end, start == rs ? rx.start_begin : rx.start_mid);
                if (s == TXQ_REGEX_ACCEPT || (end == re && txq_regex_accepts_at_end(rx, s))) flag(r);
                pos = end;
                if (end == re) ++r;
            }
        } else {
            if (at(r) < ca) ++r;  // the record that holds a began in front of it: its first byte's lane has it
            for (; r < v.r1; ++r) {
                const uint64_t rs = at(r);
                if (rs >= cb) break;
                if (rs < ca) continue;  // (offsets that do not ascend)
                uint64_t re = at(r + 1);
                if (re < rs) re = rs;
                if (re - rs > a.max_serial) { flag(r); continue; }
                if (txq_regex_accepts_at_end(rx, scan_bytes(rx, text_lo, text_hi, rs, re, rx.start_begin))) flag(r);
            }
        }
    }
}

int regex_args(const void* aoff, const void* rec, const void* grp, const void* pairs, size_t n_pairs, size_t n_records, const void* out_off,
               const void* out, size_t out_words, const void* status) {
    if (!aoff || !rec || !grp || (n_pairs && (!pairs || !out_off || !status)) || (out_words && !out)) return fail(TXQ_ERR_ARG, "null argument");
    if (n_pairs > 0x7FFFFFFFull || n_records >= 0xFFFFFFFEull) return fail(TXQ_ERR_ARG, "at most 2^31 pairs and 2^32 - 2 records per call");
    return TXQ_OK;
}

}  // namespace
}  // namespace txq

using namespace txq;

extern "C" {

int txq_regex_filter_device(const uint8_t* d_automata, const uint64_t* d_auto_offsets, size_t n_automata, size_t automata_bytes,
                            const uint8_t* d_text, const uint64_t* d_rec_offsets, size_t n_records, size_t text_bytes,
                            const uint64_t* d_group_offsets, size_t n_groups, const uint32_t* d_pairs, size_t n_pairs,
                            const uint64_t* d_out_offsets, uint32_t* d_out, size_t out_words, uint32_t* d_status, void* d_workspace,
                            void* stream) {
    if (int rc = regex_args(d_auto_offsets, d_rec_offsets, d_group_offsets, d_pairs, n_pairs, n_records, d_out_offsets, d_out, out_words, d_status))
        return rc;
    if (n_pairs && (!d_workspace || ((uintptr_t)d_workspace & 7))) return fail(TXQ_ERR_ARG, "the workspace must be an 8-byte aligned device pointer");
    if ((automata_bytes && !d_automata) || (text_bytes && !d_text)) return fail(TXQ_ERR_ARG, "null argument");
    if ((uintptr_t)d_automata & 15) return fail(TXQ_ERR_ARG, "the automata must start at a multiple of 16 bytes");
    if (int rc = require_init()) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (out_words) {
        const hipError_t e = hipMemsetAsync(d_out, 0, out_words * 4, st);
        if (e != hipSuccess) return fail_hip(e, "hipMemsetAsync");
    }
    if (n_pairs == 0) return TXQ_OK;
    const uint32_t chunk = (env_u32("TXQ_REGEX_CHUNK", kDefaultChunk, kMinChunk, kMaxChunk) + 15) / 16 * 16;
    const RxArgs a{d_automata, d_auto_offsets, n_automata, automata_bytes, {d_text, d_rec_offsets, n_records, text_bytes, d_group_offsets, n_groups},
                   d_pairs, n_pairs, d_out_offsets, d_out, out_words, d_status, (uint64_t*)d_workspace, chunk,
                   env_u32("TXQ_REGEX_MAX_SERIAL", kDefaultSerial, 1, 0x7FFFFFFFu)};
    regex_plan_kernel<<<(unsigned)((n_pairs + 255) / 256), 256, 0, st>>>(a);
    scan_kernel<<<1, 1024, 0, st>>>(a.pref + 1, n_pairs);
    regex_kernel<kSmallLds><<<kCus * 8, kBlock, 0, st>>>(a);
    regex_kernel<kLargeLds><<<kCus * 2, kBlock, 0, st>>>(a);
    regex_kernel<0><<<kCus * 8, kBlock, 0, st>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "regex kernel launch");
    return TXQ_OK;
}

int txq_regex_filter(const uint8_t* automata, const uint64_t* auto_offsets, size_t n_automata, const uint8_t* text, const uint64_t* rec_offsets,
                     size_t n_records, const uint64_t* group_offsets, size_t n_groups, const uint32_t* pairs, size_t n_pairs,
                     const uint64_t* out_offsets, uint32_t* out, size_t out_words, uint32_t* status) {
    if (!auto_offsets || !rec_offsets || !group_offsets) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = check_ascending(auto_offsets, n_automata, "automaton")) return rc;
    if (int rc = check_ascending(rec_offsets, n_records, "record")) return rc;
    if (int rc = check_ascending(group_offsets, n_groups, "group", "records", n_records)) return rc;
    const uint64_t arena0 = auto_offsets[0], arena_bytes = auto_offsets[n_automata] - arena0;
    const uint64_t text0 = rec_offsets[0], text_bytes = rec_offsets[n_records] - text0;
    if (int rc = regex_args(auto_offsets, rec_offsets, group_offsets, pairs, n_pairs, n_records, out_offsets, out, out_words, status)) return rc;
    if ((arena_bytes && !automata) || (text_bytes && !text)) return fail(TXQ_ERR_ARG, "null argument");
    for (size_t p = 0; p < n_automata; ++p) {  // every blob, every entry of its tables
        const uint64_t a0 = auto_offsets[p], a1 = auto_offsets[p + 1];
        txq_regex_view v;
        if (((a0 - arena0) & 15) || !txq_regex_open(automata + a0, (size_t)(a1 - a0), &v))
            return fail(TXQ_ERR_ARG, "automaton %zu is malformed, or does not start at a multiple of 16 bytes", p);
        bool good = true;
        for (unsigned b = 0; b < 256; ++b) good = good && v.class_of[b] < v.n_classes;
        for (size_t t = 0; t < (size_t)v.n_states * v.n_classes; ++t) good = good && v.next[t] < v.n_states;
        if (!good) return fail(TXQ_ERR_ARG, "automaton %zu: a class or a transition outside its tables", p);
    }
    for (size_t i = 0; i < n_pairs; ++i) {
        const uint32_t p = pairs[2 * i], g = pairs[2 * i + 1];
        if (p >= n_automata || g >= n_groups) return fail(TXQ_ERR_ARG, "pair %zu names automaton %u of %zu, group %u of %zu", i, p, n_automata, g, n_groups);
        const uint64_t words = (group_offsets[g + 1] - group_offsets[g] + 31) / 32;
        if (out_offsets[i] > out_words || words > out_words - out_offsets[i]) return fail(TXQ_ERR_ARG, "pair %zu: its bitmap leaves the output", i);
    }
    if (int rc = require_init()) return rc;
    DeviceStage d;  // (+16: the kernels' 16-byte loads of blobs and text end inside the slice; +8, +4: no slice of no bytes where n_pairs = 0)
    const size_t s_arena = d.add(arena_bytes + 16), s_ao = d.add((n_automata + 1) * 8), s_text = d.add(text_bytes + 16), s_rec = d.add((n_records + 1) * 8),
                 s_grp = d.add((n_groups + 1) * 8), s_pairs = d.add(n_pairs * 8 + 8), s_oo = d.add(n_pairs * 8 + 8), s_out = d.add(out_words * 4 + 4),
                 s_status = d.add(n_pairs * 4 + 4), s_work = d.add(TXQ_REGEX_WORKSPACE(n_pairs));
    if (const hipError_t e = d.alloc(); e != hipSuccess) return fail_hip(e, "hipMalloc");
    const std::vector<uint64_t> ao = rebased(auto_offsets, n_automata), ro = rebased(rec_offsets, n_records);
    d.upload(s_arena, automata + arena0, arena_bytes);
    d.upload(s_ao, ao.data(), ao.size() * 8);
    d.upload(s_text, text + text0, text_bytes);
    d.upload(s_rec, ro.data(), ro.size() * 8);
    d.upload(s_grp, group_offsets, (n_groups + 1) * 8);
    d.upload(s_pairs, pairs, n_pairs * 8);
    d.upload(s_oo, out_offsets, n_pairs * 8);
    int rc = TXQ_OK;
    if (d.error() == hipSuccess)
        rc = txq_regex_filter_device(d.at<uint8_t>(s_arena), d.at<uint64_t>(s_ao), n_automata, arena_bytes, d.at<uint8_t>(s_text), d.at<uint64_t>(s_rec),
                                     n_records, text_bytes, d.at<uint64_t>(s_grp), n_groups, d.at<uint32_t>(s_pairs), n_pairs, d.at<uint64_t>(s_oo),
                                     d.at<uint32_t>(s_out), out_words, d.at<uint32_t>(s_status), d.at<void>(s_work), nullptr);
    if (rc == TXQ_OK) d.download(out, s_out, out_words * 4);  // (waits for the kernels)
    if (rc == TXQ_OK) d.download(status, s_status, n_pairs * 4);
    if (d.error() != hipSuccess) return fail_hip(d.error(), "txq_regex_filter copies");
    return rc;
}

}  // extern "C"
