// Every record of a bin that a pattern matches within its cap, on gfx950 (txq_edit_targets* / txq_edit_targets*_device;
// `tetrex search --verify --all-targets`).  The reference has no counterpart.  The semantics are in include/txq.h.
//
// The per-record form of the two edit-distance kernels.  txq_edit.hip and txq_edit_long.hip walk a group's records in order,
// reset their state at every record end and know the record of every score they see; their wave reduction keeps the least
// key of the group.  The kernels here keep one key per (pair, record) instead — a slot, txq_edit_targets_plan.hpp — and a
// compaction turns the slots that hold a key into the ordered hit list:
//   * targets_plan_kernel: per pair the units (as edit_plan_kernel / edit_long_plan_kernel count them) and the records of its
//     group; scan_kernel turns both into prefixes.  targets_init_kernel then refuses the pairs whose slots end beyond the
//     caller's n_slots and gives every slot in use its first key: end 0 of its record where m <= e, else none;
//   * targets_kernel<W>: the lane loop of edit_kernel<W>, `best` belonging to the lane's current record.  Where the loop
//     detects the record's end, and once behind the lane's last byte, the lane flushes: one 64-bit atomicMin into the
//     record's slot where best is a key.  No wave reduction — the lanes are in different records;
//   * targets_long_kernel<G>: the systolic loop of edit_long_kernel<G>; the scoring lane of each lane group flushes for its
//     record when a reset reaches it and once behind the last step, inside the branch only that lane takes, so that all 64
//     lanes are active at the cross-lane move;
//   * targets_count_kernel counts the keys of every 256 slots, scan_kernel makes the counts a prefix, targets_write_kernel
//     writes row (pair, d, r, j) of every key at its rank — the rows in front of `capacity` — and one more thread the total.
//     No atomic append: the order is the slots', pair by pair and record by record, whatever the scheduling.
// Everything lives in the caller's workspace; the call allocates nothing, reads nothing back and waits for nothing.
#include "txq_edit_long_plan.hpp"
#include "txq_edit_targets_plan.hpp"
#include "txq_scan.hpp"

namespace txq {
namespace {

constexpr uint32_t kShortMax = TXQ_EDIT_MAX_PATTERN, kLongMax = TXQ_EDIT_LONG_MAX_PATTERN;
static_assert(kLongMax == kEditLongMaxPattern, "one word per lane");
constexpr uint32_t kDefaultChunk = 512, kDefaultSpan = 4096, kMinChunk = 16, kMaxChunk = 1u << 20;  // (those of the search kernels)
constexpr uint32_t kGridBlocks = 256 * 16;  // waves of the persistent grid: 16 per CU

struct TgArgs {
    EdArgs a;         // (keys and out unused; pref: the units' prefix)
    uint64_t* spref;  // n_pairs + 1: spref[0] = 0, spref[i + 1] = slots of pairs 0 .. i
    uint64_t* slots;  // n_slots keys
    uint64_t* bpref;  // blocks + 1: bpref[0] = 0, bpref[b + 1] = keys in blocks 0 .. b of the slots
    uint64_t n_slots;
    uint32_t* status;
    uint32_t* hits;
    uint64_t capacity;
    uint64_t* total;
};

__device__ __forceinline__ uint32_t words_of(uint32_t m) { return m <= 64 ? 1u : m <= 128 ? 2u : m <= 256 ? 4u : 8u; }

// kMax = kShortMax: units of 64 lane chunks; kLongMax: units of 64 / G spans
template <uint32_t kMax>
__global__ __launch_bounds__(256) void targets_plan_kernel(TgArgs g) {
    const EdArgs& a = g.a;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) a.pref[0] = 0, g.spref[0] = 0;
    if (i >= a.n_pairs) return;
    const PairView v = view_pair<kMax>(a, i);
    uint64_t units = 0;
    if (v.ok) units = kMax == kShortMax ? units_of(v.ge - v.gs, 64, a.chunk) : long_units(v.ge - v.gs, long_group_lanes(v.m), a.chunk);
    a.pref[i + 1] = units;
    g.spref[i + 1] = targets_slots_of(v.ok, v.r0, v.r1);
    g.status[i] = v.ok ? 0u : kTargetsRefused;
}

// thread i < n_pairs: pair i refused where its slots do not fit; thread s < slots in use: the slot's first key
template <uint32_t kMax>
__global__ __launch_bounds__(256) void targets_init_kernel(TgArgs g) {
    const EdArgs& a = g.a;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.n_pairs && !targets_fits(g.spref, i, g.n_slots)) g.status[i] = kTargetsRefused;
    if (i >= targets_used(g.spref, a.n_pairs, g.n_slots)) return;
    const uint64_t pair = pair_of_unit(g.spref, a.n_pairs, i);
    uint64_t key = kNoKey;
    if (targets_fits(g.spref, pair, g.n_slots)) {
        const PairView v = view_pair<kMax>(a, pair);  // (ok: a pair that is not has no slots)
        key = targets_initial_key(v.m, v.e, a.t.rec, v.r0 + (i - g.spref[pair]), v.r0, v.gs);
    }
    g.slots[i] = key;
}

__device__ __forceinline__ void lower_slot(uint64_t* slots, uint64_t slot, uint64_t key) {
    if (slot != kNoSlot) atomicMin((unsigned long long*)(slots + slot), (unsigned long long)key);
}

template <int W>
__global__ __launch_bounds__(64) void targets_kernel(TgArgs g) {
    __shared__ uint64_t peq[32 * W];
    __shared__ uint8_t codes[256];
    const EdArgs& a = g.a;
    const uint32_t lane = threadIdx.x;
    const uint64_t total = a.pref[a.n_pairs];
    if (blockIdx.x >= total) return;
    for (uint32_t i = lane; i < 256; i += 64) {
        const uint8_t c = a.codes[i];
        codes[i] = c < 31 ? c : (uint8_t)31;
    }
    const uintptr_t text_lo = (uintptr_t)a.t.text, text_hi = text_lo + a.t.text_bytes;
    for (uint64_t u = blockIdx.x; u < total; u += gridDim.x) {
        const uint64_t pair = pair_of_unit(a.pref, a.n_pairs, u);
        const PairView v = view_pair<kShortMax>(a, pair);
        if (!v.ok || words_of(v.m) != (uint32_t)W || !targets_fits(g.spref, pair, g.n_slots)) continue;  // (uniform over the wave)
        const uint64_t slice = u - a.pref[pair], base = g.spref[pair];
        __syncthreads();  // the unit before is done with peq
        for (uint32_t i = lane; i < 32 * W; i += 64) peq[i] = 0;
        __syncthreads();
        for (uint32_t i = lane; i < v.m; i += 64) {
            const uint32_t c = codes[a.pat[v.p0 + i]];
            if (c < 31) atomicOr(reinterpret_cast<uint32_t*>(peq) + 2 * (c * W + (i >> 6)) + ((i >> 5) & 1), 1u << (i & 31));
        }
        __syncthreads();

        const uint32_t m = v.m, e = v.e;
        const uint32_t hw = (m - 1) >> 6, hs = (m - 1) & 63;
        const uint64_t lead = (uint64_t)m + (e < m ? e : m);
        const auto [ca, cb] = chunk_bounds(v.gs, v.ge, slice, 64, lane, a.chunk);
        if (ca < v.ge) {
            uint64_t best = kNoKey;  // of record r
            uint64_t r = record_of(a.t.rec, v.r0, v.r1, ca);
            uint64_t rs = a.t.rec[r], re = a.t.rec[r + 1];
            // (offsets that do not ascend cannot take a load outside [gs, ge): every byte index below stays in [start, cb))
            if (rs < v.gs || rs > ca) rs = ca;
            const uint64_t start = ca - rs > lead ? ca - lead : rs;
            uint64_t pv[W], mv[W];
#pragma unroll
            for (int w = 0; w < W; ++w) pv[w] = ~0ULL, mv[w] = 0;
            uint32_t score = m;
            const uintptr_t first = (text_lo + start) & ~(uintptr_t)15, last = text_lo + cb;
            for (uintptr_t blk = first; blk < last; blk += 16) {
                const TextBlock raw = load_block(blk, text_lo, text_hi, 0);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t word = raw.w[q];
#pragma nounroll
                    for (uint32_t b = 0; b < 4; ++b) {
                        const uint64_t t = raw.t0 + 4u * q + b;  // (bytes below text_lo: an index >= cb, see load_block)
                        if (t < start || t >= cb) continue;
                        if (t >= re) {  // the record ended: its key goes to its slot, a fresh state in the next one that has bytes
                            lower_slot(g.slots, targets_flush(best, base, r, v.r0, v.r1), best);
                            best = kNoKey;
                            do {
                                ++r;
                                re = r + 1 <= v.r1 ? a.t.rec[r + 1] : v.ge;
                            } while (t >= re && r + 1 < v.r1);
                            if (re > v.ge || t >= re) re = v.ge;
#pragma unroll
                            for (int w = 0; w < W; ++w) pv[w] = ~0ULL, mv[w] = 0;
                            score = m;
                        }
                        const uint32_t cls = codes[(word >> (8 * b)) & 255u];
                        uint64_t carry = 0, ph_in = 0, mh_in = 0;
                        uint32_t hp = 0, hm = 0;
#pragma unroll
                        for (int w = 0; w < W; ++w) {
                            const uint64_t eq = peq[cls * W + w], p = pv[w], n = mv[w];
                            const uint64_t xv = eq | n, x = eq & p;
                            const uint64_t s1 = x + p, s2 = s1 + carry;
                            carry = (uint64_t)(s1 < x) | (uint64_t)(s2 < s1);
                            const uint64_t xh = (s2 ^ p) | eq;
                            uint64_t ph = n | ~(xh | p), mh = p & xh;
                            if (W == 1 || w >= W / 2) {
                                hp = (uint32_t)w == hw ? (uint32_t)(ph >> hs) & 1u : hp;
                                hm = (uint32_t)w == hw ? (uint32_t)(mh >> hs) & 1u : hm;
                            }
                            const uint64_t ph_out = ph >> 63, mh_out = mh >> 63;
                            ph = (ph << 1) | ph_in;
                            mh = (mh << 1) | mh_in;
                            ph_in = ph_out, mh_in = mh_out;
                            pv[w] = mh | ~(xv | ph);
                            mv[w] = ph & xv;
                        }
                        score += hp - hm;
                        if (t >= ca && score <= e) {
                            const uint64_t key = edit_key(score, t, v.gs, r, v.r0);
                            best = key < best ? key : best;
                        }
                    }
                }
            }
            lower_slot(g.slots, targets_flush(best, base, r, v.r0, v.r1), best);  // behind the lane's last byte
        }
    }
}

// every lane gets the value of the lane below it in the wave (lane 0: 0).  Called where all 64 lanes are active.
__device__ __forceinline__ uint32_t from_lane_before(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
}

template <int G>
__global__ __launch_bounds__(64) void targets_long_kernel(TgArgs g) {
    __shared__ uint64_t peq[32 * G];
    __shared__ uint8_t codes[256];
    const EdArgs& a = g.a;
    const uint32_t lane = threadIdx.x, w = lane % G, group = lane / G;
    const uint64_t total = a.pref[a.n_pairs];
    if (blockIdx.x >= total) return;
    for (uint32_t i = lane; i < 256; i += 64) {
        const uint8_t c = a.codes[i];
        codes[i] = c < 31 ? c : (uint8_t)31;
    }
    const uintptr_t text_lo = (uintptr_t)a.t.text, text_hi = text_lo + a.t.text_bytes;
    for (uint64_t u = blockIdx.x; u < total; u += gridDim.x) {
        const uint64_t pair = pair_of_unit(a.pref, a.n_pairs, u);
        const PairView v = view_pair<kLongMax>(a, pair);
        if (!v.ok || long_group_lanes(v.m) != (uint32_t)G || !targets_fits(g.spref, pair, g.n_slots)) continue;  // (uniform over the wave)
        const uint64_t slice = u - a.pref[pair], slot0 = g.spref[pair];
        __syncthreads();  // the unit before is done with peq
        for (uint32_t i = lane; i < 32 * G; i += 64) peq[i] = 0;
        __syncthreads();
        for (uint32_t i = lane; i < v.m; i += 64) {
            const uint32_t c = codes[a.pat[v.p0 + i]];
            if (c < 31) atomicOr(reinterpret_cast<uint32_t*>(peq) + 2 * (c * G + (i >> 6)) + ((i >> 5) & 1), 1u << (i & 31));
        }
        __syncthreads();

        const uint32_t m = v.m, e = v.e;
        const uint32_t hw = (m - 1) >> 6, bit = w == hw ? (m - 1) & 63 : 63u;
        const auto [ca, cb] = long_span(v.gs, v.ge, slice, G, group, a.chunk);
        // this group's walk: columns from the 16-byte block that holds `start` up to cb, column c being byte t0 + c of the
        // text (t0 + c wraps to the true index where the block begins below the text: load_block)
        uint64_t start = 0, t0 = 0, columns = 0, rf = v.r0, rf_end = 0;
        uintptr_t base = 0;
        if (ca < v.ge) {
            rf = record_of(a.t.rec, v.r0, v.r1, ca);
            rf_end = a.t.rec[rf + 1];
            start = long_start(ca, a.t.rec[rf], v.gs, m, e);
            base = (text_lo + start) & ~(uintptr_t)15;
            t0 = (uint64_t)(base - text_lo);
            columns = (uint64_t)(text_lo + cb - base);
        }
        uint64_t steps = long_steps(columns, m);  // the most of the wave's groups
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const uint64_t o = __shfl_xor(steps, d);
            steps = o > steps ? o : steps;
        }
        uint64_t pv = ~0ULL, mv = 0, rs = rf, best = kNoKey;  // (rs: the record of the scoring lane's column; best: of record rs)
        uint32_t score = m, out = 0;
        for (uint64_t s0 = 0; s0 < steps; s0 += 16) {
            TextBlock raw{};
            if (w == 0 && s0 < columns) raw = load_block(base + s0, text_lo, text_hi, 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t word = raw.w[q];
#pragma nounroll
                for (uint32_t b = 0; b < 4; ++b) {
                    const uint64_t s = s0 + 4u * q + b;
                    uint32_t msg = from_lane_before(out);
                    if (w == 0) {  // the next text byte, where this group has one
                        const uint64_t t = t0 + s;
                        msg = 0;
                        if (s < columns && t >= start && t < cb) {
                            const bool reset = t >= rf_end;  // the record ended: a fresh state in the next one that has bytes
                            if (reset) rf_end = long_next_record(a.t.rec, rf, v.r1, v.ge, t);
                            msg = long_feed(codes[(word >> (8 * b)) & 255u], reset);
                        }
                    }
                    out = long_block_step(pv, mv, peq[(msg & kMsgClass) * G + w], msg, bit);
                    if (w == hw && (out & kMsgValid)) {
                        const uint64_t t = t0 + s - hw;
                        if (out & kMsgReset) {  // record rs ended: its key goes to its slot
                            lower_slot(g.slots, targets_flush(best, slot0, rs, v.r0, v.r1), best);
                            best = kNoKey;
                            score = m;
                            (void)long_next_record(a.t.rec, rs, v.r1, v.ge, t);
                        }
                        score += (uint32_t)long_hin(out);
                        if (t >= ca && score <= e) {
                            const uint64_t key = edit_key(score, t, v.gs, rs, v.r0);
                            best = key < best ? key : best;
                        }
                    }
                }
            }
        }
        if (w == hw) lower_slot(g.slots, targets_flush(best, slot0, rs, v.r0, v.r1), best);  // behind the last step
    }
}

// keys in block b of the slots -> bpref[b + 1]
__global__ __launch_bounds__(kTargetsBlock) void targets_count_kernel(TgArgs g) {
    __shared__ uint32_t wave_count[kTargetsBlock / 64];
    const uint64_t s = (uint64_t)blockIdx.x * kTargetsBlock + threadIdx.x;
    const bool hit = s < targets_used(g.spref, g.a.n_pairs, g.n_slots) && g.slots[s] != kNoKey;
    const uint32_t n = (uint32_t)__popcll(__ballot(hit));
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) g.bpref[0] = 0;
        g.bpref[blockIdx.x + 1] = (uint64_t)wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
    }
}

// blocks 0 .. B - 1: the rows of their slots' keys; block B: the total
template <uint32_t kMax>
__global__ __launch_bounds__(kTargetsBlock) void targets_write_kernel(TgArgs g, uint64_t n_blocks) {
    __shared__ uint32_t wave_count[kTargetsBlock / 64];
    const EdArgs& a = g.a;
    if (blockIdx.x == n_blocks) {
        if (threadIdx.x == 0) *g.total = n_blocks ? g.bpref[n_blocks] : 0;
        return;
    }
    const uint64_t s = (uint64_t)blockIdx.x * kTargetsBlock + threadIdx.x;
    const uint64_t key = s < targets_used(g.spref, a.n_pairs, g.n_slots) ? g.slots[s] : kNoKey;
    const bool hit = key != kNoKey;
    const uint64_t mask = __ballot(hit);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_count[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (!hit) return;
    uint64_t row = g.bpref[blockIdx.x] + (uint64_t)__popcll(mask & ((1ULL << lane) - 1));
    for (uint32_t k = 0; k < wave; ++k) row += wave_count[k];
    if (row >= g.capacity) return;
    const uint64_t pair = pair_of_unit(g.spref, a.n_pairs, s);
    const PairView v = view_pair<kMax>(a, pair);
    targets_row(g.hits + 4 * row, pair, key, a.t.rec, v.r0, v.r1, v.gs);
}

template <uint32_t kMax>
int targets_device(const uint8_t* d_patterns, const uint64_t* d_pat_offsets, size_t n_patterns, size_t pattern_bytes, const uint8_t* d_text,
                   const uint64_t* d_rec_offsets, size_t n_records, size_t text_bytes, const uint64_t* d_group_offsets, size_t n_groups,
                   const uint32_t* d_pairs, size_t n_pairs, const uint8_t* d_codes, uint32_t* d_hits, size_t capacity, uint64_t* d_total,
                   uint32_t* d_status, size_t n_slots, void* d_workspace, void* stream) {
    if (!d_total || (n_pairs && !d_status) || (capacity && !d_hits)) return fail(TXQ_ERR_ARG, "null argument");
    // (d_total stands in for the search calls' d_out in the shared checks: it is what every call writes)
    if (int rc = edit_device_args(d_patterns, d_pat_offsets, pattern_bytes, d_text, d_rec_offsets, n_records, text_bytes, d_group_offsets, d_pairs, n_pairs,
                                  d_codes, (uint32_t*)d_total, d_workspace))
        return rc;
    if (n_slots >= 1ULL << 38 || capacity >= 1ULL << 38) return fail(TXQ_ERR_ARG, "at most 2^38 slots and rows per call");
    hipStream_t st = (hipStream_t)stream;
    if (n_pairs == 0) n_slots = 0;
    const uint64_t n_blocks = targets_blocks(n_slots);
    const bool is_short = kMax == kShortMax;
    const uint32_t chunk = (env_u32(is_short ? "TXQ_EDIT_CHUNK" : "TXQ_EDIT_LONG_SPAN", is_short ? kDefaultChunk : kDefaultSpan, kMinChunk, kMaxChunk) + 15) / 16 * 16;
    uint64_t* const ws = (uint64_t*)d_workspace;  // unit prefix, slot prefix, slots, block prefix: TXQ_EDIT_TARGETS_WORKSPACE
    TgArgs g{{d_patterns, d_pat_offsets, n_patterns, pattern_bytes, {d_text, d_rec_offsets, n_records, text_bytes, d_group_offsets, n_groups},
              d_pairs, n_pairs, d_codes, nullptr, nullptr, ws, chunk},
             ws + (n_pairs + 1), ws + 2 * (n_pairs + 1), ws + 2 * (n_pairs + 1) + n_slots, n_slots, d_status, d_hits, capacity, d_total};
    if (n_pairs) {
        const unsigned per_pair = (unsigned)((n_pairs + 255) / 256);
        const uint64_t most = n_pairs > n_slots ? n_pairs : n_slots;
        targets_plan_kernel<kMax><<<per_pair, 256, 0, st>>>(g);
        scan_kernel<<<1, 1024, 0, st>>>(g.a.pref + 1, n_pairs);
        scan_kernel<<<1, 1024, 0, st>>>(g.spref + 1, n_pairs);
        targets_init_kernel<kMax><<<(unsigned)((most + 255) / 256), 256, 0, st>>>(g);
        if (is_short) {
            targets_kernel<1><<<kGridBlocks, 64, 0, st>>>(g);
            targets_kernel<2><<<kGridBlocks, 64, 0, st>>>(g);
            targets_kernel<4><<<kGridBlocks, 64, 0, st>>>(g);
            targets_kernel<8><<<kGridBlocks, 64, 0, st>>>(g);
        } else {
            targets_long_kernel<16><<<kGridBlocks, 64, 0, st>>>(g);
            targets_long_kernel<32><<<kGridBlocks, 64, 0, st>>>(g);
            targets_long_kernel<64><<<kGridBlocks, 64, 0, st>>>(g);
        }
        if (n_blocks) {
            targets_count_kernel<<<(unsigned)n_blocks, kTargetsBlock, 0, st>>>(g);
            scan_kernel<<<1, 1024, 0, st>>>(g.bpref + 1, n_blocks);
        }
    }
    targets_write_kernel<kMax><<<(unsigned)n_blocks + 1, kTargetsBlock, 0, st>>>(g, n_blocks);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "edit targets kernel launch");
    return TXQ_OK;
}

using TargetsDeviceFn = int (*)(const uint8_t*, const uint64_t*, size_t, size_t, const uint8_t*, const uint64_t*, size_t, size_t, const uint64_t*, size_t,
                                const uint32_t*, size_t, const uint8_t*, uint32_t*, size_t, uint64_t*, uint32_t*, size_t, void*, void*);

// The host-buffer form: the buffers checked as txq_edit_search checks them, staged, `device` run on them, hits, total and
// status copied back.
int targets_staged(const uint8_t* patterns, const uint64_t* pat_offsets, size_t n_patterns, const uint8_t* text, const uint64_t* rec_offsets,
                   size_t n_records, const uint64_t* group_offsets, size_t n_groups, const uint32_t* pairs, size_t n_pairs, const uint8_t* codes,
                   uint32_t* hits, size_t capacity, uint64_t* total, uint32_t* status, size_t n_slots, uint32_t max_pattern, TargetsDeviceFn device,
                   const char* who) {
    if (!pat_offsets || !rec_offsets || !group_offsets || !total || (n_pairs && !status) || (capacity && !hits)) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = check_ascending(pat_offsets, n_patterns, "pattern")) return rc;
    if (int rc = check_ascending(rec_offsets, n_records, "record")) return rc;
    if (int rc = check_ascending(group_offsets, n_groups, "group", "records", n_records)) return rc;
    const uint64_t pat0 = pat_offsets[0], pat_bytes = pat_offsets[n_patterns] - pat0;
    const uint64_t text0 = rec_offsets[0], text_bytes = rec_offsets[n_records] - text0;
    if (int rc = edit_args(pat_offsets, rec_offsets, group_offsets, pairs, n_pairs, n_records, text_bytes, codes, total)) return rc;
    if ((pat_bytes && !patterns) || (text_bytes && !text)) return fail(TXQ_ERR_ARG, "null argument");
    if (n_slots >= 1ULL << 38 || capacity >= 1ULL << 38) return fail(TXQ_ERR_ARG, "at most 2^38 slots and rows per call");
    for (size_t i = 0; i < n_pairs; ++i) {
        const uint32_t p = pairs[3 * i], g = pairs[3 * i + 1];
        if (p >= n_patterns || g >= n_groups) return fail(TXQ_ERR_ARG, "pair %zu names pattern %u of %zu, group %u of %zu", i, p, n_patterns, g, n_groups);
        const uint64_t m = pat_offsets[p + 1] - pat_offsets[p];
        if (m < 1 || m > max_pattern) return fail(TXQ_ERR_ARG, "pair %zu: a pattern of %llu bytes (1..%u run on the device)", i, (unsigned long long)m, max_pattern);
    }
    if (int rc = require_init()) return rc;
    if (n_pairs == 0) n_slots = 0;
    DeviceStage d;  // (+16: the kernels' 16-byte loads of patterns and text end inside the slice)
    const size_t s_pat = d.add(pat_bytes + 16), s_po = d.add((n_patterns + 1) * 8), s_text = d.add(text_bytes + 16), s_rec = d.add((n_records + 1) * 8),
                 s_grp = d.add((n_groups + 1) * 8), s_pairs = d.add(n_pairs * 12 + 4), s_codes = d.add(256), s_hits = d.add(capacity * 16 + 4),
                 s_total = d.add(8), s_status = d.add(n_pairs * 4 + 4), s_work = d.add(TXQ_EDIT_TARGETS_WORKSPACE(n_pairs, n_slots));
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
                    d.at<uint64_t>(s_grp), n_groups, d.at<uint32_t>(s_pairs), n_pairs, d.at<uint8_t>(s_codes), d.at<uint32_t>(s_hits), capacity,
                    d.at<uint64_t>(s_total), d.at<uint32_t>(s_status), n_slots, d.at<void>(s_work), nullptr);
    if (rc == TXQ_OK) {
        d.download(total, s_total, 8);  // (waits for the kernels)
        d.download(status, s_status, n_pairs * 4);
        if (d.error() == hipSuccess) d.download(hits, s_hits, (size_t)(*total < capacity ? *total : capacity) * 16);
    }
    if (d.error() != hipSuccess) return fail_hip(d.error(), who);
    return rc;
}

}  // namespace
}  // namespace txq

using namespace txq;

extern "C" {

int txq_edit_targets_device(const uint8_t* d_patterns, const uint64_t* d_pat_offsets, size_t n_patterns, size_t pattern_bytes,
                            const uint8_t* d_text, const uint64_t* d_rec_offsets, size_t n_records, size_t text_bytes,
                            const uint64_t* d_group_offsets, size_t n_groups, const uint32_t* d_pairs, size_t n_pairs,
                            const uint8_t* d_codes, uint32_t* d_hits, size_t capacity, uint64_t* d_total, uint32_t* d_status, size_t n_slots,
                            void* d_workspace, void* stream) {
    return targets_device<kShortMax>(d_patterns, d_pat_offsets, n_patterns, pattern_bytes, d_text, d_rec_offsets, n_records, text_bytes, d_group_offsets,
                                     n_groups, d_pairs, n_pairs, d_codes, d_hits, capacity, d_total, d_status, n_slots, d_workspace, stream);
}

int txq_edit_targets_long_device(const uint8_t* d_patterns, const uint64_t* d_pat_offsets, size_t n_patterns, size_t pattern_bytes,
                                 const uint8_t* d_text, const uint64_t* d_rec_offsets, size_t n_records, size_t text_bytes,
                                 const uint64_t* d_group_offsets, size_t n_groups, const uint32_t* d_pairs, size_t n_pairs,
                                 const uint8_t* d_codes, uint32_t* d_hits, size_t capacity, uint64_t* d_total, uint32_t* d_status, size_t n_slots,
                                 void* d_workspace, void* stream) {
    return targets_device<kLongMax>(d_patterns, d_pat_offsets, n_patterns, pattern_bytes, d_text, d_rec_offsets, n_records, text_bytes, d_group_offsets,
                                    n_groups, d_pairs, n_pairs, d_codes, d_hits, capacity, d_total, d_status, n_slots, d_workspace, stream);
}

int txq_edit_targets(const uint8_t* patterns, const uint64_t* pat_offsets, size_t n_patterns, const uint8_t* text, const uint64_t* rec_offsets,
                     size_t n_records, const uint64_t* group_offsets, size_t n_groups, const uint32_t* pairs, size_t n_pairs, const uint8_t* codes,
                     uint32_t* hits, size_t capacity, uint64_t* total, uint32_t* status, size_t n_slots) {
    return targets_staged(patterns, pat_offsets, n_patterns, text, rec_offsets, n_records, group_offsets, n_groups, pairs, n_pairs, codes, hits, capacity,
                          total, status, n_slots, kShortMax, txq_edit_targets_device, "txq_edit_targets copies");
}

int txq_edit_targets_long(const uint8_t* patterns, const uint64_t* pat_offsets, size_t n_patterns, const uint8_t* text, const uint64_t* rec_offsets,
                          size_t n_records, const uint64_t* group_offsets, size_t n_groups, const uint32_t* pairs, size_t n_pairs, const uint8_t* codes,
                          uint32_t* hits, size_t capacity, uint64_t* total, uint32_t* status, size_t n_slots) {
    return targets_staged(patterns, pat_offsets, n_patterns, text, rec_offsets, n_records, group_offsets, n_groups, pairs, n_pairs, codes, hits, capacity,
                          total, status, n_slots, kLongMax, txq_edit_targets_long_device, "txq_edit_targets_long copies");
}

}  // extern "C"
