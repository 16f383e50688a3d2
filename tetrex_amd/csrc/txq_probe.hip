// Flat-IBF kernels for gfx950: batched bulk_contains ("probe") and device-side emplace.
//
// probe: k-mer -> h row indices (seqan::hibf hash_and_fit) -> gather h bin-wide bit rows ->
// 64-bit AND -> per-bin hit mask.  Replaces seqan::hibf containment_agent::bulk_contains as
// called from the reference at include/index_ibf.h:146-150.
//
// Mapping to the machine (wave = 64 lanes):
//   * a wave owns a tile of 64 consecutive k-mers; lane l hashes k-mer l ONCE (h row indices),
//   * a row is moved by LPK lanes x 16 B (global_load_dwordx4); LPK = pow2 >= stride/2, so a
//     128-byte row (1024 bins) takes 8 lanes and a wave gathers 8 k-mers x h rows per step,
//   * the row indices travel from the hashing lane to the gathering lane group by ds_bpermute
//     (__shfl), no LDS allocation, no redundant 64-bit multiplies,
//   * two steps are in flight at a time (2*h independent 16-byte gathers per lane before the
//     first AND, 94 VGPRs = 5 waves/SIMD); output rows of one step are contiguous (coalesced 1-KiB stores),
//   * `alive` (mask != 0, the collector's path_.none() test) falls out of one __ballot per step.
// Algorithmic HBM bytes per probe: h*W*8 (rows) + W*8 (mask) + 8 (k-mer); W = shard_words.
//
// Domain table (probe_flat, the path of txq_probe_device on a flat IBF): a batch whose values lie in a domain [0, D)
// several times smaller than the batch holds each value n/D times, and every repeat gathers the same h rows again.  The row
// T[v] = bulk_contains(v) depends on the index's bits and on nothing in the batch, so the table is kept with the index from
// call to call and only EXTENDED: a device word `valid` says that rows [0, valid) hold the masks of the current bits.
// A call has one of three shapes (the host decides which, by API call order: txq_probe_plan.hpp plan_probe_call):
//   fresh (first call, table (re)allocated, the index's bits changed - txq_emplace_device counts its calls -, a call before
//   failed, TXQ_PROBE_TABLE_KEEP=0): three launches.
//     1. probe_domain_kernel: a 1/16 sample of the k-mers -> D = 1 + the largest value below the call's capacity, and how
//        many values lie below it (device words; the host gets no answer back, the call stays stream-ordered),
//     2. probe_kernel<..., kBuild>: the values [0, D) probed into the table T[v] (row pitch = stride) - if the domain pays,
//        count * 16 >= ratio * D,
//     3. probe_kernel<..., kAnswer>: the plain kernel's lane layout; a k-mer v < rows reads ONE row T[v], any other k-mer
//        gathers its h rows as above.  A full tile whose 64 k-mers all have a row takes a body of its own (table_tile: no
//        hashing, its row loads back to back in front of its stores; TXQ_PROBE_TABLE_TILE=0: never).
//   kept: ONE launch of probe_kernel<..., kAnswer>, which also does what the other two did.  Every answer counts, exactly and
//     for nothing in the steady state, the k-mers it had to gather although they lie below the call's capacity: a wave that
//     met any adds {1 + the largest, how many} to the call's statistics.  The NEXT kept call reads them: with V = `valid` and
//     E = top if the extension pays (count >= ratio * (top - V)), else V, its k-mers below V read their row, all others
//     gather, and the values [V, E) are probed into the table by the same waves after the batch's tiles (the build's tiles).
//     So an extension takes two calls: call c gathers the new values and counts them, call c + 1 gathers them again and
//     builds their rows, call c + 2 reads them.
//   kept, TXQ_PROBE_TABLE_FUSED=0: the three launches of a fresh call, on the rows the table holds (build [valid, D)).
// One thread of every answer leaves `valid` = the rows valid after the call behind, and zeroes the words the next call adds
// into.  `valid` has two copies, used alternately: a one-launch call writes the rows [V, E) in the launch that publishes E,
// and a wave that read E there would read rows not yet written.  The statistics have three slots (add, read, zero).  No
// state word is read by the waves of a launch and written in the same launch (txq_probe_plan.hpp probe_slots).
//   kept, sorted (txq_probe_plan.hpp plan_probe_sort: one launch, no `alive`, rows of 16 or 32 whole words, a batch of at least
//     TXQ_PROBE_SORT_MIN k-mers; TXQ_PROBE_SORT=0: never): three launches in front of the answer partition the batch into value
//     buckets v >> shift, a bucket's rows about 1 MB of the table - probe_sort_count_kernel (a histogram per chunk of 4096
//     k-mers; a k-mer at or above `valid` sets the call's `outside` flag), probe_sort_scan_kernel (offsets per bucket and chunk),
//     probe_sort_scatter_kernel (records v << 32 | position, in bucket order).  The answer (probe_sorted_answer_kernel: the
//     same body, an instance of its own so that every other answer keeps its registers) then takes its tiles from the
//     records: workgroup b the tiles (b % 8) * tiles_per_xcd + (b / 8) * 4 + wave, so that XCD b % 8 walks one contiguous eighth
//     of them and its L2 holds the rows it reads; a tile stores to the rows its records name.  With `outside` set (and with
//     valid == 0, where count does not even read the batch) scan and scatter leave at once and the answer runs in batch order.
//     A sorted answer meets no k-mer at or above `valid`: it adds nothing to the statistics, and builds [V, E) like any other.
// Per probe of the answer: 8 (k-mer) + W*8 (table row) + W*8 (mask); a sorted call 32 more (k-mer twice, record twice); a fresh call n/2 bytes of sample, and per new row
// h*W*8 + W*8 to extend the table.
#include "txq_internal.hpp"
#include "txq_probe_plan.hpp"
#include <algorithm>
#include <cstdlib>

namespace txq {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ u32x4 ld16(const uint64_t* p) { return *reinterpret_cast<const u32x4*>(p); }
__device__ __forceinline__ void st16_stream(uint64_t* p, u32x4 v) {
    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
}
__device__ __forceinline__ bool nonzero(u32x4 v) { return (v.x | v.y | v.z | v.w) != 0u; }

__device__ __forceinline__ void store_chunk(const IbfDev& f, uint64_t* masks, size_t kidx, uint32_t c, u32x4 acc) {
    uint64_t* dst = masks + kidx * f.shard_words + 2u * c;
    if (2u * c + 1u < f.shard_words) st16_stream(dst, acc);
    else __builtin_nontemporal_store(((uint64_t)acc.y << 32) | acc.x, dst);  // odd tail word
}

// Where the matrix is the interleaved children of a small regular HIBF (Index::interleaved: row r of every child side by
// side), the root's rows decide which children's words survive: the hashing lane gathers the root word of its k-mer
// (at most 64 merged bins) and hands it to the gathering lanes with the row indices.
struct NoRoot { static constexpr bool kActive = false; };
struct TreeRoot {
    static constexpr bool kActive = true;
    HibfNode root;
    const ChildRec* children;  // in mask-column order; packed >> 12 = the child's merged bin in the root
    uint32_t wpr_log2;         // log2(mask words per child)
};

// The domain table of one call (see the header).  state: the words the kernels keep beside the table (txq_probe_plan.hpp
// kState..., probe_slots): `slot` says which of them this call reads, adds into, stores and zeroes.
struct TableArgs {
    uint64_t* table;  // T[v] at table + v * stride, v < rows
    uint32_t* state;
    uint32_t ratio, cap_rows;
    uint32_t cap;             // this call's capacity: the answer counts the k-mers in [rows, cap) it had to gather
    uint32_t fresh, sampled;  // sampled: a domain pass and a build ran in front of the answer (fresh calls, TXQ_PROBE_TABLE_FUSED=0)
    ProbeSlots slot;
    uint32_t experiment;      // TXQ_EXPERIMENTS builds only (TXQ_PROBE_EXPERIMENT: timing experiments, wrong masks)
    uint32_t table_tile;      // a full tile whose 64 k-mers all have a row takes table_tile (TXQ_PROBE_TABLE_TILE=0: never)
    // the sorted answer (txq_probe_plan.hpp plan_probe_sort; records == nullptr: none): the batch's records in bucket order,
    // the remap of its tiles, and this call's / the next call's `outside` flag
    const uint64_t* records;
    uint32_t tiles_per_xcd, sort_blocks;
    uint32_t outside, outside_zero;
};
// the rows of a sampled call: the build writes [lo, rows), its answer reads [0, rows)
__device__ __forceinline__ ProbeRows table_rows(const TableArgs& T) {
    const uint32_t* acc = T.state + T.slot.acc;
    return table_rows(T.fresh != 0, T.state[T.slot.valid_read], acc[0], acc[1], T.ratio, kDomainSample, T.cap_rows);
}
// the rows of an answer: k-mers below `valid` read their row, the launch itself builds [valid, rows) (a sampled call: nothing)
__device__ __forceinline__ ProbeExtend answer_rows(const TableArgs& T) {
    if (T.sampled) {
        const uint32_t rows = table_rows(T).rows;
        return ProbeExtend{rows, rows};
    }
    const uint32_t* stat = T.state + T.slot.stat_read;
    return extend_rows(T.state[T.slot.valid_read], stat[0], stat[1], T.ratio, T.cap_rows);
}
enum ProbeMode { kPlain = 0, kBuild = 1, kAnswer = 2 };

// What an answering wave learns about its k-mers in [rows, cap): 1 + the largest, and how many (wave-uniform).
struct WaveStats { uint32_t top = 0, count = 0; };

// One tile of probe_kernel: 64 consecutive k-mers, one wave.  LPK lanes per k-mer, H hash functions, U steps in flight.
// U*H independent 16-byte gathers per lane are issued before the first AND.
// MODE kBuild: the k-mers are the values of the tile themselves (no input), of which [lo, n) are written to `masks` = the table
// at row pitch stride (whole 16-byte chunks, plain stores: an answer reads them back); MODE kAnswer: k-mers below `tab_rows`
// read their row of `table` instead of gathering, and those in [cnt_lo, cnt_hi) are counted into `st`; the caller has
// loaded the tile's k-mers (v_in: lane l holds k-mer l, 0 past n).
template <int LPK, int H, int U, bool NT, class ROOT, int MODE>
__device__ __forceinline__ void probe_tile(const IbfDev& f, const uint64_t* __restrict__ kmers, size_t n, uint64_t* __restrict__ masks,
                                           uint64_t* __restrict__ alive, const ROOT& R, const uint64_t* __restrict__ table, uint32_t tab_rows,
                                           uint32_t lo, uint32_t cnt_lo, uint32_t cnt_hi, WaveStats& st, uint32_t experiment, size_t tile, uint64_t v_in = 0) {
    constexpr int KPS = 64 / LPK;          // k-mers per step
    constexpr int UU = U < LPK ? U : LPK;  // a tile has LPK steps
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPK, grp = lane / LPK;
    const uint32_t chunks = f.stride >> 1;
    (void)experiment;
    {
        const size_t base = tile << 6;
        const size_t mine = base + lane;
        const uint64_t v = MODE == kBuild ? (uint64_t)mine : MODE == kAnswer ? v_in : mine < n ? __builtin_nontemporal_load(kmers + mine) : 0;
        const bool tab = MODE == kAnswer && mine < n && v < tab_rows;  // my k-mer's mask is row v of the table
        if constexpr (MODE == kAnswer) {
            const bool beyond = mine < n && v >= cnt_lo && v < cnt_hi;
            const uint64_t b = __ballot(beyond);
            if (b) {  // (in the steady state never)
                uint32_t t = beyond ? (uint32_t)v + 1u : 0u;
                for (int o = 32; o > 0; o >>= 1) t = max(t, (uint32_t)__shfl_xor((int)t, o));
                st.top = max(st.top, (uint32_t)__builtin_amdgcn_readfirstlane((int)t));
                st.count += (uint32_t)__popcll(b);
            }
        }
        uint32_t row[H];
        if (tab) {
            row[0] = (uint32_t)v;
#pragma unroll
            for (int i = 1; i < H; ++i) row[i] = 0;
        } else {
#pragma unroll
            for (int i = 0; i < H; ++i) row[i] = (uint32_t)hash_row(v, kSeeds[i], f.hash_shift, f.bin_size);
        }
        const uint64_t tab_lanes = MODE == kAnswer ? __ballot(tab) : 0;
        uint32_t root_lo = ~0u, root_hi = ~0u;  // the root's verdict on my k-mer: bit b = it may be in the child behind merged bin b
        if constexpr (ROOT::kActive) {
            const uint64_t* rw = (const uint64_t*)R.root.words;
            uint64_t x = ~0ULL;
            for (uint32_t i = 0; i < R.root.hash_funs(); ++i)
                x &= rw[hash_row_seeded(v * kSeeds[i], R.root.hash_shift(), R.root.bin_size) * R.root.stride()];
            root_lo = (uint32_t)x;
            root_hi = (uint32_t)(x >> 32);
        }
#ifdef TXQ_EXPERIMENTS
        uint32_t sink = 0;  // (experiment bit 1: what the loads gave, one word per wave instead of the masks)
#endif
        bool my_alive = false;
        for (int s = 0; s < LPK; s += UU) {
            uint32_t r[UU][H];
#pragma unroll
            for (int u = 0; u < UU; ++u)
#pragma unroll
                for (int i = 0; i < H; ++i) r[u][i] = __shfl(row[i], (s + u) * KPS + grp);
            uint64_t verdict[UU];
            if constexpr (ROOT::kActive) {
#pragma unroll
                for (int u = 0; u < UU; ++u)
                    verdict[u] = ((uint64_t)(uint32_t)__shfl((int)root_hi, (s + u) * KPS + grp) << 32) | (uint32_t)__shfl((int)root_lo, (s + u) * KPS + grp);
            }
            bool nz[UU];
#pragma unroll
            for (int u = 0; u < UU; ++u) nz[u] = false;
            for (uint32_t c = sub; c < chunks; c += LPK) {
                uint32_t bin0 = 0, bin1 = 0;  // merged bins of the children behind words 2c and 2c + 1
                if constexpr (ROOT::kActive) {
                    bin0 = R.children[(2u * c) >> R.wpr_log2].packed >> 12;
                    bin1 = 2u * c + 1u < f.shard_words ? R.children[(2u * c + 1u) >> R.wpr_log2].packed >> 12 : bin0;
                }
                u32x4 x[UU][H];
#pragma unroll
                for (int u = 0; u < UU; ++u) {
                    const bool t = MODE == kAnswer && ((tab_lanes >> ((s + u) * KPS + grp)) & 1ULL);
#pragma unroll
                    for (int i = 0; i < H; ++i) {
                        if (MODE == kAnswer && t && i > 0) {
                            x[u][i] = u32x4{~0u, ~0u, ~0u, ~0u};
                            continue;
                        }
#ifdef TXQ_EXPERIMENTS
                        if (MODE == kAnswer && (experiment & 1u)) {  // no table or row loads: the mask is a constant
                            x[u][i] = u32x4{0x55555555u, 0x33333333u, 0x0f0f0f0fu, 0x00ff00ffu};
                            continue;
                        }
#endif
                        const uint64_t* p = (MODE == kAnswer && t ? table : f.words) + (size_t)r[u][i] * f.stride + 2u * c;
                        x[u][i] = NT ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)) : ld16(p);
                    }
                }
#pragma unroll
                for (int u = 0; u < UU; ++u) {
                    u32x4 acc = x[u][0];
#pragma unroll
                    for (int i = 1; i < H; ++i) acc &= x[u][i];
                    if constexpr (ROOT::kActive) {
                        const uint32_t m0 = (verdict[u] >> bin0) & 1ULL ? ~0u : 0u, m1 = (verdict[u] >> bin1) & 1ULL ? ~0u : 0u;
                        acc.x &= m0; acc.y &= m0; acc.z &= m1; acc.w &= m1;
                    }
                    const size_t kidx = base + (s + u) * KPS + grp;
#ifdef TXQ_EXPERIMENTS
                    if (MODE == kAnswer && (experiment & 2u)) {  // no mask stores
                        sink ^= acc.x ^ acc.y ^ acc.z ^ acc.w;
                        nz[u] |= nonzero(acc);
                        continue;
                    }
#endif
                    if (MODE == kBuild) {
                        if (kidx >= lo && kidx < n) *reinterpret_cast<u32x4*>(masks + kidx * f.stride + 2u * c) = acc;
                    } else if (kidx < n) store_chunk(f, masks, kidx, c, acc);
                    nz[u] |= nonzero(acc);
                }
            }
            if (alive) {
                const uint64_t gm = LPK == 64 ? ~0ULL : ((1ULL << LPK) - 1ULL);
                const int my_step = lane / KPS, my_grp = lane % KPS;
#pragma unroll
                for (int u = 0; u < UU; ++u) {
                    const uint64_t b = __ballot(nz[u]);
                    if (my_step == s + u) my_alive = ((b >> (my_grp * LPK)) & gm) != 0;
                }
            }
        }
        if (alive) {
            const uint64_t bits = __ballot(my_alive && mine < n);
            if (lane == 0) alive[tile] = bits;
        }
#ifdef TXQ_EXPERIMENTS
        if (MODE == kAnswer && (experiment & 2u)) {
            const uint64_t bits = __ballot(sink & 1u);
            if (lane == 0) masks[base * f.shard_words] = bits;
        }
#endif
    }
}

// One full tile of an answer whose 64 k-mers all have a row in the table (lane l: row `row`): no hashing, no statistics, no
// choice per lane.  The steps are taken in groups of G = min(LPK, 8): G shuffles of the row index, G 16-byte loads of T[v]
// back to back, then the G stores, then the `alive` ballots.
// Loads and stores share the one in-order vmcnt counter: a wait on loads issued AFTER a store also waits for that store's
// acknowledgement.  Here every load a store depends on is older than every store in flight, so the waits in front of the
// stores can be counted ones that leave the wave's own stores outstanding; with more than one group (LPK > 8) the loads of
// group g + 1 are issued before the stores of group g.
// WHOLE: every lane has a chunk and the row has no odd tail word (chunks == LPK, shard_words even): the body is straight-line
// code, and the compiler's waits are exactly those.  Otherwise the lanes past the row's chunks are masked once around a group's
// loads and once around its stores, and the tail lane stores 8 bytes: behind such a branch the compiler's counted waits assume
// the path WITHOUT the stores, and would wait for earlier stores of the group.  With one group the loads are therefore waited
// for as a whole in front of the stores, which then need no wait at all; with several (LPK > 8 and an odd or masked row) the
// compiler's waits stand.  Requires chunks <= LPK (the caller takes it at LPK <= 16 only).
// SORTED (WHOLE rows, no `alive`): the tile is 64 records of the bucketed batch, lane l: row `row`, written to row `dst` of
// the masks (a second shuffle per step; the rows of a store instruction are then no longer adjacent), of which the first
// `count` exist (RAGGED: count < 64, the last tile; its lanes past `count` load row 0 and store nothing).
template <int LPK, bool WHOLE, bool SORTED = false, bool RAGGED = false>
__device__ __forceinline__ void table_tile(const IbfDev& f, uint64_t* __restrict__ masks, uint64_t* __restrict__ alive,
                                           const uint64_t* __restrict__ table, uint32_t row, uint32_t experiment, size_t tile,
                                           uint32_t dst = 0, uint32_t count = 64) {
    constexpr int KPS = 64 / LPK;
    constexpr int G = LPK < 8 ? LPK : 8;
    constexpr int GROUPS = LPK / G;
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPK, grp = lane / LPK;
    const bool on = WHOLE || (uint32_t)sub < (f.stride >> 1);
    const size_t base = tile << 6;
    const uint64_t gm = LPK == 64 ? ~0ULL : ((1ULL << LPK) - 1ULL);
    const int my_step = lane / KPS, my_grp = lane % KPS;
    (void)experiment;
#ifdef TXQ_EXPERIMENTS
    uint32_t sink = 0;
#endif
    bool my_alive = false;
    u32x4 x[2][G];
    auto load_group = [&](int g, u32x4* out) {
        uint32_t r[G];
#pragma unroll
        for (int u = 0; u < G; ++u) r[u] = (uint32_t)__shfl((int)row, (g * G + u) * KPS + grp);
        if constexpr (!WHOLE) {
#pragma unroll
            for (int u = 0; u < G; ++u) out[u] = u32x4{0u, 0u, 0u, 0u};
        }
#ifdef TXQ_EXPERIMENTS
        if (experiment & 1u) {  // no row loads: the mask is a constant
#pragma unroll
            for (int u = 0; u < G; ++u) out[u] = u32x4{0x55555555u, 0x33333333u, 0x0f0f0f0fu, 0x00ff00ffu};
            return;
        }
#endif
        if (on) {
#pragma unroll
            for (int u = 0; u < G; ++u) out[u] = ld16(table + (size_t)r[u] * f.stride + 2u * sub);
        }
    };
    load_group(0, x[0]);
#pragma unroll
    for (int g = 0; g < GROUPS; ++g) {
        if (g + 1 < GROUPS) load_group(g + 1, x[(g + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);  // (left alone, the scheduler sinks loads of the group between the stores before it)
        const u32x4* cur = x[g & 1];
        if constexpr (!WHOLE && GROUPS == 1) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the group's loads, nothing else is in flight
#ifdef TXQ_EXPERIMENTS
        if (experiment & 2u) {  // no mask stores
#pragma unroll
            for (int u = 0; u < G; ++u) sink ^= cur[u].x ^ cur[u].y ^ cur[u].z ^ cur[u].w;
        } else
#endif
        if constexpr (SORTED) {
            // (the destination rows are shuffled here, not with the row indices: a second group's would cost LPK 16 its fourth wave)
            uint32_t to[G];
#pragma unroll
            for (int u = 0; u < G; ++u) to[u] = (uint32_t)__shfl((int)dst, (g * G + u) * KPS + grp);
#pragma unroll
            for (int u = 0; u < G; ++u)
                if (!RAGGED || (uint32_t)((g * G + u) * KPS + grp) < count) st16_stream(masks + (size_t)to[u] * f.shard_words + 2u * sub, cur[u]);
        } else if constexpr (WHOLE) {
#pragma unroll
            for (int u = 0; u < G; ++u) st16_stream(masks + (base + (g * G + u) * KPS + grp) * f.shard_words + 2u * sub, cur[u]);
        } else if (on) {
#pragma unroll
            for (int u = 0; u < G; ++u) store_chunk(f, masks, base + (g * G + u) * KPS + grp, sub, cur[u]);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (!SORTED && alive) {
#pragma unroll
            for (int u = 0; u < G; ++u) {
                const uint64_t b = __ballot(on && nonzero(cur[u]));
                if (my_step == g * G + u) my_alive = ((b >> (my_grp * LPK)) & gm) != 0;
            }
        }
    }
    if (!SORTED && alive) {
        const uint64_t bits = __ballot(my_alive);
        if (lane == 0) alive[tile] = bits;
    }
#ifdef TXQ_EXPERIMENTS
    if (experiment & 2u) {
        const uint64_t bits = __ballot(sink & 1u);
        if (lane == 0) masks[base * f.shard_words] = bits;
    }
#endif
}

// The tiles of a sorted answer (answer_body below): workgroup b, b + gridDim.x, ... of the plan's workgroups takes tile
// (b % 8) * tiles_per_xcd + (b / 8) * 4 + wave of the records.  Every record's value lies below `valid`.
template <int LPK>
__device__ __forceinline__ void sorted_tiles(const IbfDev& f, size_t n, uint64_t* __restrict__ masks, const TableArgs& T) {
    const size_t n_tiles = (n + 63) >> 6;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t b = blockIdx.x; b < T.sort_blocks; b += gridDim.x) {
        const size_t tile = (size_t)(b % kSortXcds) * T.tiles_per_xcd + (size_t)(b / kSortXcds) * 4u + wave;
        if (tile >= n_tiles) continue;
        const size_t mine = (tile << 6) + lane;
        if ((tile << 6) + 64 <= n) {
            const uint64_t rec = __builtin_nontemporal_load(T.records + mine);
            table_tile<LPK, true, true, false>(f, masks, nullptr, T.table, (uint32_t)(rec >> 32), T.experiment, tile, (uint32_t)rec);
        } else {
            const uint64_t rec = mine < n ? __builtin_nontemporal_load(T.records + mine) : 0;
            table_tile<LPK, true, true, true>(f, masks, nullptr, T.table, (uint32_t)(rec >> 32), T.experiment, tile, (uint32_t)rec,
                                                       (uint32_t)(n - (tile << 6)));
        }
    }
}

// The answer of a table call (probe_kernel<..., kAnswer> and probe_sorted_answer_kernel below): the batch's tiles read the
// table below `valid` - a full tile that lies below it as a whole through table_tile, any other (the ragged last tile, a
// k-mer at or above `valid`, a tree root) through probe_tile; then the tiles of the values [valid, rows) of answer_rows are
// built into T.table as a second loop of the same waves (its registers are the larger of the two bodies, not their sum) -
// nothing in a sampled call, whose build ran before.  Each wave that met k-mers in [rows, cap) adds them to this call's
// statistics, and one thread leaves behind what the next call reads: `valid` = rows in the copy this launch does not read,
// and the next call's statistics, sample words and `outside` flag zeroed.
// SORT: the batch was bucketed in front of this launch (T.records); if none of its k-mers lies at or above `valid` the tiles
// are those of the records (sorted_tiles), else the in-order loop runs as if nothing had been bucketed.
template <int LPK, int H, int U, bool NT, class ROOT, bool SORT>
__device__ __forceinline__ void answer_body(const IbfDev& f, const uint64_t* __restrict__ kmers, size_t n, uint64_t* __restrict__ masks,
                                            uint64_t* __restrict__ alive, const ROOT& R, const TableArgs& T) {
    const size_t wave = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const size_t n_waves = (size_t)gridDim.x * (blockDim.x >> 6);
    WaveStats st;
    const ProbeExtend ex = answer_rows(T);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        T.state[T.slot.valid_write] = ex.rows;
        T.state[T.slot.stat_zero] = 0;
        T.state[T.slot.stat_zero + 1] = 0;
        T.state[T.slot.acc_zero] = 0;
        T.state[T.slot.acc_zero + 1] = 0;
        T.state[T.outside_zero] = 0;
    }
    const size_t n_tiles = (n + 63) >> 6;
    // (rows of up to 32 words only: at LPK 32 and 64 the body's two row buffers cost the kernel 1 to 4 waves/SIMD and
    // measured no gain, profiles/probe_table_tile_ab.txt)
    constexpr bool kTableTile = !ROOT::kActive && LPK <= 16;
    const bool tile_ok = kTableTile && T.table_tile && ex.valid;
    const bool whole = (f.stride >> 1) == (uint32_t)LPK && !(f.shard_words & 1u);
    bool sorted = false;
    if constexpr (SORT) {
        sorted = T.state[T.outside] == 0;
        if (sorted) {
            if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(T.state + kStateSorted, 1u);
            sorted_tiles<LPK>(f, n, masks, T);
        }
    }
    for (size_t tile = sorted ? n_tiles : wave; tile < n_tiles; tile += n_waves) {
        const size_t mine = (tile << 6) + (threadIdx.x & 63);
        const uint64_t v = mine < n ? __builtin_nontemporal_load(kmers + mine) : 0;
        if constexpr (kTableTile) {
            if (tile_ok && (tile << 6) + 64 <= n && __ballot(v < ex.valid) == ~0ULL) {
                if (whole) table_tile<LPK, true>(f, masks, alive, T.table, (uint32_t)v, T.experiment, tile);
                else table_tile<LPK, false>(f, masks, alive, T.table, (uint32_t)v, T.experiment, tile);
                continue;
            }
        }
        probe_tile<LPK, H, U, NT, ROOT, kAnswer>(f, kmers, n, masks, alive, R, T.table, ex.valid, 0, ex.rows, T.cap, st, T.experiment, tile, v);
    }
    if (st.count && (threadIdx.x & 63) == 0) {
        atomicMax(T.state + T.slot.stat_add, st.top);
        atomicAdd(T.state + T.slot.stat_add + 1, st.count);
    }
    const size_t x_tiles = ((size_t)ex.rows + 63) >> 6;
    for (size_t tile = (ex.valid >> 6) + wave; tile < x_tiles; tile += n_waves)
        probe_tile<LPK, H, U, NT, ROOT, kBuild>(f, nullptr, ex.rows, T.table, nullptr, R, nullptr, 0, ex.valid, 0, 0, st, 0, tile);
}

// A wave owns the tiles wave, wave + n_waves, ... of the batch.  Requires bin_size < 2^32 and an even stride.
// MODE kBuild: the tiles are those of the values [lo, rows) of table_rows, written to T.table.
// MODE kAnswer: answer_body, in batch order.
template <int LPK, int H, int U, bool NT, class ROOT = NoRoot, int MODE = kPlain>
__global__ __launch_bounds__(256) void probe_kernel(IbfDev f, const uint64_t* __restrict__ kmers, size_t n,
                                                    uint64_t* __restrict__ masks, uint64_t* __restrict__ alive, ROOT R = ROOT{},
                                                    TableArgs T = TableArgs{}) {
    const size_t wave = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const size_t n_waves = (size_t)gridDim.x * (blockDim.x >> 6);
    WaveStats st;
    if constexpr (MODE == kPlain) {
        const size_t n_tiles = (n + 63) >> 6;
        for (size_t tile = wave; tile < n_tiles; tile += n_waves)
            probe_tile<LPK, H, U, NT, ROOT, kPlain>(f, kmers, n, masks, alive, R, nullptr, 0, 0, 0, 0, st, 0, tile);
    } else if constexpr (MODE == kBuild) {
        const ProbeRows tr = table_rows(T);
        const size_t n_tiles = ((size_t)tr.rows + 63) >> 6;
        for (size_t tile = (tr.lo >> 6) + wave; tile < n_tiles; tile += n_waves)
            probe_tile<LPK, H, U, NT, ROOT, kBuild>(f, nullptr, tr.rows, T.table, nullptr, R, nullptr, 0, tr.lo, 0, 0, st, 0, tile);
    } else {
        (void)wave, (void)n_waves, (void)st;
        answer_body<LPK, H, U, NT, ROOT, false>(f, kmers, n, masks, alive, R, T);
    }
}

// The answer of a call whose batch was bucketed (plan_probe_sort: LPK 8 or 16, no `alive`, no root): the same body with the
// sorted tiles compiled in - an instance of its own, so that every other answer keeps the registers it had.  It is held to
// the waves per SIMD of the answer it stands in for (profiles/probe_sorted_resource_usage.txt): left alone, LPK 16 with 3 and
// 5 hash functions took 130 VGPRs, two more than four waves allow.
constexpr int sorted_answer_waves(int lpk, int h) { return lpk == 16 && h == 2 ? 2 : (lpk == 8 && h == 5) || (lpk == 16 && h == 4) ? 3 : 4; }
template <int LPK, int H>
__global__ __launch_bounds__(256, sorted_answer_waves(LPK, H)) void probe_sorted_answer_kernel(IbfDev f, const uint64_t* __restrict__ kmers, size_t n, uint64_t* __restrict__ masks,
                                                                  TableArgs T) {
    answer_body<LPK, H, 2, false, NoRoot, true>(f, kmers, n, masks, nullptr, NoRoot{}, T);
}

// <= 64 bins in this shard: one 8-byte word per row, one lane per k-mer.
template <int H>
__global__ __launch_bounds__(256) void probe_w1_kernel(IbfDev f, const uint64_t* __restrict__ kmers, size_t n,
                                                       uint64_t* __restrict__ masks, uint64_t* __restrict__ alive) {
    const size_t stride_threads = (size_t)gridDim.x * blockDim.x;
    const size_t n_pad = (n + 63) & ~(size_t)63;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad; i += stride_threads) {
        uint64_t acc = 0;
        if (i < n) {
            const uint64_t v = kmers[i];
            uint64_t w[H];
#pragma unroll
            for (int j = 0; j < H; ++j) w[j] = f.words[hash_row(v, kSeeds[j], f.hash_shift, f.bin_size) * f.stride];
            acc = w[0];
#pragma unroll
            for (int j = 1; j < H; ++j) acc &= w[j];
            masks[i] = acc;
        }
        if (alive) {
            const uint64_t bits = __ballot(acc != 0);
            if ((threadIdx.x & 63) == 0) alive[i >> 6] = bits;
        }
    }
}

// Fallback for rows >= 2^32 (row index needs 64 bits): one wave per k-mer, lanes sweep the row.
template <int H>
__global__ __launch_bounds__(256) void probe_bigrows_kernel(IbfDev f, const uint64_t* __restrict__ kmers, size_t n,
                                                            uint64_t* __restrict__ masks, uint64_t* __restrict__ alive) {
    const int lane = threadIdx.x & 63;
    const size_t n_waves = (size_t)gridDim.x * (blockDim.x >> 6);
    for (size_t k = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); k < n; k += n_waves) {
        const uint64_t v = kmers[k];
        uint64_t row[H];
#pragma unroll
        for (int j = 0; j < H; ++j) row[j] = hash_row(v, kSeeds[j], f.hash_shift, f.bin_size);
        bool nz = false;
        for (uint32_t w = lane; w < f.shard_words; w += 64) {
            uint64_t acc = f.words[row[0] * f.stride + w];
#pragma unroll
            for (int j = 1; j < H; ++j) acc &= f.words[row[j] * f.stride + w];
            masks[k * f.shard_words + w] = acc;
            nz |= acc != 0;
        }
        if (alive) {
            const bool any = __ballot(nz) != 0;
            if (lane == 0 && any) atomicOr((unsigned long long*)(alive + (k >> 6)), 1ULL << (k & 63));
        }
    }
}

// emplace: value i -> bin bins_of[i]; sets h bits with atomicOr (idempotent, order-free).
__global__ __launch_bounds__(256) void emplace_kernel(IbfDev f, const uint64_t* __restrict__ values,
                                                      const uint32_t* __restrict__ bins_of, size_t n) {
    const size_t stride_threads = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride_threads) {
        const uint32_t bin = bins_of[i];
        const uint32_t w = bin >> 6;
        if (bin >= f.bins || w < f.word0 || w >= f.word0 + f.shard_words) continue;
        const uint64_t v = values[i];
        const unsigned long long bit = 1ULL << (bin & 63);
        for (uint32_t j = 0; j < f.hash_funs; ++j) {
            const uint64_t r = hash_row(v, kSeeds[j], f.hash_shift, f.bin_size);
            atomicOr((unsigned long long*)(f.words + r * f.stride + (w - f.word0)), bit);
        }
    }
}

// The domain pass of the table path: acc[0] = max(v + 1), acc[1] = count over the k-mers v < cap of a SAMPLE (acc zeroed
// by the call before): the head of each of `segs` equal segments of the batch, 1 / kDomainSample of it in all.  A head is
// shared by `parts` blocks (blockIdx.x = segment * parts + part), so that a thread has at most kDomainLoads k-mers and
// issues their loads together; one block per segment had eight dependent loads per thread on the bench batch, 17 us for 8 MB.
// The gate does not decide correctness (a k-mer the sample missed, v >= D, gathers its rows), so a sample is enough, and
// a batch whose domain does not pay costs a few microseconds rather than a pass over all its k-mers.
static constexpr int kDomainLoads = 4;
__global__ __launch_bounds__(256) void probe_domain_kernel(const uint64_t* __restrict__ kmers, size_t n, uint32_t cap, uint32_t segs, uint32_t parts,
                                                           uint32_t* __restrict__ acc) {
    uint32_t top = 0, count = 0;
    const uint32_t seg = blockIdx.x / parts, part = blockIdx.x % parts;
    const size_t lo = n * seg / segs, hi = n * (seg + 1) / segs;
    const size_t end = lo + (hi - lo + kDomainSample - 1) / kDomainSample;
    for (size_t i0 = lo + (size_t)part * (256 * kDomainLoads) + threadIdx.x; i0 < end; i0 += (size_t)parts * (256 * kDomainLoads)) {
        uint64_t v[kDomainLoads];
#pragma unroll
        for (int u = 0; u < kDomainLoads; ++u) v[u] = i0 + u * 256 < end ? kmers[i0 + u * 256] : ~0ULL;
#pragma unroll
        for (int u = 0; u < kDomainLoads; ++u)
            if (v[u] < cap) {
                top = max(top, (uint32_t)v[u] + 1u);
                ++count;
            }
    }
    for (int o = 32; o > 0; o >>= 1) {
        top = max(top, (uint32_t)__shfl_xor((int)top, o));
        count += (uint32_t)__shfl_xor((int)count, o);
    }
    __shared__ uint32_t s_top[4], s_count[4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_top[wave] = top;
        s_count[wave] = count;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int waves = blockDim.x >> 6;
        for (int w = 1; w < waves; ++w) {
            top = max(top, s_top[w]);
            count += s_count[w];
        }
        if (top) atomicMax(acc, top);
        if (count) atomicAdd(acc + 1, count);
    }
}

// The partition in front of a sorted answer (txq_probe_plan.hpp plan_probe_sort): three launches, no answer to the host.
// A k-mer is in the domain when v < valid, the `valid` the answer will use (answer_rows).
// counts[bucket * chunks + chunk], and behind them (at buckets * chunks) the buckets' totals.
struct SortArgs {
    uint32_t* counts;
    uint64_t* records;
    uint32_t shift, buckets, chunks;
};
// exclusive scan over the 256 threads of a workgroup (wsum: 4 words of LDS); `total` = the sum over all of them
__device__ __forceinline__ uint32_t block_scan256(uint32_t x, uint32_t* wsum, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
        if ((int)lane >= o) incl += up;
    }
    __syncthreads();  // (wsum may still be read from the scan before)
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
    for (uint32_t w = 0; w < 4; ++w) {
        if (w < wave) before += wsum[w];
        total += wsum[w];
    }
    return before + incl - x;
}
static constexpr int kSortPerThread = kSortChunk / 256;

// workgroup c: the histogram of chunk c over the buckets; a k-mer at or above `valid` sets the call's `outside` flag
__global__ __launch_bounds__(256) void probe_sort_count_kernel(const uint64_t* __restrict__ kmers, size_t n, SortArgs S, TableArgs T) {
    __shared__ uint32_t hist[kSortMaxBuckets];
    const uint32_t valid = answer_rows(T).valid;
    if (valid == 0) {  // no row to read (a batch whose domain never paid): nothing is bucketed, the batch is not even read
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(T.state + T.outside, 1u);
        return;
    }
    hist[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * kSortChunk + threadIdx.x;
    uint64_t v[kSortPerThread];
#pragma unroll
    for (int j = 0; j < kSortPerThread; ++j) v[j] = base + j * 256 < n ? __builtin_nontemporal_load(kmers + base + j * 256) : 0;
    bool out = false;
#pragma unroll
    for (int j = 0; j < kSortPerThread; ++j) {
        if (base + j * 256 >= n) continue;
        if (v[j] < valid) atomicAdd(&hist[(uint32_t)v[j] >> S.shift], 1u);
        else out = true;
    }
    if (__ballot(out) && (threadIdx.x & 63) == 0) atomicOr(T.state + T.outside, 1u);
    __syncthreads();
    if (threadIdx.x < S.buckets) S.counts[(size_t)threadIdx.x * S.chunks + blockIdx.x] = hist[threadIdx.x];
}

// workgroup b: the exclusive prefix sum of bucket b's counts over the chunks, in place, and the bucket's total
// (the count kernel found a k-mer outside: the answer will not read the records, scan and scatter leave at once)
__global__ __launch_bounds__(256) void probe_sort_scan_kernel(SortArgs S, TableArgs T) {
    __shared__ uint32_t wsum[4];
    if (T.state[T.outside]) return;
    uint32_t* row = S.counts + (size_t)blockIdx.x * S.chunks;
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < S.chunks; c0 += 256) {
        const uint32_t c = c0 + threadIdx.x;
        const uint32_t x = c < S.chunks ? row[c] : 0;
        uint32_t total;
        const uint32_t ex = block_scan256(x, wsum, total);
        if (c < S.chunks) row[c] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) S.counts[(size_t)S.buckets * S.chunks + blockIdx.x] = carry;
}

// The chunk once more: its records staged in LDS in bucket order, then written so that each bucket's run of the chunk is
// contiguous in the records (the order inside a bucket: whatever the LDS atomics gave).
__global__ __launch_bounds__(256) void probe_sort_scatter_kernel(const uint64_t* __restrict__ kmers, size_t n, SortArgs S, TableArgs T) {
    __shared__ uint32_t hist[kSortMaxBuckets], delta[kSortMaxBuckets], wsum[4];
    __shared__ uint64_t stage[kSortChunk];
    if (T.state[T.outside]) return;
    const uint32_t valid = answer_rows(T).valid;
    hist[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * kSortChunk + threadIdx.x;
    uint64_t v[kSortPerThread];
    uint32_t rank[kSortPerThread];
#pragma unroll
    for (int j = 0; j < kSortPerThread; ++j) v[j] = base + j * 256 < n ? __builtin_nontemporal_load(kmers + base + j * 256) : ~0ULL;
#pragma unroll
    for (int j = 0; j < kSortPerThread; ++j) rank[j] = v[j] < valid ? atomicAdd(&hist[(uint32_t)v[j] >> S.shift], 1u) : 0u;
    __syncthreads();
    const bool mine = threadIdx.x < S.buckets;
    uint32_t total;
    const uint32_t bucket_base = block_scan256(mine ? S.counts[(size_t)S.buckets * S.chunks + threadIdx.x] : 0u, wsum, total);
    const uint32_t local = block_scan256(hist[threadIdx.x], wsum, total);  // total: the chunk's k-mers in the domain
    const uint32_t global = mine ? bucket_base + S.counts[(size_t)threadIdx.x * S.chunks + blockIdx.x] : 0u;
    __syncthreads();
    hist[threadIdx.x] = local;
    delta[threadIdx.x] = global - local;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSortPerThread; ++j)
        if (v[j] < valid) stage[hist[(uint32_t)v[j] >> S.shift] + rank[j]] = (v[j] << 32) | (uint32_t)(base + j * 256);
    __syncthreads();
    for (uint32_t p = threadIdx.x; p < total; p += 256) {
        const uint64_t rec = stage[p];
        S.records[(size_t)(uint32_t)(delta[(uint32_t)(rec >> 32) >> S.shift] + p)] = rec;
    }
}

// ---- launchers --------------------------------------------------------------------------

static inline unsigned grid_for(size_t work_items, unsigned per_block) {
    size_t blocks = (work_items + per_block - 1) / per_block;
    // Up to 256 blocks per CU before the kernels start to grid-stride: letting the dispatcher hand out
    // short blocks balances slightly better than 8 long ones per CU (1024-bin index: +0.6 % cache-resident,
    // within the noise on matrices that miss the Infinity Cache).  TXQ_PROBE_BLOCKS_PER_CU is the A/B knob.
    const size_t per_cu = (size_t)knobs().probe_blocks_per_cu;
    const size_t cap = 256u * (per_cu ? per_cu : 1);
    if (blocks > cap) blocks = cap;
    if (blocks == 0) blocks = 1;
    return (unsigned)blocks;
}

template <int LPK>
static hipError_t launch_lpk(const IbfDev& f, const uint64_t* k, size_t n, uint64_t* m, uint64_t* a, hipStream_t s) {
    const unsigned grid = grid_for((n + 63) / 64, 4);
    // experiment knobs (round 1 tuning): steps in flight and non-temporal row loads
    // (profiles/r1_probe_variants_ab.txt: 1/2/4/8 steps in flight differ by <= 2 % — occupancy already
    // supplies the memory-level parallelism, and 4 steps cost 124 VGPRs = half the waves per SIMD;
    // non-temporal ROW loads cost 20 % on a cache-resident matrix and gain nothing on an 8 GB one.
    // Default: 2 steps in flight, 5 waves/SIMD (94 VGPRs), plain row loads.)
    const int unroll = knobs().probe_unroll;
    const bool nt = knobs().probe_nt;
    if (f.hash_funs == 3 && LPK == 8 && (unroll != 2 || nt)) {
        if (unroll == 1 && !nt) probe_kernel<LPK, 3, 1, false><<<grid, 256, 0, s>>>(f, k, n, m, a);
        else if (unroll == 4 && !nt) probe_kernel<LPK, 3, 4, false><<<grid, 256, 0, s>>>(f, k, n, m, a);
        else if (unroll == 8 && !nt) probe_kernel<LPK, 3, 8, false><<<grid, 256, 0, s>>>(f, k, n, m, a);
        else if (unroll == 2 && nt) probe_kernel<LPK, 3, 2, true><<<grid, 256, 0, s>>>(f, k, n, m, a);
        else if (unroll == 4 && nt) probe_kernel<LPK, 3, 4, true><<<grid, 256, 0, s>>>(f, k, n, m, a);
        else return hipErrorInvalidValue;
        return hipGetLastError();
    }
    if (!with_hash_funs(f.hash_funs, [&](auto h) { probe_kernel<LPK, decltype(h)::value, 2, false><<<grid, 256, 0, s>>>(f, k, n, m, a); }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

void preload_probe_kernels() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&emplace_kernel));
    (void)hipGetLastError();
}

hipError_t launch_probe(const IbfDev& f, const uint64_t* k, size_t n, uint64_t* m, uint64_t* a, hipStream_t s) {
    if (n == 0 || f.shard_words == 0) return hipSuccess;
    if (f.bin_size >> 32) {
        if (a) {
            hipError_t e = hipMemsetAsync(a, 0, ((n + 63) / 64) * 8, s);
            if (e != hipSuccess) return e;
        }
        const unsigned grid = grid_for(n, 4);
        if (!with_hash_funs(f.hash_funs, [&](auto h) { probe_bigrows_kernel<decltype(h)::value><<<grid, 256, 0, s>>>(f, k, n, m, a); }))
            return hipErrorInvalidValue;
        return hipGetLastError();
    }
    if (f.stride == 1) {
        const unsigned grid = grid_for((n + 63) & ~(size_t)63, 256);
        if (!with_hash_funs(f.hash_funs, [&](auto h) { probe_w1_kernel<decltype(h)::value><<<grid, 256, 0, s>>>(f, k, n, m, a); }))
            return hipErrorInvalidValue;
        return hipGetLastError();
    }
    const uint32_t chunks = f.stride >> 1;
    if (chunks <= 1) return launch_lpk<1>(f, k, n, m, a, s);
    if (chunks <= 2) return launch_lpk<2>(f, k, n, m, a, s);
    if (chunks <= 4) return launch_lpk<4>(f, k, n, m, a, s);
    if (chunks <= 8) return launch_lpk<8>(f, k, n, m, a, s);
    if (chunks <= 16) return launch_lpk<16>(f, k, n, m, a, s);
    if (chunks <= 32) return launch_lpk<32>(f, k, n, m, a, s);
    return launch_lpk<64>(f, k, n, m, a, s);
}

// The domain-table path (header comment).  T.ratio: the table is used when at least ratio * D k-mers of the batch lie below D
// (0: whenever D fits the table).  The table holds T.cap_rows >= cap rows; the caller keeps other calls off it until the answer ran.
template <int LPK>
static hipError_t launch_table_lpk(const IbfDev& f, const uint64_t* k, size_t n, uint64_t* m, uint64_t* a, const TableArgs& T, const SortArgs& S,
                                   hipStream_t s) {
    // a build's grid covers the call's capacity (neither `valid` nor D is known on the host); waves with nothing to do leave at once
    const unsigned bgrid = (unsigned)std::min<size_t>(((size_t)T.cap + 255) / 256, kBuildBlocks);
    unsigned grid = grid_for((n + 63) / 64, 4);
    if (T.records) {  // the sorted answer: the batch bucketed first; a grid of a multiple of 8 workgroups, so that b % 8 stays with a workgroup
        probe_sort_count_kernel<<<S.chunks, 256, 0, s>>>(k, n, S, T);
        probe_sort_scan_kernel<<<S.buckets, 256, 0, s>>>(S, T);
        probe_sort_scatter_kernel<<<S.chunks, 256, 0, s>>>(k, n, S, T);
        grid = (std::max(std::min<unsigned>(grid, T.sort_blocks), bgrid) + kSortXcds - 1) / kSortXcds * kSortXcds;
    }
    if (T.sampled) {
        // the sample: the heads of `segs` segments, each shared by as many blocks as give a thread at most kDomainLoads k-mers
        const uint32_t segs = (uint32_t)std::min<size_t>(std::max<size_t>(n / 1024, 1), 512);
        const size_t head = ((n + segs - 1) / segs + kDomainSample - 1) / kDomainSample;
        const uint32_t parts = (uint32_t)std::max<size_t>((head + 256 * kDomainLoads - 1) / (256 * kDomainLoads), 1);
        probe_domain_kernel<<<segs * parts, 256, 0, s>>>(k, n, T.cap, segs, parts, T.state + T.slot.acc);
    }
    // (one hash function: a table row would be the IBF's own row - table_capacity never sends such an index here)
    if (f.hash_funs < 2 || !with_hash_funs(f.hash_funs, [&](auto h) {
            constexpr int H = decltype(h)::value;
            if constexpr (H >= 2) {
                if (T.sampled) probe_kernel<LPK, H, 2, false, NoRoot, kBuild><<<bgrid, 256, 0, s>>>(f, nullptr, 0, T.table, nullptr, NoRoot{}, T);
                // a one-launch call builds too: a small batch that has to build many rows does not do it with a handful of blocks
                if constexpr (LPK == 8 || LPK == 16) {
                    if (T.records) {
                        probe_sorted_answer_kernel<LPK, H><<<grid, 256, 0, s>>>(f, k, n, m, T);
                        return;
                    }
                }
                probe_kernel<LPK, H, 2, false, NoRoot, kAnswer><<<T.sampled ? grid : std::max(grid, bgrid), 256, 0, s>>>(f, k, n, m, a, NoRoot{}, T);
            }
        }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t probe_flat(Index& ix, const Knobs& kn, const uint64_t* k, size_t n, uint64_t* m, uint64_t* a, hipStream_t s) {
    const IbfDev& f = ix.ibf[0];
    const size_t cap = n && f.shard_words ? table_capacity(kn.probe_table, kn.kmer_table_mb, f.bin_size, f.stride, f.hash_funs, n) : 0;
    if (!cap) return launch_probe(f, k, n, m, a, s);
    Index::ProbeTable& pt = ix.probe_table;
    // one table per index: a call on another stream (txq_probe's second stream, another host thread) waits for the
    // answer of the call before it — which may have extended the table this call reads, and zeroed its sample words; the
    // lock keeps (wait, launches, record) of two host threads apart, and txq_emplace_device's change of the bits from both
    std::lock_guard<std::mutex> lock(pt.mutex);
    if (pt.refused) return launch_probe(f, k, n, m, a, s);
    bool reallocated = false;
    if (pt.cap_rows < cap) {
        pt.cap_rows = 0;
        // growing: the kernels of an earlier call may still read the old table
        const auto after_last_call = free_after([&pt] { if (pt.recorded) (void)hipEventSynchronize(pt.done.get()); });
        if (pt.state.reserve(exactly(kStateWords * sizeof(uint32_t)), free_now()) || make(pt.done) != hipSuccess ||
            pt.rows.reserve(exactly(cap * f.stride * 8), after_last_call)) {
            (void)hipGetLastError();  // (out of memory is not an error of this call: the rows are gathered as before)
            pt.refused = true;
            return launch_probe(f, k, n, m, a, s);
        }
        pt.cap_rows = cap;
        reallocated = true;
    }
    if (pt.recorded) {
        hipError_t e = hipStreamWaitEvent(s, pt.done.get(), 0);
        if (e != hipSuccess) return e;
    }
    const ProbeCall call = plan_probe_call(pt.keep, ix.generation, reallocated, kn.probe_table_keep);
    pt.keep.valid = false;  // until this call's launches are through: a call after a failed one zeroes the state words again
    if (call.zero_state) {  // on this call's stream, like everything else: later calls are ordered behind it by `done`
        hipError_t e = hipMemsetAsync(pt.state.get(), 0, kStateWords * sizeof(uint32_t), s);
        if (e != hipSuccess) return e;
        pt.sort_planned = 0;  // (counted on the same base as the device's kStateSorted)
    }
    // a kept call is one launch: the answer counts what it had to gather and builds what the call before counted
    // (TXQ_PROBE_TABLE_FUSED=0: sample, build and answer as in a fresh call, on the rows the table holds)
    const bool sampled = call.fresh || !kn.probe_table_fused;
    const uint32_t chunks = f.stride >> 1;
    const uint32_t lpk = chunks <= 1 ? 1 : chunks <= 2 ? 2 : chunks <= 4 ? 4 : chunks <= 8 ? 8 : chunks <= 16 ? 16 : chunks <= 32 ? 32 : 64;
    // a large kept call is answered from its batch in value-bucket order (txq_probe_plan.hpp plan_probe_sort); scratch that
    // cannot be had is no error, the call is answered in batch order as before
    ProbeSort ps = plan_probe_sort(!sampled && kn.probe_table_tile, a != nullptr, false, lpk, f.stride, f.shard_words, n, pt.cap_rows,
                                   kn.probe_sort && !pt.sort_refused, kn.probe_sort_min, kn.probe_sort_bucket_kb, kn.kmer_table_mb);
    if (ps.on) {
        const auto after_last_call = free_after([&pt] { if (pt.recorded) (void)hipEventSynchronize(pt.done.get()); });
        if (pt.sort_records.reserve(exactly(n * sizeof(uint64_t)), after_last_call) ||
            pt.sort_counts.reserve(exactly(((size_t)ps.buckets * ps.chunks + kSortMaxBuckets) * sizeof(uint32_t)), after_last_call)) {
            (void)hipGetLastError();
            pt.sort_refused = true;
            ps = ProbeSort{};
        }
    }
    const uint32_t parity = (uint32_t)((pt.keep.calls - 1) & 1);
    const TableArgs T{pt.rows.get(), pt.state.get(), kn.probe_table == 1 ? 0u : kTableRatio, (uint32_t)pt.cap_rows, (uint32_t)cap, call.fresh ? 1u : 0u,
                      sampled ? 1u : 0u, probe_slots(pt.keep.calls - 1), (uint32_t)kn.probe_experiment, kn.probe_table_tile ? 1u : 0u,
                      ps.on ? pt.sort_records.get() : nullptr, (uint32_t)ps.tiles_per_xcd, (uint32_t)ps.blocks,
                      kStateOutside + parity, kStateOutside + (parity ^ 1u)};
    const SortArgs S{pt.sort_counts.get(), pt.sort_records.get(), ps.shift, ps.buckets, ps.chunks};
    if (ps.on) ++pt.sort_planned;
    hipError_t e;
    if (chunks <= 1) e = launch_table_lpk<1>(f, k, n, m, a, T, S, s);
    else if (chunks <= 2) e = launch_table_lpk<2>(f, k, n, m, a, T, S, s);
    else if (chunks <= 4) e = launch_table_lpk<4>(f, k, n, m, a, T, S, s);
    else if (chunks <= 8) e = launch_table_lpk<8>(f, k, n, m, a, T, S, s);
    else if (chunks <= 16) e = launch_table_lpk<16>(f, k, n, m, a, T, S, s);
    else if (chunks <= 32) e = launch_table_lpk<32>(f, k, n, m, a, T, S, s);
    else e = launch_table_lpk<64>(f, k, n, m, a, T, S, s);
    if (e != hipSuccess) return e;
    e = hipEventRecord(pt.done.get(), s);
    if (e != hipSuccess) return e;
    pt.recorded = true;
    pt.keep.valid = true;
    return hipSuccess;
}

// the interleaved children of a small regular HIBF (even stride, rows < 2^32, root of at most 64 merged bins)
template <int LPK>
static hipError_t launch_tree_lpk(const IbfDev& f, const TreeRoot& root, const uint64_t* k, size_t n, uint64_t* m, uint64_t* a, hipStream_t s) {
    const unsigned grid = grid_for((n + 63) / 64, 4);
    if (!with_hash_funs(f.hash_funs, [&](auto h) { probe_kernel<LPK, decltype(h)::value, 2, false, TreeRoot><<<grid, 256, 0, s>>>(f, k, n, m, a, root); }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}
hipError_t launch_probe_interleaved(const IbfDev& f, const HibfNode& root, const void* children, uint32_t wpr_log2, const uint64_t* k, size_t n,
                                    uint64_t* m, uint64_t* a, hipStream_t s) {
    if (n == 0 || f.shard_words == 0) return hipSuccess;
    if ((f.bin_size >> 32) || f.stride < 2 || (f.stride & 1) || root.bins > 64) return hipErrorInvalidValue;
    const TreeRoot r{root, (const ChildRec*)children, wpr_log2};
    const uint32_t chunks = f.stride >> 1;
    if (chunks <= 1) return launch_tree_lpk<1>(f, r, k, n, m, a, s);
    if (chunks <= 2) return launch_tree_lpk<2>(f, r, k, n, m, a, s);
    if (chunks <= 4) return launch_tree_lpk<4>(f, r, k, n, m, a, s);
    if (chunks <= 8) return launch_tree_lpk<8>(f, r, k, n, m, a, s);
    if (chunks <= 16) return launch_tree_lpk<16>(f, r, k, n, m, a, s);
    return hipErrorInvalidValue;
}

hipError_t launch_emplace(const IbfDev& f, const uint64_t* values, const uint32_t* bins_of, size_t n, hipStream_t s) {
    if (n == 0 || f.shard_words == 0) return hipSuccess;
    emplace_kernel<<<grid_for(n, 256), 256, 0, s>>>(f, values, bins_of, n);
    return hipGetLastError();
}

}  // namespace txq
