// Which kernel descends an HIBF for a batch of plain k-mers, and the launch arithmetic of each (txq_hibf.hip hibf_probe,
// hibf_probe_fused, layout_order_fused, hibf_probe_layout_order): plain functions on numbers, no HIP call, no Index, no Knobs,
// so that a CPU program can print them (tests/native/hibf_descent_plan_dump.cpp) and tests/hibf_descent_ref.py can restate them.
// The launchers call these and restate nothing; DESIGN.md "HIBF descent: plan and grids" names the caps and the tests that
// pass each of them.
//   descent_path        interleaved probe, child-stationary, small, fused or level-synchronous
//   plan_fused          hibf_fused_kernel<G> in user order: LDS per wave, waves per block, grid, G, w_iters
//   plan_fused_layout   hibf_fused_kernel<G, LAYOUT>: the same for a layout-order row (row in LDS or written directly)
//   plan_stationary     hibf_root_kernel + hibf_children_kernel<U, UNIFORM>: steps, groups, phases, tiles, grids
//   small_blocks        hibf_small_kernel
//   plan_levels         hibf_level_kernel<G> + mask_alive_kernel: G, w_iters, the chunk of a call and its frontier capacity
//   layout_level_*      hibf_layout_level_kernel: tile, tiles and grid of one level's launch, the piece of a very large batch
#pragma once
#include "txq_count_plan.hpp"
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace txq {

// What the launchers know about the index (Index, filled at upload).
struct DescentShape {
    uint32_t shard_words = 0;         // w_out: words of a mask row of this shard
    uint64_t n_ibf = 1;               // IBFs of the tree: the most entries a k-mer's stack can hold
    uint64_t total_tbs = 0;           // technical bins over all IBFs
    uint32_t max_stride = 1;          // widest row of any IBF (words)
    uint64_t max_level_width = 1;     // most IBFs on one level
    uint32_t depth = 1;               // levels
    bool has_nodes = false;           // the 32-byte node records exist (MapsPlan::compact)
    // regular two-level trees (RegularPlan); n_children == 0: none
    uint32_t n_children = 0, child_row_words = 0;
    uint64_t children_bytes = 0;
    bool children_uniform = false;
    uint32_t root_stride = 1;         // words of a root row: one k-mer's piece of the root pass' output
    bool probes_interleaved = false;  // Index::probes_interleaved: plain probes go to the interleaved children
};

// The switches of Knobs (txq_internal.hpp) that the descent reads.
struct DescentKnobs {
    bool levels = false, stationary = true, small = true, lane_hash = false, layout_fused = true, layout_direct = true;
    int steps_per_group = 0, tile = 0, unroll = 1;
    long long waves = 0, stack_lds = 128;
};

enum class DescentPath : int { Interleaved = 0, Stationary = 1, Small = 2, Fused = 3, Levels = 4 };

static constexpr uint32_t kSmallThreads = 256, kSmallStack = 32, kSmallPitch = kSmallThreads + 1;  // hibf_small_kernel
static constexpr size_t kFusedLdsBudget = 64u << 10;     // LDS of one wave of hibf_fused_kernel, at most
static constexpr size_t kFusedWaves = (size_t)256 * 64;  // its waves per launch (64 per CU), unless TXQ_HIBF_WAVES
static constexpr size_t kSmallBlocks = 256 * 8;          // most blocks of hibf_small_kernel
static constexpr size_t kRootBlocks = 256 * 32;          // most blocks of hibf_root_kernel
static constexpr size_t kLevelBlocks = 2048;             // most blocks of hibf_level_kernel and of mask_alive_kernel
static constexpr uint32_t kStationaryTile = 2048;        // k-mers per workgroup of hibf_children_kernel, unless TXQ_HIBF_TILE
static constexpr uint32_t kLayoutLevelTile = 2048;       // k-mers per workgroup of hibf_layout_level_kernel

// Entries of a wave's IBF stack kept in LDS (TXQ_HIBF_STACK_LDS, default 128; even: the stack follows the row's 8-byte words);
// the whole stack when the output row could not take the rest.
inline uint32_t fused_stack_lds(long long knob_stack_lds, uint32_t stack_cap, uint32_t w_out) {
    uint32_t in_lds = (uint32_t)std::max(2LL, knob_stack_lds) & ~1u;
    if (in_lds >= stack_cap || (uint64_t)stack_cap - in_lds > 2ull * w_out) in_lds = (stack_cap + 1) & ~1u;
    return in_lds;
}

// Waves per workgroup of hibf_fused_kernel: its waves share nothing (a wave's row and stack are its own piece of the LDS, only
// wave-level synchronisation), so the block size is free — taken so that the CU's 160 KB of LDS hold the most waves (a 22 KB
// layout-order row of the 65 536-bin trees: 7 single-wave blocks against 3 blocks of two; an 11 KB user-order row: 14 against 12).
inline unsigned fused_waves_per_block(size_t wave_bytes) {
    constexpr size_t kLdsPerCu = 160u << 10, kGranule = 1280;  // (allocation granule: the larger of the documented ones — a safe count)
    unsigned best = 1;
    size_t best_resident = 0;
    for (unsigned w = 4; w >= 1; w >>= 1) {
        if (wave_bytes * w > (64u << 10)) continue;
        const size_t block = (wave_bytes * w + kGranule - 1) / kGranule * kGranule;
        const size_t resident = std::min<size_t>(kLdsPerCu / block * w, 32);  // (a CU runs at most 8 waves per SIMD: short rows keep blocks of four)
        if (resident > best_resident) { best_resident = resident; best = w; }  // (ties: the larger block, met first)
    }
    return best;
}

struct FusedPlan {
    bool ok = false;             // false: this kernel does not take the call (the other fields up to wave_bytes are still set)
    uint32_t stack_cap = 0, stack_lds = 0, row_lds_words = 0;
    size_t wave_words = 0, wave_bytes = 0;
    unsigned waves_per_block = 0, grid = 0;
    int G = 1;                   // lanes per IBF, four row words each
    uint32_t w_iters = 1;        // sweeps of G lanes over the widest row
};

// G = the power of two >= quads of four row words of the widest IBF, at most 64; wider rows take w_iters sweeps
inline void fused_lanes(uint32_t max_stride, int* g_out, uint32_t* w_iters) {
    const uint32_t quads = (max_stride + 3) / 4;  // a lane owns four row words
    int g = 1;
    while (g < 64 && (uint32_t)g < quads) g <<= 1;
    *g_out = g;
    *w_iters = (quads + (uint32_t)g - 1) / (uint32_t)g;
}

inline void fused_grid(FusedPlan& p, long long knob_waves, size_t n) {
    p.waves_per_block = fused_waves_per_block(p.wave_bytes);
    // 64 waves per CU are launched: with an 8 KiB row the LDS keeps 14 of them resident and the rest queue up,
    // with the short rows of a column shard more are resident and the finer grain is worth 14 % (TXQ_HIBF_WAVES overrides)
    const size_t want_waves = knob_waves > 0 ? (size_t)knob_waves : kFusedWaves;
    const size_t total_waves = n < want_waves ? n : want_waves;
    p.grid = (unsigned)((total_waves + p.waves_per_block - 1) / p.waves_per_block);
}

// hibf_fused_kernel<G> in user-bin order; ok: a k-mer's row and IBF stack fit the LDS, the node records exist, no TXQ_HIBF_LEVELS=1
inline FusedPlan plan_fused(const DescentShape& sh, const DescentKnobs& kn, size_t n) {
    FusedPlan p;
    const uint32_t w_out = sh.shard_words;
    p.stack_cap = (uint32_t)sh.n_ibf;
    p.stack_lds = fused_stack_lds(kn.stack_lds, p.stack_cap, w_out);
    p.row_lds_words = w_out;
    p.wave_words = (size_t)w_out + p.stack_lds / 2;
    p.wave_bytes = p.wave_words * 8;
    p.ok = w_out && p.wave_bytes <= kFusedLdsBudget && sh.has_nodes && !kn.levels;
    if (!p.ok) return p;
    fused_grid(p, kn.waves, n);
    fused_lanes(sh.max_stride, &p.G, &p.w_iters);
    return p;
}

// hibf_fused_kernel<G, LAYOUT> on rows of v_words words; has_vnodes: the layout-order node records exist, has_split: the tree has
// split user bins.  direct (the default): no row in LDS, the whole stack is; TXQ_HIBF_LAYOUT_DIRECT=0: the row in LDS.
// Not ok: no records or TXQ_HIBF_LAYOUT_FUSED=0, a wave's LDS beyond the budget, or split bins with w_iters > 1 (they are
// unified for one pass of words per lane): the level kernels then.
inline FusedPlan plan_fused_layout(uint32_t v_words, uint64_t n_ibf, uint32_t max_stride, bool has_vnodes, bool has_split, const DescentKnobs& kn, size_t n) {
    FusedPlan p;
    if (!has_vnodes || !kn.layout_fused) return p;
    p.stack_cap = (uint32_t)n_ibf;
    p.stack_lds = kn.layout_direct ? ((p.stack_cap + 1) & ~1u) : fused_stack_lds(kn.stack_lds, p.stack_cap, v_words);
    p.row_lds_words = kn.layout_direct ? 0 : v_words;
    p.wave_words = (size_t)p.row_lds_words + p.stack_lds / 2;
    p.wave_bytes = p.wave_words * 8;
    if (p.wave_bytes > kFusedLdsBudget) return p;
    fused_grid(p, kn.waves, n);
    fused_lanes(max_stride, &p.G, &p.w_iters);
    p.ok = !(p.w_iters > 1 && has_split);
    return p;
}

struct StationaryPlan {
    bool ok = false;  // false: not a regular tree of rows of >= 2 words and a mask of > 16 words, TXQ_HIBF_STATIONARY=0, or a grid beyond 2^31
    uint32_t lanes_per_child = 0, children_per_step = 0, n_steps = 0, steps_per_group = 0, n_groups = 0, groups_per_phase = 0, phases = 0, tile = 0;
    size_t n_tiles = 0;
    unsigned grid = 0, root_blocks = 0;
    int unroll = 4;        // the U of hibf_children_kernel<U, UNIFORM> that is launched
    bool uniform = false;  // its UNIFORM
};

// A wave step covers 128 mask words: 64 lanes x 16 bytes, lanes_per_child lanes on each child.  A group = whole wave steps
// whose children fit ~2 MB (half an XCD's L2), at least 8 groups when there are 8 steps; workgroup b takes group
// (b / groups_per_phase / n_tiles) * groups_per_phase + b % groups_per_phase and tile (b / groups_per_phase) % n_tiles.
inline StationaryPlan plan_stationary(const DescentShape& sh, const DescentKnobs& kn, size_t n) {
    StationaryPlan p;
    // (narrow masks, <= 16 words, are better off with one lane per k-mer: hibf_small_kernel)
    if (!sh.n_children || sh.child_row_words < 2 || sh.shard_words <= 16 || !kn.stationary) return p;
    const uint32_t lpc = sh.child_row_words / 2, cps = 64 / lpc;
    const uint32_t n_steps = (sh.n_children + cps - 1) / cps;
    const uint64_t per_step = sh.children_bytes / n_steps + 1;
    uint32_t spg = (uint32_t)std::max<uint64_t>(1, ((uint64_t)2 << 20) / per_step);
    if (n_steps >= 8 && (n_steps + spg - 1) / spg < 8) spg = n_steps / 8;
    if (kn.steps_per_group) spg = (uint32_t)kn.steps_per_group;
    const uint32_t n_groups = (n_steps + spg - 1) / spg;
    const uint32_t gpp = n_groups < 8 ? n_groups : 8;
    const uint32_t phases = (n_groups + gpp - 1) / gpp;
    uint32_t tile = kStationaryTile;
    if (kn.tile) tile = (uint32_t)std::max(64, kn.tile);
    const size_t n_tiles = (n + tile - 1) / tile;
    p.lanes_per_child = lpc;
    p.children_per_step = cps;
    p.n_steps = n_steps;
    p.steps_per_group = spg;
    p.n_groups = n_groups;
    p.groups_per_phase = gpp;
    p.phases = phases;
    p.tile = tile;
    p.n_tiles = n_tiles;
    if (!((size_t)phases * n_tiles * gpp < ((size_t)1 << 31) && n_tiles < ((size_t)1 << 31))) return p;
    p.ok = true;
    p.grid = (unsigned)((size_t)phases * n_tiles * gpp);
    p.root_blocks = (unsigned)std::min<size_t>((n + 255) / 256, kRootBlocks);
    p.uniform = sh.children_uniform && !kn.lane_hash;  // (A/B: per-lane hashing on a uniform tree)
    const int u = kn.unroll;
    p.unroll = u == 1 || u == 2 || u == 8 || (u == 3 && p.uniform) ? u : 4;  // (the instantiated ones; U = 3 only with scalar hashing)
    return p;
}

// small trees: every IBF at most 256 technical bins, at most 32 IBFs, at most 16 mask words
inline bool small_applies(const DescentShape& sh, const DescentKnobs& kn) {
    return sh.max_stride <= 4 && sh.n_ibf <= kSmallStack && sh.total_tbs < 0xFFFF && sh.shard_words <= 16 && kn.small;
}
inline unsigned small_blocks(size_t n) {
    return (unsigned)std::min<size_t>((n + kSmallThreads - 1) / kSmallThreads, kSmallBlocks);
}
inline size_t small_lds_bytes(uint32_t w_out) {
    return (size_t)w_out * kSmallPitch * 8 + (size_t)kSmallStack * kSmallThreads * 2;
}

struct LevelsPlan {
    int G = 1;             // lanes per work item, one row word each
    uint32_t w_iters = 1;  // sweeps over rows wider than 64 words
    size_t chunk = 1;      // k-mers per pass over the levels (count_hibf_chunk: a level's frontier fits kHibfCapItems)
    size_t cap = 1;        // work items a frontier buffer holds
    unsigned blocks_deeper = 1, alive_blocks = 1;
};

// blocks of hibf_level_kernel<g> on level lvl of a chunk of m k-mers: level 0 is sized by the chunk, deeper levels are
// grid-stride over a count only the device knows
inline unsigned level_blocks(int g, uint32_t lvl, size_t m) {
    const size_t groups = lvl ? kLevelBlocks * 256 / (size_t)g : m;
    size_t blocks = (groups * (size_t)g + 255) / 256;
    if (blocks > kLevelBlocks) blocks = kLevelBlocks;
    return (unsigned)(blocks ? blocks : 1);
}

inline LevelsPlan plan_levels(const DescentShape& sh, size_t n) {
    LevelsPlan p;
    // Frontier bound: a (k-mer, IBF) pair occurs at most once, so level l holds at most chunk * (#IBFs on level l) items.
    p.chunk = count_hibf_chunk(n, sh.max_level_width);
    p.cap = p.chunk * sh.max_level_width;
    int g = 1;
    while (g < 64 && (uint32_t)g < sh.max_stride) g <<= 1;
    p.G = g;
    p.w_iters = (sh.max_stride + (uint32_t)g - 1) / (uint32_t)g;
    p.blocks_deeper = level_blocks(g, 1, 0);
    p.alive_blocks = (unsigned)std::min<size_t>(((n + 63) / 64 * 64 + 255) / 256, kLevelBlocks);
    return p;
}

// the kernel(s) hibf_probe runs for a batch of n > 0 plain k-mers
inline DescentPath descent_path(const DescentShape& sh, const DescentKnobs& kn, size_t n) {
    if (sh.probes_interleaved) return DescentPath::Interleaved;
    if (!plan_fused(sh, kn, n).ok) return DescentPath::Levels;  // (also where the other kernels below would apply: they share the gate)
    if (plan_stationary(sh, kn, n).ok) return DescentPath::Stationary;
    if (small_applies(sh, kn)) return DescentPath::Small;
    return DescentPath::Fused;
}

// hibf_layout_level_kernel, one launch per level: workgroup = (group g of 8 of a phase, tile of kLayoutLevelTile k-mers)
inline uint32_t layout_level_tiles(size_t n) { return (uint32_t)((n + kLayoutLevelTile - 1) / kLayoutLevelTile); }
inline uint32_t layout_level_phases(uint32_t n_groups) { return (n_groups + 7) / 8; }
// blocks of a level's launch; 0: too many k-mers for one layout-order probe
inline uint32_t layout_level_grid(uint32_t n_groups, uint32_t n_tiles) {
    const uint64_t g = (uint64_t)layout_level_phases(n_groups) * n_tiles * 8;
    return g >= ((uint64_t)1 << 31) ? 0u : (uint32_t)g;
}
// k-mers that go through the levels together: their gates (the words of IBFs with merged bins, about 96 MB) stay in the
// Infinity Cache between two levels, and never fewer than 4 M
inline size_t layout_level_piece(uint32_t v_inner_words) {
    return std::max<size_t>((size_t)4 << 20, (((size_t)96 << 20) / ((size_t)std::max(v_inner_words, 1u) * 8)) / kLayoutLevelTile * kLayoutLevelTile);
}

}  // namespace txq
