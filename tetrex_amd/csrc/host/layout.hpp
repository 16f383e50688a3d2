// Host side: the size-aware HIBF layout of `tetrex index --layout sized` — a pure function of k-mer count estimates
// (no GPU, no files), after the hierarchical-binning DP of the HIBF paper (Mehringer et al. 2023).
//
// Input: one HyperLogLog estimate per user bin, and a table of union estimates over runs of the bins in LAYOUT ORDER
// (estimate descending, ties by user bin id): unions[s * window + L - 1] = estimate of the union of the bins at sorted
// positions s .. s+L-1, for L <= window.  Every merge the DP can make, in the root or in any child, is such a run, so one
// table serves the whole tree.  Output: the shapes and maps of every IBF of the tree (what HibfImage holds, without words).
//
// DP of one IBF over n sorted bins with T = min(t_max, 64 * ceil(n / 64)) technical bins, all of them used.
// Cell (i, j) = the best placement of the first j+1 bins in the first i+1 technical bins, scored
// (i+1) * maxTB + alpha * lowerLevelBits; it keeps that pair (maxTB, lower) and how it was reached.
//   split: bin j over s = i - i' technical bins, each weighing ceil(c_j / s) * corr[s]
//   merge: bins j'+1 .. j (2 <= j - j' <= window) into one technical bin weighing their union estimate; the lower-level
//          cost grows by (sum of their estimates) * ceil(log_T(j - j'))
// corr[s] = ln(1 - fpr^(1/h)) / ln(1 - p_s^(1/h)), p_s = 1 - (1 - fpr)^(1/s): the s parts of a split bin together keep fpr.
// Ties: a candidate replaces the cell's best only with a strictly smaller score; splits are tried before merges, each by
// ascending length — so the first of equal candidates in that order wins, and the result is a function of the input alone.
// Each merged run becomes a child IBF laid out by the same DP over its own sub-range, until no merge remains.
//
// IBF numbering: depth-first pre-order — the root is 0, and an IBF's children follow it in the order of its technical
// bins, each with its whole sub-tree before the next child.  Technical bins keep the DP's order (estimate descending);
// leaves have next_ibf_id 0 (as the uniform builder writes them), merged bins tb_to_user_bin = UINT64_MAX.
// Sizing: an IBF's bin_size is the largest over its technical bins of compute_bitcount(ceil(ceil(c / s) * corr[s]), fpr)
// for the parts of a split (or whole) bin and compute_bitcount(ceil(union), relaxed_fpr) for merged bins (at least 1).
#pragma once
#include <cstdint>
#include <vector>

namespace tetrex {

// IBFIndex::compute_bitcount (reference include/index_ibf.h:133-139)
uint64_t compute_bitcount(uint64_t n, float fpr);

struct LayoutParams {
    uint64_t tmax = 0;  // 0: default_tmax(B)
    float fpr = 0.05f;
    float relaxed_fpr = 0.3f;  // of merged bins, as seqan::hibf's default
    unsigned hash_count = 3;
    double alpha = 1.2;  // weight of the lower levels' bits
};

struct LayoutIbf {
    uint64_t bin_size = 0;
    std::vector<uint64_t> next_ibf_id;     // [technical bin]: child of a merged bin, 0 for a leaf
    std::vector<uint64_t> tb_to_user_bin;  // [technical bin]: user bin, UINT64_MAX for a merged bin
};

struct HibfLayout {
    uint64_t tmax = 0, window = 0;
    std::vector<uint64_t> order;  // layout order: user bin at sorted position s
    std::vector<LayoutIbf> ibfs;  // [0] = root
};

// One step of a user bin's path from the root: technical bins [tb, tb + parts) of IBF `ibf` (parts > 1 only at the leaf).
struct PathStep {
    uint64_t ibf, tb, parts;
};

// 64 * ceil(ceil(sqrt(B)) / 64): the uniform builder's rule
uint64_t default_tmax(uint64_t user_bins);
// W = min(B, 4 * ceil(B / t_max)): the longest run one merged bin may take
uint64_t union_window(uint64_t user_bins, uint64_t tmax);
// user bins by estimate descending, ties by id
std::vector<uint64_t> layout_order(const double* counts, uint64_t user_bins);
// corr[s] for s = 0 .. max_parts (corr[0] unused)
std::vector<double> split_corrections(uint64_t max_parts, double fpr, unsigned hash_count);
// counts: by user bin id; unions: user_bins x window (see above).  Throws std::invalid_argument on a bad input.
HibfLayout hibf_layout(const double* counts, uint64_t user_bins, const double* unions, uint64_t window, const LayoutParams& params);
// The same over a GIVEN order (a permutation of 0 .. B-1, anything else is refused): unions[s * window + L - 1] is then the
// union of the bins order[s .. s+L-1].  The DP reads counts[order[pos]] and that table, nothing else, so it never needs the
// order to be sorted; with layout_order(counts) this is hibf_layout.  HibfLayout::order holds the order used.
HibfLayout hibf_layout_ordered(const double* counts, uint64_t user_bins, const uint64_t* order, const double* unions, uint64_t window,
                               const LayoutParams& params);

// Similarity rearrangement (`tetrex index --layout sized --rearrange`): before the layout, user bins that share k-mers are
// moved next to each other, so that a merged bin (a run of the order, sized by its union) covers bins that overlap.
// Two pure steps; the pairwise union estimates between them come from the device (include/txq.h txq_pair_unions_device).
//   intervals: walk the sorted order from position 0; an interval starts at position s and takes the following positions e
//     while counts[order[e]] >= ratio * counts[order[s]] and while it is shorter than max_len; then the next one starts.
//     Bins only move inside their interval, so the order stays "large bins first" up to the factor ratio (in (0, 1]).
//   chain: inside an interval of n bins with pairwise union estimates u[i * n + j] (i, j: positions in the interval), position
//     0 stays; then, n - 1 times, the bin not yet placed with the largest J = (c_last + c_j - u[last][j]) / u[last][j] to the
//     bin placed last follows it (u == 0: J = 0; ties: the smaller position).  Intervals of one or two bins are left alone.
// This is a greedy nearest-neighbour chain, O(n^2), not seqan::hibf's agglomerative clustering.
constexpr uint64_t kRearrangeMaxLen = 4096;  // one interval's pairwise table: at most 4096^2 doubles (128 MiB)
// first sorted position of every interval, ascending (interval i ends where i + 1 starts, the last one at B)
std::vector<uint64_t> rearrange_intervals(const double* counts, const uint64_t* order, uint64_t user_bins, double ratio,
                                          uint64_t max_len = kRearrangeMaxLen);
// counts[n]: the interval's estimates by position; returns the chain as positions of the interval
std::vector<uint64_t> rearrange_chain(const double* counts, const double* unions, uint64_t n);
// each user bin's path, root first
std::vector<std::vector<PathStep>> layout_paths(const HibfLayout& layout, uint64_t user_bins);

}  // namespace tetrex
