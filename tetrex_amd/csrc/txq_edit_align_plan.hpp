// The step logic of the alignment kernel (txq_edit_align.hip), where a CPU can run it: what a result triple
// asks for, the band's geometry, the update of one row with the lanes as an array, the two direction bits of a cell and the
// walk back over them.  Plain functions, no HIP: the kernel calls them and does not restate them, and
// tests/native/edit_align_sim.cpp runs the same steps on the CPU under sanitizers, a cross-lane move being an index into an array.
//
// A pair's search result (d, r, j) says that D[m][j] = d in record r.  Every cell on the walk back from (m, j), and every cell
// whose value the walk compares, lies on one of the 2 d + 1 diagonals around the one through (m, j), and its value restricted
// to those diagonals is its value in the full matrix; the values of other cells only grow (DESIGN.md §15 has the argument).
// Lane k owns diagonal k - d: at row i it holds column j' = j - m + i + k - d.  Its upper neighbour (i - 1, j') is lane k + 1
// of the row before, its diagonal neighbour (i - 1, j' - 1) is itself in the row before, its left neighbour (i, j' - 1) is lane
// k - 1 of the same row.  So a row is: one value from the lane above, a minimum of two sums per lane, and
//     v[k] = min over l <= k of t[l] + (k - l)
// for the dependency inside the row — a prefix minimum of t[l] - l, about log2(2 d + 1) cross-lane steps.  Column 0 is the D[i][0] = i
// boundary (the window R[max(0, j - m - d) .. j) clipped at the record's start), columns below 0 and above j are not cells.
#pragma once
#include "txq_text.hpp"

namespace txq {

constexpr uint32_t kAlignMaxDistance = 31;   // 2 d + 1 diagonals in one wave (TXQ_EDIT_ALIGN_MAX_DISTANCE)
constexpr uint32_t kAlignMaxPattern = 4096;  // rows of direction bits in LDS (TXQ_EDIT_LONG_MAX_PATTERN)
constexpr uint32_t kAlignInf = 1u << 28;     // no cell: sums of a few of these and of lane numbers stay below 2^32
constexpr uint32_t kAlignNone = 0xFFFFFFFFu, kAlignDeclined = 0xFFFFFFFEu;
constexpr uint32_t kOpMatch = 0, kOpMismatch = 1, kOpInsert = 2, kOpDelete = 3;  // = X I D

// ---- what a triple asks for --------------------------------------------------------------------------------------------
enum class AlignKind { None, Refused, Declined, Run };
// (d, r, j) as the search call left them — device data, possibly garbage — for a pattern of m bytes and the group's records
// [r0, r1) in bytes [gs, ge) of the text.  Run: r is a record of the group that lies inside it, j <= its length, d <= m and
// d within both limits, so every index derived from (m, d, j) stays inside the record.
TXQ_TEXT_FN AlignKind align_kind(uint32_t d, uint32_t r, uint32_t j, uint64_t m, uint32_t max_errors, const uint64_t* rec, uint64_t r0, uint64_t r1,
                                 uint64_t gs, uint64_t ge) {
    if (d == kAlignNone) return r == kAlignDeclined ? AlignKind::Refused : AlignKind::None;
    if (d > kAlignMaxDistance || d > max_errors || m > kAlignMaxPattern || d > m) return AlignKind::Declined;
    if (r < r0 || r >= r1) return AlignKind::Declined;
    const uint64_t rs = rec[r], re = rec[r + 1];
    if (rs < gs || re > ge || rs > re || j > re - rs) return AlignKind::Declined;
    return AlignKind::Run;
}

// ---- the same for a window against a view (txq_edit_align_windows_device) -------------------------------------
// The pattern is a window into one letter buffer, the text one entry of a table of views: the records of one bin, all of them
// the pair's ONE group.  The layout is txq_text_view's of include/txq.h.
struct AlignTextView {
    const uint8_t* text;
    const uint64_t* rec;  // n_rec + 1 offsets into text
    uint64_t n_rec, text_bytes;
};
constexpr uint32_t kAlignMaxWindow = 512;  // rows of the one instance that aligns windows (TXQ_EDIT_MAX_PATTERN)
// Is pair (window p, view g) one the call answers?  No: its window index or view index is out of range, the window has no
// letters or leaves the letter buffer (win_begin / win_len are read only for p < n_windows).
TXQ_TEXT_FN bool align_window_ok(uint32_t p, uint32_t g, uint64_t n_windows, uint64_t n_views, const uint64_t* win_begin, const uint32_t* win_len,
                                 uint64_t letters_bytes) {
    if (p >= n_windows || g >= n_views) return false;
    const uint64_t p0 = win_begin[p], m = win_len[p];
    return m != 0 && p0 <= letters_bytes && m <= letters_bytes - p0;
}
// (d, r, j) for a window of m >= 1 letters against view v, whose table entry is the caller's word and whose offsets are device
// data: r indexes the view's offsets.  Run: m <= kAlignMaxWindow and what align_kind asks with the view as the group — records
// [0, n_rec) in bytes [0, text_bytes) —, so rec[r] and rec[r + 1] are among the view's n_rec + 1 offsets and every byte read lies
// in [text, text + text_bytes).
TXQ_TEXT_FN AlignKind align_window_kind(uint32_t d, uint32_t r, uint32_t j, uint64_t m, uint32_t max_errors, const AlignTextView& v) {
    if (d != kAlignNone && m > kAlignMaxWindow) return AlignKind::Declined;
    return align_kind(d, r, j, m, max_errors, v.rec, 0, v.n_rec, 0, v.text_bytes);
}

// ---- the band ------------------------------------------------------------------------------------------------------------
struct AlignBand {
    uint32_t m, d, j;
};
// the column of lane k at row i (negative, or above j: no cell)
TXQ_TEXT_FN int64_t align_column(const AlignBand& b, uint32_t i, uint32_t k) { return (int64_t)b.j - b.m + i + k - b.d; }
TXQ_TEXT_FN bool align_in_band(const AlignBand& b, uint32_t k, int64_t col) { return k <= 2 * b.d && col >= 0 && col <= (int64_t)b.j; }
TXQ_TEXT_FN uint32_t align_row0(const AlignBand& b, uint32_t k) { return align_in_band(b, k, align_column(b, 0, k)) ? 0u : kAlignInf; }
// Rows come in blocks of 64, rows i0 + 1 .. i0 + 64: lane l fetches the pattern byte of row i0 + 1 + l and the record bytes
// at align_text_index(b, i0, l) and 64 behind it (a byte outside [0, j) of the record is not loaded: no class).  Lane k at row
// i0 + 1 + ii then compares with byte number ii + k of those 128.
TXQ_TEXT_FN int64_t align_text_index(const AlignBand& b, uint32_t i0, uint32_t l) { return (int64_t)b.j - b.m - b.d + i0 + l; }

// ---- one row -------------------------------------------------------------------------------------------------------------
// the cell's value before the dependency inside the row: up / diag are D[i - 1][col] / D[i - 1][col - 1] in the band
TXQ_TEXT_FN uint32_t align_cell(bool in_band, int64_t col, uint32_t i, uint32_t up, uint32_t diag, bool match) {
    if (!in_band) return kAlignInf;
    if (col == 0) return i;
    const uint32_t a = up + 1, b = diag + (match ? 0u : 1u);
    return a < b ? a : b;
}
// The prefix minimum runs on x[k] = t[k] + 64 - k, so that it is a plain minimum over lanes 0 .. k; afterwards v[k] = x[k] - 64
// + k.  One step joins x with the x of a lane below (kAlignInf where there is none).  Which lanes, in which order, is the
// caller's: the simulator doubles the distance, s = 1, 2, 4, .. <= 2 d; the kernel does the same inside rows of 16 lanes and then
// joins the rows, which is what DPP moves offer.  Any order that has joined lanes 0 .. k into lane k gives the same values.
TXQ_TEXT_FN uint32_t align_scan_bias(uint32_t t, uint32_t k) { return t + 64 - k; }
TXQ_TEXT_FN uint32_t align_scan_step(uint32_t x, uint32_t below) { return below < x ? below : x; }
TXQ_TEXT_FN uint32_t align_scan_value(bool in_band, uint32_t x, uint32_t k) { return in_band ? x - 64 + k : kAlignInf; }
// the operation that leads into a cell of value v: the first rule of include/txq.h that holds
TXQ_TEXT_FN uint32_t align_op(int64_t col, uint32_t v, uint32_t up, uint32_t diag, bool match) {
    if (col <= 0) return kOpInsert;  // D[i][0] = i comes from D[i - 1][0]
    if (diag + (match ? 0u : 1u) == v) return match ? kOpMatch : kOpMismatch;
    return up + 1 == v ? kOpInsert : kOpDelete;
}

// ---- the walk back -------------------------------------------------------------------------------------------------------
// Row i's operations are two 64-bit words, bit k of `lo` / `hi` the low / high bit of lane k's operation.  The walk starts at
// (m, lane d) and ends at row 0; runs close in walk order, the last letters first.
struct AlignWalk {
    uint32_t i, k, run_op, run_len, n_runs;
};
TXQ_TEXT_FN AlignWalk align_walk_begin(const AlignBand& b) { return {b.m, b.d, 0, 0, 0}; }
// the lane left the band (k wraps below 0): the bits were not those of a band that holds the path
TXQ_TEXT_FN bool align_walk_lost(const AlignWalk& w, const AlignBand& b) { return w.k > 2 * b.d; }
// One cell: returns the run that closed, as (length << 2) | op — never 0 —, or 0; it is run number w.n_runs - 1.
TXQ_TEXT_FN uint32_t align_walk_step(AlignWalk& w, uint64_t lo, uint64_t hi) {
    const uint32_t op = (uint32_t)((lo >> w.k) & 1) | (uint32_t)((hi >> w.k) & 1) << 1;
    uint32_t closed = 0;
    if (w.run_len && op != w.run_op) {
        closed = w.run_len << 2 | w.run_op;
        w.run_len = 0;
        ++w.n_runs;
    }
    w.run_op = op;
    ++w.run_len;
    if (op == kOpDelete) --w.k;
    else {
        --w.i;
        if (op == kOpInsert) ++w.k;
    }
    return closed;
}
// at row 0: the last run (m >= 1, so there is one)
TXQ_TEXT_FN uint32_t align_walk_end(AlignWalk& w) {
    ++w.n_runs;
    return w.run_len << 2 | w.run_op;
}
// run number `run` of n_runs in walk order is word 2 + this of the pair's answer
TXQ_TEXT_FN uint32_t align_run_slot(uint32_t n_runs, uint32_t run) { return n_runs - 1 - run; }

}  // namespace txq
