// How a (window, view) pair of txq_edit_window_targets.hip finds its pattern and its text, where a CPU can run it
// (DESIGN.md §22).  Plain functions, no HIP: the kernels call them and do not restate them, and
// tests/native/edit_window_targets_sim.cpp runs the kernel's lane schedule on the CPU under sanitizers with the same functions.
//
// The kernel is targets_kernel<W> of txq_edit_targets.hip behind another view of a pair.  There a pair is (pattern of an offset
// table, group of ONE text); here it is (window into one letter buffer, view of a table): the pattern is letters[p0 .. p0 + m),
// the text is the view's, and the view is one group of all its records — records [0, n_rec), bytes [rec[0], rec[n_rec]) of a
// text that lies at [text, text + text_bytes).  Slots, first keys, the flush rule, the compaction and the rows are those of
// txq_edit_targets_plan.hpp with r0 = 0, r1 = n_rec, gs = rec[0], ge = rec[n_rec].
#pragma once
#include "txq_edit_targets_plan.hpp"

namespace txq {
namespace wt {

constexpr uint32_t kMaxWindow = 512;  // letters of a window at most (TXQ_EDIT_MAX_PATTERN)

// one entry of the view table: txq_text_view of include/txq.h
struct View {
    const uint8_t* text;
    const uint64_t* rec;  // n_rec + 1 offsets into text
    uint64_t n_rec, text_bytes;
};

// What a pair works on.  ok = false: its window index or view index is out of range, its window has no letters, more than
// kMaxWindow or leaves the letter buffer, or the view's ends leave text_bytes or do not ascend.  Nothing behind a failed check
// is read: win_begin / win_len only for p < n_windows, the table only for g < n_views, of the view's offsets only the first
// and the last.  The table entry itself (pointers and sizes) is the caller's word.
struct Pair {
    bool ok;
    uint32_t m, e;
    uint64_t p0;  // the window: letters[p0 .. p0 + m)
    View v;       // the text
    uint64_t r1;  // records [0, r1)
    uint64_t gs, ge;
};

TXQ_TEXT_FN Pair view_pair(const uint32_t* pairs, uint64_t i, const uint64_t* win_begin, const uint32_t* win_len, uint64_t n_windows, uint64_t letters_bytes,
                           const View* views, uint64_t n_views) {
    Pair a{};
    const uint32_t p = pairs[3 * i], g = pairs[3 * i + 1];
    a.e = pairs[3 * i + 2];
    if (p >= n_windows || g >= n_views) return a;
    const uint64_t p0 = win_begin[p];
    const uint32_t m = win_len[p];
    if (m == 0 || m > kMaxWindow || p0 > letters_bytes || m > letters_bytes - p0) return a;
    a.v = views[g];
    a.m = m, a.p0 = p0, a.r1 = a.v.n_rec;
    a.gs = a.v.rec[0], a.ge = a.v.rec[a.v.n_rec];
    a.ok = a.gs <= a.ge && a.ge <= a.v.text_bytes;
    return a;
}

// 64-bit words of a window's Peq rows: the instance that walks it
TXQ_TEXT_FN uint32_t words_of(uint32_t m) { return m <= 64 ? 1u : m <= 128 ? 2u : m <= 256 ? 4u : 8u; }

// units of 64 lane chunks that a pair's text is cut into (a refused pair: none)
TXQ_TEXT_FN uint64_t units_of_pair(const Pair& a, uint32_t chunk) { return a.ok ? units_of(a.ge - a.gs, 64, chunk) : 0; }

// the bytes in front of a lane's chunk that its walk needs: a match that ends in the chunk begins at most m + min(e, m) before
TXQ_TEXT_FN uint64_t lead_of(uint32_t m, uint32_t e) { return (uint64_t)m + (e < m ? e : m); }

// Where the walk of a lane begins whose chunk begins at ca in a record that begins at rs: `lead` bytes in front of ca, or at the
// record's first byte.  (Offsets that do not ascend cannot take a load outside [gs, ge): an rs outside [gs, ca] counts as ca.)
TXQ_TEXT_FN uint64_t walk_start(uint64_t ca, uint64_t rs, uint64_t gs, uint64_t lead) {
    if (rs < gs || rs > ca) rs = ca;
    return ca - rs > lead ? ca - lead : rs;
}

}  // namespace wt
}  // namespace txq
