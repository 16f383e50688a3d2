// The step logic of the long-pattern edit-distance kernel (txq_edit_long.hip; DESIGN.md §12 "Long patterns"), where a CPU
// can run it: the block step of Myers' algorithm in Hyyrö's block-based form, the value that moves from lane to lane, the
// choice of the lane group, the unit and span arithmetic, the lead-in start and the walk over record ends.  Plain functions,
// no HIP: the kernel calls them and does not restate them, and tests/native/edit_long_sim.cpp runs the same schedule on the
// CPU under sanitizers, with the lanes as an array and the cross-lane move as a shift by one.
//
// The pattern's W = ceil(m / 64) words lie over the lanes of a group, word w in lane w.  Lane w keeps the vertical deltas
// Pv / Mv of rows 64 w .. 64 w + 63.  At step s it works on text column s - w: what it needs from above is the horizontal
// delta at row 64 w - 1 of that column (hin in {-1, 0, +1}; 0 for lane 0, since D[0][j] = 0), which lane w - 1 produced one
// step earlier, and the column's class.  Both travel in one 32-bit message, with a flag "a record begins at this column":
// the lane it reaches starts that column from the fresh state (Pv all ones, Mv zero: D[i][0] = i), so the reset moves down
// the pattern with its column and every lane sees, column after column, what the one-integer recurrence does to its word.
#pragma once
#include "txq_edit_common.hpp"

namespace txq {

constexpr uint32_t kEditLongMaxPattern = 4096;  // 64 lanes of one word (TXQ_EDIT_LONG_MAX_PATTERN)

// ---- the message from lane w - 1 to lane w --------------------------------------------------------------------------
constexpr uint32_t kMsgClass = 31;         // bits 0..4: the column's class (31: matches nothing)
constexpr uint32_t kMsgReset = 1u << 5;    // a record begins at this column
constexpr uint32_t kMsgValid = 1u << 6;    // there is a column (clear while the pipeline fills and drains)
constexpr uint32_t kMsgPlus = 1u << 8;     // hin = +1
constexpr uint32_t kMsgMinus = 1u << 9;    // hin = -1 (never both)

// what lane 0 makes of a text byte: hin = 0
TXQ_TEXT_FN uint32_t long_feed(uint32_t cls, bool reset) { return (cls & kMsgClass) | (reset ? kMsgReset : 0u) | kMsgValid; }
TXQ_TEXT_FN int long_hin(uint32_t msg) { return (int)((msg >> 8) & 1u) - (int)((msg >> 9) & 1u); }

// ---- the block step -------------------------------------------------------------------------------------------------
// One column in one word: `msg` as it arrived (a reset is applied first), eq the word's match vector for the column's
// class.  Updates pv / mv and returns the message for the lane below: the same column, hout the horizontal delta at bit
// `bit` of the word — 63 in a lane that has a lane below, (m - 1) & 63 in the lane that holds the pattern's last row, where
// hout is the change of the score.  A message without kMsgValid changes nothing and is passed on as it is.
TXQ_TEXT_FN uint32_t long_block_step(uint64_t& pv, uint64_t& mv, uint64_t eq, uint32_t msg, uint32_t bit) {
    const bool valid = (msg & kMsgValid) != 0, reset = (msg & kMsgReset) != 0;
    const uint64_t p = reset ? ~0ULL : pv, n = reset ? 0ULL : mv;
    const uint64_t hp_in = (msg >> 8) & 1u, hm_in = (msg >> 9) & 1u;
    const uint64_t xv = eq | n;
    const uint64_t eqc = eq | hm_in;  // hin = -1: the diagonal above the word's first row allows a zero step
    const uint64_t xh = (((eqc & p) + p) ^ p) | eqc;
    uint64_t ph = n | ~(xh | p), mh = p & xh;
    const uint32_t hp = (uint32_t)(ph >> bit) & 1u, hm = (uint32_t)(mh >> bit) & 1u;
    ph = (ph << 1) | hp_in;
    mh = (mh << 1) | hm_in;
    pv = valid ? mh | ~(xv | ph) : pv;
    mv = valid ? ph & xv : mv;
    return valid ? (msg & 0xFFu) | hp << 8 | hm << 9 : msg;
}

// ---- groups, units, spans -------------------------------------------------------------------------------------------
// lanes of the group a pattern of m bytes runs on: the smallest of 16, 32, 64 that holds its words (m <= 4096)
TXQ_TEXT_FN uint32_t long_group_lanes(uint32_t m) {
    const uint32_t words = (m + 63) >> 6;
    return words <= 16 ? 16u : words <= 32 ? 32u : 64u;
}
// A wave carries 64 / G groups, each on its own span of `span` text bytes: a unit is one wave's spans.
TXQ_TEXT_FN uint32_t long_groups(uint32_t G) { return 64u / G; }
TXQ_TEXT_FN uint64_t long_units(uint64_t bytes, uint32_t G, uint32_t span) { return units_of(bytes, long_groups(G), span); }
TXQ_TEXT_FN ChunkBounds long_span(uint64_t gs, uint64_t ge, uint64_t slice, uint32_t G, uint32_t group, uint32_t span) {
    return chunk_bounds(gs, ge, slice, long_groups(G), group, span);
}

// The byte at which a span [ca, ..) starts from the fresh state: its record's start rs, or ca - (m + min(e, m)) where that
// is later.  Exact for every D[m][j] <= e at j >= ca: an alignment of cost <= e that ends at j begins no earlier than
// j - m - e + 1, D[m][j] <= m needs no earlier start than j - 2 m + 1, and a later start only raises a value.  (rs outside
// [gs, ca] — offsets that do not ascend — counts as ca: every byte index then stays in [start, cb).)
TXQ_TEXT_FN uint64_t long_start(uint64_t ca, uint64_t rs, uint64_t gs, uint32_t m, uint32_t e) {
    const uint64_t lead = (uint64_t)m + (e < m ? e : m);
    if (rs < gs || rs > ca) rs = ca;
    return ca - rs > lead ? ca - lead : rs;
}

// Byte t is at or behind the end of record r: the next record of [.., r1) that holds t (r is advanced over records of no
// bytes), and its end, which the function returns — never beyond the group's end ge, whatever the offsets say.
TXQ_TEXT_FN uint64_t long_next_record(const uint64_t* rec, uint64_t& r, uint64_t r1, uint64_t ge, uint64_t t) {
    uint64_t re;
    do {
        ++r;
        re = r + 1 <= r1 ? rec[r + 1] : ge;
    } while (t >= re && r + 1 < r1);
    if (re > ge || t >= re) re = ge;
    return re;
}

// Steps of a group that walks `columns` text bytes: its last column reaches the lane of the pattern's last row, lane
// (m - 1) >> 6, that many steps after lane 0 took it.
TXQ_TEXT_FN uint64_t long_steps(uint64_t columns, uint32_t m) { return columns ? columns + ((m - 1) >> 6) : 0; }

}  // namespace txq
