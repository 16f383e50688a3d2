// The sliding window count on an HIBF (txq_count_windows, txq_count.hip count_windows_tree_kernel), where a
// CPU can run it.  Plain functions, no HIP: the kernel and the launcher call them and do not restate them, and
// tests/native/count_windows_tree_sim.cpp walks a synthetic tree level by level with the same functions under sanitizers.
//
// A unit is U consecutive windows (txq_count_windows_plan.hpp), U <= 32 on a tree.  The work item of a level is
// (unit, IBF, mask): bit w of the mask says that window cw_unit_first(unit, U) + w visits the IBF.  ONE wave owns an item: it
// walks the set bits in window order and keeps the current window's counters on that IBF, sliding from the previous VISITED
// window to the next one — a subsequence of a sliding sequence still slides, so cw_step holds between two visited windows
// that are not neighbours.  For every merged bin a window passes, the wave ORs the window's bit into the bin's mask word;
// after the item's last window every non-zero mask word is the child's item (unit, child, mask) of the next level.
#pragma once
#include "txq_count_windows_plan.hpp"
#include <stddef.h>

namespace txq {

constexpr uint32_t kCountWindowsTreeDefault = 1;    // TXQ_COUNT_WINDOWS_TREE: 1 slides on a tree, 0 counts every (window, IBF) pair in full
constexpr uint32_t kCountWindowsTreeUnitMax = 32;  // windows of a unit on a tree: one bit each in a u32 mask

struct CwTreeItem {
    uint32_t unit, ibf, mask;
};

// Totals of a call (txq_count_windows_trace): a wave sums its items' totals and adds them once, at its end, to the set of
// totals of its slot; the sets are summed on the host
enum : uint32_t { kCwTraceVisits = 0, kCwTraceAdded = 1, kCwTraceSubtracted = 2, kCwTraceItems = 3, kCwTraceWords = 4 };
constexpr uint32_t kCwTraceSlots = 64;

// the windows of a unit on a tree, from TXQ_COUNT_WINDOWS_UNIT as the flat kernel reads it
TXQ_CW_FN uint32_t cwt_unit(uint32_t asked) {
    return asked < 1 ? 1 : asked > kCountWindowsTreeUnitMax ? kCountWindowsTreeUnitMax : asked;
}

// the level-0 mask of unit u: all of its windows visit the root
TXQ_CW_FN uint32_t cwt_level0_mask(uint64_t u, uint32_t U, uint64_t n_windows) {
    const uint64_t n = cw_unit_last(u, U, n_windows) - cw_unit_first(u, U);
    return n >= 32 ? 0xFFFFFFFFu : (1u << n) - 1u;
}

// The walk over the set bits of an item's mask, in window order.
struct CwTreeWalk {
    uint32_t left;    // bits still to visit
    bool first;       // the next window opens the item: the counters hold whatever the wave's last item left
    uint64_t pb, pe;  // the previous VISITED window
};

TXQ_CW_FN CwTreeWalk cwt_walk(uint32_t mask) { return CwTreeWalk{mask, true, 0, 0}; }
TXQ_CW_FN bool cwt_more(const CwTreeWalk& w) { return w.left != 0; }
// the position in its unit of the window the walk stands on (cwt_more)
TXQ_CW_FN uint32_t cwt_window(const CwTreeWalk& w) { return (uint32_t)__builtin_ctz(w.left); }
// what turns the counters into those of that window [b, e), and on to the next set bit
TXQ_CW_FN CwStep cwt_advance(CwTreeWalk& w, uint64_t b, uint64_t e) {
    const CwStep s = cw_step(w.first, w.pb, w.pe, b, e);
    w.first = false;
    w.pb = b, w.pe = e;
    w.left &= w.left - 1u;
    return s;
}

// Units per device call: a (unit, IBF) pair occurs at most once per level, so level l holds at most
// units * (IBFs on level l) items, and units * max_level_width is what a frontier buffer must hold: within cap_items,
// except that a call holds at least one unit.  Device calls are cut at unit boundaries.
TXQ_CW_FN size_t cwt_units_per_call(size_t n_units, size_t max_level_width, size_t cap_items) {
    const size_t fit = cap_items / (max_level_width ? max_level_width : 1);
    const size_t c = fit > 1 ? fit : 1;
    return c < n_units ? c : n_units;
}
TXQ_CW_FN size_t cwt_frontier_items(size_t units_per_call, size_t max_level_width) { return units_per_call * (max_level_width ? max_level_width : 1); }

}  // namespace txq
