"""Python restatement of the sliding window count on an HIBF (include/txq.h txq_count_windows, csrc/txq_count_windows_tree_plan.hpp;
DESIGN.md §17): TreeRef's descent (tests/search_ref.py) with every window written out as a query of its own, keeping for each
level the windows that visit each IBF; from those visit sets the work items (unit, IBF) of every level, and cw_step between two
consecutive VISITED windows of an item — what the kernel adds and subtracts, and what txq_count_windows_trace reports."""
import numpy as np

from search_ref import count_on, pack

TREE_UNIT_MAX = 32  # txq_count_windows_tree_plan.hpp kCountWindowsTreeUnitMax


def descend(ref, values, offsets, thresholds):
    """TreeRef.search, which also returns the levels: a list of {IBF: ascending array of the queries that visit it}."""
    nq = len(offsets) - 1
    W = (ref.user_bins + 63) // 64
    counts = np.zeros((nq, 64 * W), dtype=np.int64)
    hits = np.zeros((nq, 64 * W), dtype=bool)
    t = np.asarray(thresholds, dtype=np.int64)
    level, levels = {0: np.arange(nq)}, []
    while level:
        levels.append(level)
        nxt = {}
        for i, qs in level.items():
            c = count_on(ref.ox[i], values, offsets, qs)[:, :ref.descs[i]["bins"]]
            starts, merged, ub, child = ref.segs[i]
            sums = np.add.reduceat(c, starts, axis=1)
            for s in range(starts.size):
                passed = sums[:, s] >= t[qs]
                if merged[s]:
                    if passed.any():
                        nxt.setdefault(int(child[s]), []).append(qs[passed])
                else:
                    counts[qs, int(ub[s])] = np.maximum(counts[qs, int(ub[s])], sums[:, s])
                    hits[qs, int(ub[s])] |= passed
        level = {i: np.sort(np.concatenate(v)) for i, v in nxt.items()}
    return pack(hits), counts, levels


def cw_step(first, pb, pe, b, e):
    """txq_count_windows_plan.hpp cw_step: (reset, values added, values subtracted)"""
    if first or b >= pe or b < pb or e < pe or (b - pb) + (e - pe) >= e - b:
        return True, e - b, 0
    return False, e - pe, b - pb


def unit_of(asked):
    return max(1, min(int(asked), TREE_UNIT_MAX))


def walk(levels, begins, lens, U):
    """What the item walk does at unit size U: dict of visits, added, subtracted, items, level_items (items per level) and
    skipped (steps that slide from a visited window to a later one across a window that did not visit the IBF)."""
    b = np.asarray(begins, dtype=np.int64)
    e = b + np.asarray(lens, dtype=np.int64)
    out = dict(visits=0, added=0, subtracted=0, items=0, skipped=0, level_items=[])
    for level in levels:
        n_items = 0
        for qs in level.values():
            unit, pj = -1, -1
            for j in qs.tolist():
                first = j // U != unit
                n_items += first
                unit = j // U
                reset, add, sub = cw_step(first, b[pj], e[pj], b[j], e[j])
                out["added"] += int(add)
                out["subtracted"] += int(sub)
                out["skipped"] += (not reset) and j > pj + 1
                pj = j
            out["visits"] += len(qs)
        out["items"] += n_items
        out["level_items"].append(n_items)
    return out
