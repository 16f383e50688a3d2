// The host planning of `tetrex search` as plain functions: a query's threshold, the windows of a
// record, the runs of hit windows that become rows, and how windows and records are cut into device batches.  No txq call
// and no I/O: tests/native/search_plan_dump.cpp prints what these compute and tests/test_search_plan.py holds it to the Python
// restatements (tests/search_window_ref.py, tests/frame_window_ref.py).  The command (search_cmd.cpp) and the batchers
// (search_device.cpp) call them and restate nothing.
#pragma once
#include "../txq_frame_windows_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace tetrex {
namespace plan {

// t of a query of n values: -e E gives max(n - k E, 0) (q-gram lemma), --threshold F gives ceil(F n)
struct Threshold {
    bool by_fraction = false;
    double fraction = 0;
    uint64_t k = 0, errors = 0;
    uint64_t of(uint64_t n) const {
        if (by_fraction) return (uint64_t)std::ceil(fraction * (double)n);
        return n > k * errors ? n - k * errors : 0;
    }
};

// The windows of a record of L letters under --window W --step S are those of a frame of L residues
// (csrc/txq_frame_windows_plan.hpp): window j is txq::fw::window_at(record_windows(...), j), letters [a, a + len).
inline txq::fw::Frame record_windows(uint64_t L, uint32_t k, uint32_t W, uint32_t S) { return txq::fw::frame_plan(L, k, W, S); }

// The hits (.query: the window, .bin, .count) of one record, or one frame of it, sorted by bin and then by window: every
// maximal run of consecutive windows of one bin is handed to each(first, last, best) — its first and last hit and its best
// one, the highest count, the earliest window on a tie.
template <class Hit, class Each>
void for_each_run(const std::vector<Hit>& hits, Each&& each) {
    for (size_t i = 0; i < hits.size();) {
        size_t e = i + 1, best = i;
        while (e < hits.size() && hits[e].bin == hits[i].bin && hits[e].query == hits[e - 1].query + 1) {
            if (hits[e].count > hits[best].count) best = e;
            ++e;
        }
        each(hits[i], hits[e - 1], hits[best]);
        i = e;
    }
}

// --verify-windows: the CONFIRMED windows of one record (.query: the window, .bin, .count, .distance, .strand
// '+' or '-'; a window is there once per bin, on the strand that verification settled), sorted by bin, then strand (+ first),
// then window.  Every maximal run of consecutive windows of one (bin, strand) is one row: its first and last item, its best
// one by count (the highest, the earliest window on a tie: for_each_run's rule) and its nearest one (the least distance, the
// earliest window on a tie), as indexes into the items.  The rows come by bin, then by their first window, + before -.
struct WindowRun {
    size_t first, last, best, nearest;
};
template <class Item>
std::vector<WindowRun> confirmed_runs(const std::vector<Item>& items) {
    std::vector<WindowRun> runs;
    for (size_t i = 0; i < items.size();) {
        WindowRun r{i, i, i, i};
        size_t e = i + 1;
        while (e < items.size() && items[e].bin == items[i].bin && items[e].strand == items[i].strand && items[e].query == items[e - 1].query + 1) {
            if (items[e].count > items[r.best].count) r.best = e;
            if (items[e].distance < items[r.nearest].distance) r.nearest = e;
            r.last = e++;
        }
        runs.push_back(r);
        i = e;
    }
    std::stable_sort(runs.begin(), runs.end(), [&](const WindowRun& x, const WindowRun& y) {
        if (items[x.first].bin != items[y.first].bin) return items[x.first].bin < items[y.first].bin;
        return items[x.first].query < items[y.first].query;
    });
    return runs;
}

// --window-targets: the TARGET HITS of one record (confirmed_runs' items with .target, the hit record's place
// in its bin's file; a window is there once per bin and target, on the strand that verification settled for that target),
// sorted by bin, then target, then strand (+ first), then window.  The items of a (bin, target) are merged by
// confirmed_runs' rule, so every maximal run of consecutive windows that hit one target on one strand is one row, `nearest`
// being the run's nearest window to THAT target.  The rows come by bin, then target, then by their first window, + before -.
template <class Item>
std::vector<WindowRun> target_runs(const std::vector<Item>& items) {
    std::vector<WindowRun> runs;
    for (size_t a = 0; a < items.size();) {
        size_t b = a + 1;
        while (b < items.size() && items[b].bin == items[a].bin && items[b].target == items[a].target) ++b;
        for (const WindowRun& r : confirmed_runs(std::vector<Item>(items.begin() + (long)a, items.begin() + (long)b)))
            runs.push_back({r.first + a, r.last + a, r.best + a, r.nearest + a});
        a = b;
    }
    return runs;
}

// Device batches: batch i is the items [cut[i], cut[i + 1]); most_*: the largest batch's, for buffers sized before the first
// batch runs ("Host")
struct Cuts {
    std::vector<size_t> cut{0};
    uint64_t most_values = 0, most_bytes = 0;
    size_t most_items = 0;
};

// Sliding windows (begins and begins + lens do not decrease) cut greedily: a batch ends at a window boundary, holds at most
// max_windows windows and spans at most max_values values from its first window's begin to its last window's end; a window
// longer than that is a batch of its own.
inline Cuts cut_windows(const std::vector<uint64_t>& begins, const std::vector<uint32_t>& lens, uint64_t max_values, size_t max_windows) {
    Cuts c;
    const size_t N = begins.size();
    for (size_t j0 = 0; j0 < N;) {
        size_t j1 = j0;
        while (j1 < N && j1 - j0 < max_windows && (j1 == j0 || begins[j1] + lens[j1] - begins[j0] <= max_values)) ++j1;
        c.most_items = std::max(c.most_items, j1 - j0);
        c.most_values = std::max(c.most_values, begins[j1 - 1] + lens[j1 - 1] - begins[j0]);
        c.cut.push_back(j0 = j1);
    }
    return c;
}

// Records (record r: bytes rec_offsets[r] .. rec_offsets[r + 1], at most bound_of(r) values) cut greedily: a batch holds at
// most max_values values by their bounds and at most max_records records (0: any number); a record above the bound on values
// is a batch of its own.
template <class Bound>
Cuts cut_records(const std::vector<uint64_t>& rec_offsets, Bound&& bound_of, uint64_t max_values, size_t max_records) {
    Cuts c;
    const size_t R = rec_offsets.empty() ? 0 : rec_offsets.size() - 1;
    for (size_t r0 = 0; r0 < R;) {
        size_t r1 = r0;
        uint64_t bound = 0;
        while (r1 < R) {
            const uint64_t b = bound_of(r1);
            if (r1 > r0 && (bound + b > max_values || (max_records && r1 - r0 >= max_records))) break;
            bound += b;
            ++r1;
        }
        c.most_values = std::max(c.most_values, bound);
        c.most_bytes = std::max(c.most_bytes, rec_offsets[r1] - rec_offsets[r0]);
        c.most_items = std::max(c.most_items, r1 - r0);
        c.cut.push_back(r0 = r1);
    }
    return c;
}

}  // namespace plan
}  // namespace tetrex
