// Stand-alone check of csrc/txq_count_windows_tree_plan.hpp: the walk of count_windows_tree_kernel (txq_count.hip) on the CPU.
// A synthetic tree of 3 levels — merged bins, user bins and runs of split bins, a membership bit per (value, IBF, technical
// bin) — is descended level by level with the plan header's functions only: the level-0 mask of a unit, the walk over an
// item's set bits with cw_step between two VISITED windows, the mask word per merged bin, the items of the next level, and
// the cut of a call into device calls whose frontier buffer is a heap block of exactly cwt_frontier_items items.  One set of
// counters and mask words serves all items of a level, as a wave's LDS does: the counters are poisoned before the first
// item and never cleaned, the mask words must be zero when an item begins.  Checked against an independent recount and
// descent of every window on its own: every (window, IBF) count vector, every child's visit set, hits and counts per user
// bin, and the added and subtracted totals against cw_step summed over every IBF's visiting windows.
// Built with sanitizers by tests/test_count_windows_tree_sim.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/count_windows_tree_sim.cpp -o sim && ./sim
// Prints "count_windows_tree_sim ok: <cases> cases, <visits> visits, <slid> slid, <skipped> slid across a window that did not visit"
// and exits 0, or names the first difference and exits 1.
#include "../../tetrex_amd/csrc/txq_count_windows_tree_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <vector>

using namespace txq;

namespace {

constexpr int kMerged = -1;

struct Tb {
    int user;   // user bin, or kMerged
    int child;  // IBF of a merged bin
};
struct Ibf {
    int level;
    std::vector<Tb> tb;
};

// 3 levels, widths 1, 3, 3; user bins 0 .. 12; runs of 2 and 3 split bins, two runs of user bin 5 that are not adjacent
std::vector<Ibf> make_tree() {
    const int M = kMerged;
    std::vector<Ibf> t(7);
    t[0] = {0, {{M, 1}, {0, 0}, {0, 0}, {M, 2}, {1, 0}, {M, 3}}};
    t[1] = {1, {{M, 4}, {2, 0}, {2, 0}, {2, 0}, {3, 0}}};
    t[2] = {1, {{4, 0}, {M, 5}, {5, 0}, {M, 6}, {5, 0}, {5, 0}}};
    t[3] = {1, {{6, 0}, {7, 0}}};
    t[4] = {2, {{8, 0}, {9, 0}, {9, 0}}};
    t[5] = {2, {{10, 0}}};
    t[6] = {2, {{11, 0}, {11, 0}, {12, 0}}};
    return t;
}
constexpr int kUserBins = 13;
constexpr size_t kMaxLevelWidth = 3, kDepth = 3, kMaxTbs = 6;

// is value v in technical bin b of IBF i?  (merged bins: about 0.6 of the pairs, user bins: about 0.45)
bool member(uint64_t v, int i, int b, bool merged) {
    uint64_t x = ((v * 7 + (uint64_t)i) * 8 + (uint64_t)b) * 0x9E3779B97F4A7C15ull;
    x ^= x >> 29;
    x *= 0xBF58476D1CE4E5B9ull;
    return ((x >> 40) % 100) < (merged ? 60u : 45u);
}

struct Windows {
    const char* name;
    std::vector<uint64_t> begin;
    std::vector<uint32_t> len;
};

Windows sliding(const char* name, uint32_t len, uint64_t step, size_t n) {
    Windows w{name, {}, {}};
    for (size_t j = 0; j < n; ++j) w.begin.push_back(j * step), w.len.push_back(len);
    return w;
}

// the window sets of tests/native/count_windows_sim.cpp
std::vector<Windows> window_sets() {
    std::vector<Windows> sets;
    for (uint32_t len : {0u, 1u, 63u, 64u, 65u, 300u})
        for (uint64_t step : {(uint64_t)1, (uint64_t)7, (uint64_t)len, (uint64_t)len + 5})
            for (size_t n : {(size_t)0, (size_t)1, (size_t)37, (size_t)130}) sets.push_back(sliding("sliding", len, step, n));
    {
        Windows w{"shrinking then growing", {}, {}};
        uint64_t b = 0, e = 80;
        for (int j = 0; j < 50; ++j) {
            w.begin.push_back(b), w.len.push_back((uint32_t)(e - b));
            if (j < 25) b += 3, e += 1;
            else b += 1, e += 6;
        }
        sets.push_back(w);
    }
    for (uint64_t total : {(uint64_t)101, (uint64_t)149, (uint64_t)150, (uint64_t)151}) {
        Windows w{"end-aligned tail", {}, {}};
        const uint32_t len = 50;
        uint64_t at = 0;
        for (; at + len <= total; at += 25) w.begin.push_back(at), w.len.push_back(len);
        if (w.begin.back() + len < total) w.begin.push_back(total - len), w.len.push_back(len);
        sets.push_back(w);
    }
    {
        Windows w{"repeated", {}, {}};
        for (int j = 0; j < 40; ++j) w.begin.push_back((uint64_t)(j / 3) * 9), w.len.push_back(70u);
        sets.push_back(w);
    }
    {
        Windows w{"gaps with empty windows", {}, {}};
        for (int j = 0; j < 41; ++j) {
            const uint64_t b = (uint64_t)(j / 2) * 30;
            if (j % 2 == 0) w.begin.push_back(b), w.len.push_back(20u);
            else w.begin.push_back(b + 25), w.len.push_back(0u);
        }
        sets.push_back(w);
    }
    return sets;
}

struct Answer {
    std::vector<uint32_t> counts;  // [window][user bin]: the largest run sum
    std::vector<uint8_t> hits;     // [window][user bin]
};

// the technical-bin pass on the counters of window j on IBF f: user bins' runs into the answer, the merged bins that pass
void bin_pass(const Ibf& f, const uint32_t* cnt, uint32_t thr, size_t j, Answer& a, std::vector<int>& passed_merged) {
    for (size_t b = 0; b < f.tb.size(); ++b) {
        if (f.tb[b].user == kMerged) {
            if (cnt[b] >= thr) passed_merged.push_back((int)b);
        } else if (b + 1 == f.tb.size() || f.tb[b + 1].user != f.tb[b].user) {  // the last technical bin of a run
            uint32_t sum = cnt[b];
            for (size_t s = b; s > 0 && f.tb[s - 1].user == f.tb[b].user; --s) sum += cnt[s - 1];
            uint32_t& c = a.counts[j * kUserBins + f.tb[b].user];
            c = std::max(c, sum);
            if (sum >= thr) a.hits[j * kUserBins + f.tb[b].user] = 1;
        }
    }
}

int fail_at(const char* what, const Windows& w, uint32_t U, size_t cap, size_t j, int ibf) {
    std::printf("count_windows_tree_sim: %s: set '%s' (%zu windows, first length %u), U = %u, frontier cap %zu, window %zu, IBF %d\n", what, w.name,
                w.begin.size(), w.begin.empty() ? 0u : w.len[0], U, cap, j, ibf);
    return 1;
}

}  // namespace

int main() {
    // the call-cut formula at its edges
    if (cwt_units_per_call(1000, 1, 1u << 24) != 1000 || cwt_units_per_call((size_t)1 << 30, 1, 1u << 24) != ((size_t)1 << 24) ||
        cwt_units_per_call(1000, 3, 3) != 1 || cwt_units_per_call(1000, 3, 5) != 1 || cwt_units_per_call(1000, 3, 6) != 2 ||
        cwt_units_per_call(1000, 100, 7) != 1 || cwt_units_per_call(0, 3, 6) != 0 || cwt_units_per_call(1, 1, 1) != 1 ||
        cwt_frontier_items(2, 3) != 6 || cwt_frontier_items(1, 100) != 100 || cwt_unit(0) != 1 || cwt_unit(16) != 16 || cwt_unit(64) != 32 ||
        cwt_level0_mask(0, 32, 32) != 0xFFFFFFFFu || cwt_level0_mask(0, 32, 31) != 0x7FFFFFFFu || cwt_level0_mask(2, 3, 7) != 1u ||
        cwt_level0_mask(1, 16, 40) != 0xFFFFu || cwt_level0_mask(0, 1, 5) != 1u) {
        std::printf("count_windows_tree_sim: the call cut, the unit or the level-0 mask is off at an edge\n");
        return 1;
    }
    const std::vector<Ibf> tree = make_tree();
    std::mt19937_64 rng(20240923);
    size_t cases = 0, visits_all = 0, slid = 0, skipped = 0;
    for (const Windows& w : window_sets()) {
        const size_t n = w.begin.size();
        uint64_t n_values = 0;
        for (size_t j = 0; j < n; ++j) n_values = std::max(n_values, w.begin[j] + w.len[j]);
        uint64_t* values = (uint64_t*)std::malloc(n_values ? n_values * 8 : 1);  // exactly the values: ASan sees one past
        for (uint64_t i = 0; i < n_values; ++i) values[i] = rng() % 97;
        std::vector<uint32_t> thr(n);
        for (size_t j = 0; j < n; ++j) thr[j] = j % 11 == 5 ? 0u : j % 13 == 7 ? w.len[j] + 1u : (w.len[j] * 11u) / 20u;

        // every window on its own: recount on every visited IBF, descend where a merged bin passes
        Answer want{std::vector<uint32_t>(n * kUserBins, 0), std::vector<uint8_t>(n * kUserBins, 0)};
        std::map<std::pair<size_t, int>, std::vector<uint32_t>> want_cnt;  // (window, IBF) -> counts per technical bin
        std::vector<std::vector<size_t>> visitors(tree.size());               // IBF -> windows that visit it, ascending
        for (size_t j = 0; j < n; ++j) {
            std::vector<int> todo{0};
            while (!todo.empty()) {
                const int i = todo.back();
                todo.pop_back();
                const Ibf& f = tree[i];
                std::vector<uint32_t> c(f.tb.size(), 0);
                for (size_t b = 0; b < f.tb.size(); ++b)
                    for (uint64_t x = w.begin[j]; x < w.begin[j] + w.len[j]; ++x) c[b] += member(values[x], i, (int)b, f.tb[b].user == kMerged);
                std::vector<int> pm;
                bin_pass(f, c.data(), thr[j], j, want, pm);
                for (int b : pm) todo.push_back(f.tb[b].child);
                want_cnt[{j, i}] = c;
                visitors[i].push_back(j);
            }
        }
        for (auto& v : visitors) std::sort(v.begin(), v.end());

        for (uint32_t U_asked : {1u, 2u, 3u, 16u, 32u, 64u}) {
            const uint32_t U = cwt_unit(U_asked);
            // cw_step summed over every IBF's visiting windows, unit by unit: what the walk must add and subtract
            uint64_t want_added = 0, want_subtracted = 0;
            size_t want_items = 0;
            for (const auto& v : visitors) {
                uint64_t pb = 0, pe = 0, unit = UINT64_MAX;
                for (size_t j : v) {
                    const bool first = j / U != unit;
                    if (first) ++want_items;
                    unit = j / U;
                    const uint64_t b = w.begin[j], e = b + w.len[j];
                    const CwStep st = cw_step(first, pb, pe, b, e);
                    if (st.add_lo < st.add_hi) want_added += st.add_hi - st.add_lo;
                    if (st.sub_lo < st.sub_hi) want_subtracted += st.sub_hi - st.sub_lo;
                    pb = b, pe = e;
                }
            }
            for (size_t cap_items : {(size_t)1 << 24, (size_t)3, (size_t)7}) {  // one call; a single unit per call; two units per call
                if (cap_items != ((size_t)1 << 24) && U_asked == 64) continue;
                ++cases;
                const size_t n_units = (size_t)cw_units(n, U);
                const size_t per_call = cwt_units_per_call(n_units, kMaxLevelWidth, cap_items);
                const size_t cap = cwt_frontier_items(per_call, kMaxLevelWidth);
                if (n_units && (per_call < 1 || (cap_items == 3 && per_call != 1) || (cap_items == 7 && per_call != std::min<size_t>(2, n_units))))
                    return fail_at("units per call", w, U, cap_items, 0, 0);
                Answer got{std::vector<uint32_t>(n * kUserBins, 0), std::vector<uint8_t>(n * kUserBins, 0)};
                std::map<std::pair<size_t, int>, int> seen;
                uint64_t added = 0, subtracted = 0;
                size_t items = 0;
                uint32_t cnt[kMaxTbs], kid_mask[kMaxTbs];
                std::memset(cnt, 0xA5, sizeof cnt);  // (an item's first window must reset)
                std::memset(kid_mask, 0, sizeof kid_mask);
                for (size_t u0 = 0; u0 < n_units; u0 += per_call) {
                    const size_t nu = std::min(per_call, n_units - u0), j_call = (size_t)cw_unit_first(u0, U);
                    const size_t n_call = std::min(nu * U, n - j_call);  // the device call's windows: it starts at a unit boundary
                    CwTreeItem* frontier[2] = {(CwTreeItem*)std::malloc(cap * sizeof(CwTreeItem)), (CwTreeItem*)std::malloc(cap * sizeof(CwTreeItem))};
                    size_t level_items[kDepth + 1] = {nu, 0, 0, 0};
                    for (size_t lvl = 0; lvl < kDepth; ++lvl) {
                        const CwTreeItem* in = lvl ? frontier[(lvl - 1) & 1] : nullptr;
                        CwTreeItem* out = frontier[lvl & 1];
                        std::set<std::pair<uint32_t, uint32_t>> pairs;
                        for (size_t it = 0; it < level_items[lvl]; ++it) {
                            const uint32_t unit = in ? in[it].unit : (uint32_t)it, id = in ? in[it].ibf : 0u;
                            const uint32_t mask = in ? in[it].mask : cwt_level0_mask(unit, U, n_call);
                            const Ibf& f = tree[id];
                            if (!pairs.insert({unit, id}).second || (size_t)f.level != lvl || !mask) return fail_at("an item twice, on a wrong level or empty", w, U, cap_items, j_call + (size_t)unit * U, (int)id);
                            for (uint32_t m : kid_mask)
                                if (m) return fail_at("mask words not zero at the start of an item", w, U, cap_items, j_call + (size_t)unit * U, (int)id);
                            ++items;
                            uint32_t last_wi = 0;
                            bool any = false;
                            for (CwTreeWalk wk = cwt_walk(mask); cwt_more(wk);) {
                                const uint32_t wi = cwt_window(wk);
                                const size_t j = j_call + (size_t)cw_unit_first(unit, U) + wi;
                                if (wi >= U || j >= j_call + n_call || (any && wi <= last_wi)) return fail_at("a window outside its unit or out of order", w, U, cap_items, j, (int)id);
                                const uint64_t b = w.begin[j], e = b + w.len[j];
                                const CwStep st = cwt_advance(wk, b, e);
                                if (st.reset) std::memset(cnt, 0, sizeof cnt);
                                else {
                                    ++slid;
                                    if (wi > last_wi + 1) ++skipped;
                                }
                                if (!any && !st.reset) return fail_at("an item's first window does not reset", w, U, cap_items, j, (int)id);
                                for (uint64_t x = st.add_lo; x < st.add_hi; ++x)
                                    for (size_t bin = 0; bin < f.tb.size(); ++bin) cnt[bin] += member(values[x], (int)id, (int)bin, f.tb[bin].user == kMerged);
                                for (uint64_t x = st.sub_lo; x < st.sub_hi; ++x)
                                    for (size_t bin = 0; bin < f.tb.size(); ++bin) cnt[bin] -= member(values[x], (int)id, (int)bin, f.tb[bin].user == kMerged);
                                if (st.add_lo < st.add_hi) added += st.add_hi - st.add_lo;
                                if (st.sub_lo < st.sub_hi) subtracted += st.sub_hi - st.sub_lo;
                                const auto ref = want_cnt.find({j, (int)id});
                                if (ref == want_cnt.end()) return fail_at("a visit the independent descent does not make", w, U, cap_items, j, (int)id);
                                if (std::memcmp(ref->second.data(), cnt, f.tb.size() * 4)) return fail_at("counts differ from the recount", w, U, cap_items, j, (int)id);
                                ++seen[{j, (int)id}];
                                std::vector<int> pm;
                                bin_pass(f, cnt, thr[j], j, got, pm);
                                for (int bin : pm) kid_mask[bin] |= 1u << wi;
                                last_wi = wi, any = true;
                            }
                            for (size_t bin = 0; bin < f.tb.size(); ++bin)
                                if (kid_mask[bin]) {
                                    if (level_items[lvl + 1] >= cap) return fail_at("more items than the frontier buffer holds", w, U, cap_items, j_call, (int)id);
                                    out[level_items[lvl + 1]++] = CwTreeItem{unit, (uint32_t)f.tb[bin].child, kid_mask[bin]};
                                    kid_mask[bin] = 0;
                                }
                        }
                    }
                    if (level_items[kDepth]) return fail_at("items below the last level", w, U, cap_items, j_call, 0);
                    std::free(frontier[0]);
                    std::free(frontier[1]);
                }
                // every child's visit set is the independent descent's: every visit seen once, none else (checked above)
                if (seen.size() != want_cnt.size()) return fail_at("visits missing", w, U, cap_items, 0, 0);
                for (const auto& s : seen)
                    if (s.second != 1) return fail_at("a (window, IBF) pair visited twice", w, U, cap_items, s.first.first, s.first.second);
                if (got.counts != want.counts || got.hits != want.hits) return fail_at("hits or counts of user bins differ", w, U, cap_items, 0, 0);
                if (added != want_added || subtracted != want_subtracted || items != want_items) {
                    std::printf("added %llu (cw_step: %llu), subtracted %llu (%llu), items %zu (%zu)\n", (unsigned long long)added, (unsigned long long)want_added,
                                (unsigned long long)subtracted, (unsigned long long)want_subtracted, items, want_items);
                    return fail_at("totals differ from the sums of cw_step", w, U, cap_items, 0, 0);
                }
                visits_all += seen.size();
            }
        }
        std::free(values);
    }
    std::printf("count_windows_tree_sim ok: %zu cases, %zu visits, %zu slid, %zu slid across a window that did not visit\n", cases, visits_all, slid, skipped);
    return 0;
}
