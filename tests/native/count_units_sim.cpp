// Stand-alone check of csrc/txq_count_plan.hpp: the walk of count_flat_kernel (txq_count.hip) over the units of a flat call on
// the CPU — seg_len, unit_start at either end of every unit, query_of at its first value, then query by query as the kernel
// steps, empty queries skipped as it skips them — and the tests by which count_zero_long_kernel and count_finish_kernel pick
// their queries.  Checked for every offsets array:
//   * every value of [offsets[0], offsets[nq]) is counted by exactly one unit, under the query that owns it;
//   * a query of at most `seg` values is counted by one unit in one piece, and written directly exactly once;
//   * a longer query is only ever added to its accumulator, and exactly those rows are zeroed beforehand;
//   * count_finish_kernel's test picks exactly the empty queries and the queries not written directly;
//   * no read of `offsets` outside [0, nq]: the array is a heap block of exactly nq + 1 words, so one is an address error.
// The launchers' two formulas (count_flat_per_call, count_hibf_chunk) are checked against their definitions in words.
// Built with sanitizers by tests/test_count_units_sim.py:
//   g++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/count_units_sim.cpp -o sim && ./sim
// Prints "count_units_sim ok: <cases> cases, <queries> queries, <units> units, <long> long, <second> second-items" and exits 0, or names the
// first thing that differs and exits 1.  (second-items: units a grid of kCountGrid workgroups reaches only on a later round.)
#include "../../tetrex_amd/csrc/txq_count_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace txq;

namespace {

struct Case {
    std::string name;
    std::vector<uint64_t> lens;
};

size_t g_cases = 0, g_queries = 0, g_units = 0, g_long = 0, g_second = 0;

#define FAIL(...)                                                                   \
    do {                                                                            \
        std::printf("count_units_sim: case '%s', base %llu: ", c.name.c_str(), (unsigned long long)base0); \
        std::printf(__VA_ARGS__);                                                   \
        std::printf("\n");                                                          \
        return false;                                                               \
    } while (0)

// one call of count_flat: count_zero_long_kernel, count_flat_kernel, count_finish_kernel on offsets that start at base0
bool run(const Case& c, uint64_t base0) {
    const uint32_t nq = (uint32_t)c.lens.size();
    uint64_t* off = (uint64_t*)std::malloc(((size_t)nq + 1) * 8);  // exactly nq + 1 words: ASan sees one past and one before
    off[0] = base0;
    for (uint32_t q = 0; q < nq; ++q) off[q + 1] = off[q] + c.lens[q];
    const uint64_t base = off[0], end = off[nq];
    std::vector<uint8_t> zeroed(nq, 0), finished(nq, 0);
    std::vector<uint32_t> direct(nq, 0), added(nq, 0);
    std::vector<uint64_t> counted(nq, 0);
    std::vector<uint8_t> cover((size_t)(end - base), 0);
    ++g_cases, g_queries += nq;

    // count_zero_long_kernel
    if (end > base) {
        const uint64_t seg = seg_len(end - base);
        for (uint32_t q = 0; q < nq; ++q)
            if (off[q + 1] - off[q] > seg) zeroed[q] = 1;
    }
    // count_flat_kernel (one column tile: the tiles repeat the same walk)
    uint64_t seg = 0;
    if (end > base) {
        seg = seg_len(end - base);
        const uint64_t n_units = (end - base + seg - 1) / seg;
        if (seg < kSegMin || n_units > kTargetUnits || n_units * seg < end - base) FAIL("seg %llu gives %llu units", (unsigned long long)seg, (unsigned long long)n_units);
        uint64_t prev_hi = base;
        for (uint64_t u = 0; u < n_units; ++u) {
            const uint64_t lo = unit_start(off, nq, end, seg, base + u * seg);
            const uint64_t hi = u + 1 == n_units ? end : unit_start(off, nq, end, seg, base + (u + 1) * seg);
            if (lo != prev_hi && !(lo >= hi)) FAIL("unit %llu starts at %llu, the unit before ended at %llu", (unsigned long long)u, (unsigned long long)lo, (unsigned long long)prev_hi);
            if (lo >= hi) continue;
            prev_hi = hi;
            ++g_units;
            if (u >= kCountGrid) ++g_second;
            uint32_t q = query_of(off, nq, lo);
            if (q >= nq || off[q] > lo || off[q + 1] <= lo) FAIL("query_of(%llu) = %u", (unsigned long long)lo, q);
            uint64_t pos = lo;
            while (pos < hi) {
                if (q >= nq) FAIL("unit %llu walks past the last query", (unsigned long long)u);
                const uint64_t qb = off[q], qe = off[q + 1];
                const uint64_t stop = qe < hi ? qe : hi;
                if (pos < qb || stop <= pos) FAIL("unit %llu counts [%llu, %llu) under query %u = [%llu, %llu)", (unsigned long long)u, (unsigned long long)pos,
                                                 (unsigned long long)stop, q, (unsigned long long)qb, (unsigned long long)qe);
                for (uint64_t i = pos; i < stop; ++i) ++cover[(size_t)(i - base)];
                counted[q] += stop - pos;
                const bool whole = qe - qb <= seg;
                if (whole) {
                    if (pos != qb || stop != qe) FAIL("query %u of %llu values (seg %llu) is written directly from [%llu, %llu) of unit %llu", q,
                                                      (unsigned long long)(qe - qb), (unsigned long long)seg, (unsigned long long)pos, (unsigned long long)stop, (unsigned long long)u);
                    ++direct[q];
                } else {
                    if (!zeroed[q]) FAIL("query %u is added to an accumulator that was not zeroed", q);
                    ++added[q];
                }
                pos = stop;
                if (pos < hi) {
                    ++q;
                    while (off[q + 1] <= pos) ++q;  // (reads off[q + 1]: q + 1 <= nq or ASan stops here)
                }
            }
        }
        if (prev_hi != end) FAIL("the last unit ends at %llu of %llu", (unsigned long long)prev_hi, (unsigned long long)end);
    }
    // count_finish_kernel
    for (uint32_t q = 0; q < nq; ++q) {
        const uint64_t len = off[q + 1] - off[q];
        if (len && len <= seg) continue;
        finished[q] = 1;
    }

    for (size_t i = 0; i < cover.size(); ++i)
        if (cover[i] != 1) FAIL("value %llu is counted %u times", (unsigned long long)(base + i), (unsigned)cover[i]);
    for (uint32_t q = 0; q < nq; ++q) {
        const uint64_t len = c.lens[q];
        const bool is_long = seg && len > seg;
        g_long += is_long;
        if (counted[q] != len) FAIL("query %u: %llu of its %llu values counted", q, (unsigned long long)counted[q], (unsigned long long)len);
        if (len == 0 && (direct[q] || added[q] || zeroed[q] || !finished[q])) FAIL("empty query %u: direct %u, added %u, zeroed %d, finished %d", q, direct[q], added[q], zeroed[q], finished[q]);
        if (len && !is_long && (direct[q] != 1 || added[q] || zeroed[q] || finished[q]))
            FAIL("query %u of %llu <= seg %llu values: direct %u, added %u, zeroed %d, finished %d", q, (unsigned long long)len, (unsigned long long)seg, direct[q], added[q], zeroed[q], finished[q]);
        if (is_long && (direct[q] || !added[q] || !zeroed[q] || !finished[q]))
            FAIL("query %u of %llu > seg %llu values: direct %u, added %u, zeroed %d, finished %d", q, (unsigned long long)len, (unsigned long long)seg, direct[q], added[q], zeroed[q], finished[q]);
        if (finished[q] == (direct[q] != 0)) FAIL("query %u is written %s", q, finished[q] ? "twice" : "by nobody");
    }
    std::free(off);
    return true;
}

// lengths that cycle through the edges of `seg`, then filler, `total` values in all
Case edges_to_total(const char* name, uint64_t total, std::mt19937_64& rng) {
    const uint64_t seg = seg_len(total);
    Case c{name, {}};
    const uint64_t cycle[] = {seg - 1, seg, seg + 1, 1, 0, 0, 2 * seg + 3, 64};
    uint64_t sum = 0;
    for (size_t i = 0; sum < total; ++i) {
        uint64_t n = i % 11 < 8 ? cycle[i % 11] : 200 + rng() % 600;
        if (i % 13 == 12) {  // this query begins at most 3 values before a nominal unit boundary
            const uint64_t to = (seg - sum % seg) % seg, k = rng() % 4;
            if (to > k && sum + to - k < total) c.lens.push_back(to - k), sum += to - k;
        }
        n = std::min(n, total - sum);
        c.lens.push_back(n), sum += n;
    }
    return c;
}

std::vector<Case> cases() {
    std::mt19937_64 rng(20240911);
    std::vector<Case> cs;
    const uint64_t S = kSegMin;
    cs.push_back({"no queries", {}});
    cs.push_back({"all empty", {0, 0, 0, 0, 0}});
    for (uint64_t n : {(uint64_t)0, (uint64_t)1, S - 1, S, S + 1, 2 * S, 2 * S + 1, (uint64_t)5000}) cs.push_back({"one query of " + std::to_string(n), {n}});
    // runs of empty queries at a unit's first and last position (nominal boundaries at multiples of 512)
    cs.push_back({"empty runs at boundaries", {S, 0, 0, 0, S, 0, 0, 100, 0, 0, 0, S - 100, 0, S, 0, 0}});
    cs.push_back({"empty runs around short queries", {0, 0, S - 1, 0, 0, 1, 0, 0, S, 0, 0, 0, 1, 0, S - 1, 0, 0}});
    cs.push_back({"empty runs inside and around long queries", {0, 0, 2 * S, 0, 0, S + 1, 0, 0, 0, 3 * S, 0, 1, 0, 0, 2 * S + 5, 0, 0}});
    cs.push_back({"empty first and last", {0, 700, 0}});
    cs.push_back({"empty runs first and last", {0, 0, 0, S, S + 1, 1, 0, 0, 0}});
    // seg - 1, seg, seg + 1 and 2 seg in every order, alone and with a short query between
    {
        std::vector<uint64_t> e{S - 1, S, S + 1, 2 * S};
        std::sort(e.begin(), e.end());
        do {
            cs.push_back({"edge lengths", e});
            Case c{"edge lengths with short queries", {}};
            for (uint64_t n : e) c.lens.push_back(n), c.lens.push_back(3), c.lens.push_back(0);
            cs.push_back(c);
        } while (std::next_permutation(e.begin(), e.end()));
    }
    // a query of at most seg values that begins 0 .. 3 values before a nominal boundary, behind a short and behind a long query
    for (uint64_t k = 0; k < 4; ++k)
        for (uint64_t n : {(uint64_t)1, (uint64_t)5, S - 1, S, S + 1})
            for (uint64_t first : {S - k, 3 * S - k, 2 * S + 7 - k}) cs.push_back({"begins just before a boundary", {first, n, 40, 0, S}});
    // the default seg: lengths of tests/test_gpu_count_scale.py
    {
        Case c{"boundary batch", {511, 512, 513, 0, 1, 512, 512, 1024, 1025, 3, 0}};
        cs.push_back(c);
        std::reverse(c.lens.begin(), c.lens.end());
        cs.push_back(c);
    }
    // totals just below and above kTargetUnits * kSegMin: seg 512, 512, 513, 513, 525
    for (uint64_t total : {kTargetUnits * S - 1, kTargetUnits * S, kTargetUnits * S + 1, kTargetUnits * (S + 1), (uint64_t)4300800}) {
        cs.push_back(edges_to_total("edges up to a total", total, rng));
        Case one{"one query of a total", {total}};
        cs.push_back(one);
        Case many{"short queries up to a total", {}};
        for (uint64_t sum = 0; sum < total;) {
            const uint64_t n = std::min<uint64_t>(total - sum, rng() % 5 ? 300 + rng() % 400 : 0);
            many.lens.push_back(n), sum += n;
        }
        cs.push_back(many);
    }
    // random mixes: empty, tiny, about seg, long
    for (int i = 0; i < 400; ++i) {
        Case c{"random " + std::to_string(i), {}};
        const size_t nq = 1 + rng() % 60;
        const unsigned empty_in_8 = rng() % 8;
        for (size_t q = 0; q < nq; ++q) {
            const unsigned kind = rng() % 8;
            if (kind < empty_in_8 / 2) c.lens.push_back(0);
            else if (kind < 5) c.lens.push_back(rng() % 40);
            else if (kind < 7) c.lens.push_back(S - 3 + rng() % 7);
            else c.lens.push_back(S + 1 + rng() % (4 * S));
        }
        cs.push_back(c);
    }
    return cs;
}

bool formulas() {
    // count_flat_per_call: as many queries as 256 MiB of u32 rows hold, at least one, no more than there are
    for (size_t W : {(size_t)1, (size_t)2, (size_t)141, (size_t)257, (size_t)1 << 20})
        for (size_t nq : {(size_t)1, (size_t)2, (size_t)7436, (size_t)7437, (size_t)7500, (size_t)1 << 24}) {
            const size_t row = W * 64, p = count_flat_per_call(nq, row);
            const bool fits = p * row * 4 <= ((size_t)256 << 20);
            if (p < 1 || p > nq || (!fits && p != 1) || (p < nq && (p + 1) * row * 4 <= ((size_t)256 << 20))) {
                std::printf("count_units_sim: count_flat_per_call(%zu, %zu) = %zu\n", nq, row, p);
                return false;
            }
        }
    if (count_flat_per_call(7500, 141 * 64) != 7436 || count_hibf_chunk(508460, 33) != 508400) {  // (9000 bins: 141 words)
        std::printf("count_units_sim: count_flat_per_call(7500, 9024) = %zu, count_hibf_chunk(508460, 33) = %zu\n", count_flat_per_call(7500, 141 * 64), count_hibf_chunk(508460, 33));
        return false;
    }
    // count_hibf_chunk: chunk * width <= 2^24 items unless one query alone exceeds it
    for (size_t width : {(size_t)1, (size_t)33, (size_t)128, (size_t)1 << 25})
        for (size_t nq : {(size_t)1, (size_t)42, (size_t)508400, (size_t)508460, (size_t)1 << 26}) {
            const size_t ch = count_hibf_chunk(nq, width);
            if (ch < 1 || ch > nq || (ch > 1 && ch * width > ((size_t)1 << 24)) || (ch < nq && (ch + 1) * width <= ((size_t)1 << 24))) {
                std::printf("count_units_sim: count_hibf_chunk(%zu, %zu) = %zu\n", nq, width, ch);
                return false;
            }
        }
    return true;
}

}  // namespace

int main() {
    if (!formulas()) return 1;
    for (const Case& c : cases())
        for (uint64_t base0 : {(uint64_t)0, (uint64_t)1000003})  // offsets[0] != 0: a later device call of one host call
            if (!run(c, base0)) return 1;
    std::printf("count_units_sim ok: %zu cases, %zu queries, %zu units, %zu long, %zu second-items\n", g_cases, g_queries, g_units, g_long, g_second);
    return 0;
}
