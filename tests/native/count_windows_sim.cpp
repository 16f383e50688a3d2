// Stand-alone check of csrc/txq_count_windows_plan.hpp: the walk of count_windows_kernel (txq_count.hip) over units and
// windows on the CPU — the unit cut, the entering range added, the leaving range subtracted, the counters zeroed where
// cw_step says so, u32 counters that are never cleared in between — over a synthetic membership bit per (value, bin), against
// a recount of every window from nothing.  The value array is a heap block of exactly the values the windows span, so a range
// outside them is an address error.  Built with sanitizers by tests/test_count_windows_sim.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/count_windows_sim.cpp -o sim && ./sim
// Prints "count_windows_sim ok: <cases> cases, <windows> windows, <slid> slid" and exits 0, or names the first window that differs
// and exits 1.
#include "../../tetrex_amd/csrc/txq_count_windows_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace txq;

namespace {

constexpr uint32_t kBins = 8;

struct Windows {
    const char* name;
    std::vector<uint64_t> begin;
    std::vector<uint32_t> len;
};

// is value v in bin b?  (about half of the pairs)
bool member(uint64_t v, uint32_t b) {
    uint64_t x = (v * kBins + b) * 0x9E3779B97F4A7C15ull;
    x ^= x >> 29;
    x *= 0xBF58476D1CE4E5B9ull;
    return (x >> 40) & 1u;
}

Windows sliding(const char* name, uint32_t len, uint64_t step, size_t n) {
    Windows w{name, {}, {}};
    for (size_t j = 0; j < n; ++j) w.begin.push_back(j * step), w.len.push_back(len);
    return w;
}

std::vector<Windows> window_sets() {
    std::vector<Windows> sets;
    for (uint32_t len : {0u, 1u, 63u, 64u, 65u, 300u})
        for (uint64_t step : {(uint64_t)1, (uint64_t)7, (uint64_t)len, (uint64_t)len + 5})
            for (size_t n : {(size_t)0, (size_t)1, (size_t)37, (size_t)130}) sets.push_back(sliding("sliding", len, step, n));
    {   // a length that shrinks, then grows: begin and end still do not decrease
        Windows w{"shrinking then growing", {}, {}};
        uint64_t b = 0, e = 80;
        for (int j = 0; j < 50; ++j) {
            w.begin.push_back(b), w.len.push_back((uint32_t)(e - b));
            if (j < 25) b += 3, e += 1;  // shrinks by 2 a window, down to 30
            else b += 1, e += 6;         // grows by 5 a window
        }
        sets.push_back(w);
    }
    {   // the end-aligned tail window of `tetrex search --window`: closer than the step to its predecessor
        for (uint64_t total : {(uint64_t)101, (uint64_t)149, (uint64_t)150, (uint64_t)151}) {
            Windows w{"end-aligned tail", {}, {}};
            const uint32_t len = 50;
            const uint64_t step = 25;
            uint64_t at = 0;
            for (; at + len <= total; at += step) w.begin.push_back(at), w.len.push_back(len);
            if (w.begin.back() + len < total) w.begin.push_back(total - len), w.len.push_back(len);
            sets.push_back(w);
        }
    }
    {   // every window three times
        Windows w{"repeated", {}, {}};
        for (int j = 0; j < 40; ++j) w.begin.push_back((uint64_t)(j / 3) * 9), w.len.push_back(70u);
        sets.push_back(w);
    }
    {   // windows with gaps between them and an empty window in every gap
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

}  // namespace

int main() {
    std::mt19937_64 rng(20240607);
    size_t cases = 0, windows = 0, slid = 0;
    for (const Windows& w : window_sets()) {
        const size_t n = w.begin.size();
        uint64_t n_values = 0;
        for (size_t j = 0; j < n; ++j) {
            n_values = std::max(n_values, w.begin[j] + w.len[j]);
            if (j && (w.begin[j] < w.begin[j - 1] || w.begin[j] + w.len[j] < w.begin[j - 1] + w.len[j - 1])) {
                std::printf("count_windows_sim: the set '%s' does not slide at window %zu\n", w.name, j);
                return 1;
            }
        }
        uint64_t* values = (uint64_t*)std::malloc(n_values ? n_values * 8 : 1);  // exactly the values: ASan sees one past
        for (uint64_t i = 0; i < n_values; ++i) values[i] = rng() % 97;          // (values repeat)
        for (uint32_t U : {1u, 2u, 3u, 16u, 64u}) {
            ++cases;
            std::vector<uint32_t> done(n, 0);
            for (uint64_t u = 0; u < cw_units(n, U); ++u) {
                uint32_t cnt[kBins];
                std::memset(cnt, 0xA5, sizeof cnt);  // (the first window of a unit must reset)
                uint64_t pb = 0, pe = 0;
                const uint64_t j0 = cw_unit_first(u, U), j1 = cw_unit_last(u, U, n);
                if (j0 >= j1 || j1 > n) {
                    std::printf("count_windows_sim: unit %llu of U = %u is windows %llu..%llu of %zu\n", (unsigned long long)u, U, (unsigned long long)j0, (unsigned long long)j1, n);
                    return 1;
                }
                for (uint64_t j = j0; j < j1; ++j) {
                    const uint64_t b = w.begin[j], e = b + w.len[j];
                    const CwStep st = cw_step(j == j0, pb, pe, b, e);
                    if (st.reset) std::memset(cnt, 0, sizeof cnt);
                    else ++slid;
                    for (uint64_t i = st.add_lo; i < st.add_hi; ++i)
                        for (uint32_t bin = 0; bin < kBins; ++bin) cnt[bin] += member(values[i], bin);
                    for (uint64_t i = st.sub_lo; i < st.sub_hi; ++i)
                        for (uint32_t bin = 0; bin < kBins; ++bin) cnt[bin] -= member(values[i], bin);
                    for (uint32_t bin = 0; bin < kBins; ++bin) {
                        uint32_t want = 0;
                        for (uint64_t i = b; i < e; ++i) want += member(values[i], bin);
                        if (cnt[bin] != want) {
                            std::printf("count_windows_sim: set '%s' (%zu windows, first length %u), U = %u, window %llu [%llu, %llu) after [%llu, %llu), bin %u: "
                                        "count %u, recount %u (reset %d, add [%llu, %llu), subtract [%llu, %llu))\n",
                                        w.name, n, n ? w.len[0] : 0u, U, (unsigned long long)j, (unsigned long long)b, (unsigned long long)e,
                                        (unsigned long long)pb, (unsigned long long)pe, bin, cnt[bin], want, (int)st.reset, (unsigned long long)st.add_lo,
                                        (unsigned long long)st.add_hi, (unsigned long long)st.sub_lo, (unsigned long long)st.sub_hi);
                            return 1;
                        }
                    }
                    // a slide never touches more values than the window holds
                    if (!st.reset && (st.add_hi - st.add_lo) + (st.sub_hi - st.sub_lo) >= e - b) {
                        std::printf("count_windows_sim: set '%s', U = %u, window %llu slides over more values than it holds\n", w.name, U, (unsigned long long)j);
                        return 1;
                    }
                    ++done[j], ++windows;
                    pb = b, pe = e;
                }
            }
            for (size_t j = 0; j < n; ++j)
                if (done[j] != 1) {
                    std::printf("count_windows_sim: set '%s', U = %u: window %zu counted %u times\n", w.name, U, j, done[j]);
                    return 1;
                }
        }
        std::free(values);
    }
    std::printf("count_windows_sim ok: %zu cases, %zu windows, %zu slid\n", cases, windows, slid);
    return 0;
}
