// The unit cut and the entering and leaving ranges of the sliding window count (txq_count_windows, txq_count.hip; DESIGN.md
// §17), where a CPU can run them.  Plain functions, no HIP: the kernel calls them and does not restate them, and
// tests/native/count_windows_sim.cpp walks units and windows with the same functions under sanitizers.
//
// Window j owns values [begin[j], begin[j] + len[j]); begin and begin + len are non-decreasing.  A unit is U consecutive
// windows, counted by one workgroup that keeps the CURRENT window's counters: the unit's first window is counted in full, and
// every next one from its predecessor — the values that enter are added, those that leave are subtracted — unless the two
// do not overlap, or sliding would touch at least as many values as counting the window anew: then the counters are zeroed
// and the window is counted in full.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TXQ_CW_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define TXQ_CW_FN inline __attribute__((always_inline))
#endif

namespace txq {

constexpr uint32_t kCountWindowsUnitDefault = 16;  // TXQ_COUNT_WINDOWS_UNIT (DESIGN.md §17 has the measurement)
constexpr uint32_t kCountWindowsUnitMax = 1u << 20;

// units of U windows that n_windows make, and the windows [first, last) of unit u
TXQ_CW_FN uint64_t cw_units(uint64_t n_windows, uint32_t U) { return (n_windows + U - 1) / U; }
TXQ_CW_FN uint64_t cw_unit_first(uint64_t u, uint32_t U) { return u * U; }
TXQ_CW_FN uint64_t cw_unit_last(uint64_t u, uint32_t U, uint64_t n_windows) {
    const uint64_t e = (u + 1) * U;
    return e < n_windows ? e : n_windows;
}

// What turns the counters of the window before, [pb, pe), into those of window [b, e): zero them first (reset), add the
// values [add_lo, add_hi), subtract the values [sub_lo, sub_hi).  A range with lo >= hi is empty.
struct CwStep {
    bool reset;
    uint64_t add_lo, add_hi, sub_lo, sub_hi;
};

// first: the window opens its unit (the counters hold nothing of a predecessor; pb, pe are not looked at)
TXQ_CW_FN CwStep cw_step(bool first, uint64_t pb, uint64_t pe, uint64_t b, uint64_t e) {
    CwStep s{true, b, e, 0, 0};
    if (first || b >= pe) return s;                 // no predecessor, or nothing shared with it (an empty one included)
    if (b < pb || e < pe) return s;                 // (not a sliding sequence: every window of it is still counted within itself)
    // pb <= b < pe <= e: the windows share [b, pe)
    if ((b - pb) + (e - pe) >= e - b) return s;     // sliding reads no fewer rows than counting anew
    s.reset = false;
    s.add_lo = pe, s.add_hi = e;
    s.sub_lo = pb, s.sub_hi = b;
    return s;
}

}  // namespace txq
