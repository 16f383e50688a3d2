// The unit cut of the flat threshold count (txq_count on a flat IBF, txq_count.hip count_flat_kernel) and the two formulas by
// which its launchers cut a call into device calls, where a CPU can run them.  Plain functions on numbers and on the offsets
// array, no HIP call: the kernels and launchers call them and do not restate them, and tests/native/count_units_sim.cpp walks
// the units with the same functions under sanitizers.
//
// Query q owns values [offsets[q], offsets[q+1]).  The value range [offsets[0], offsets[nq]) is cut into units of `seg`
// values (seg_len).  A unit nominally starts at base + u * seg; it really starts there only if that position is the first
// value of a query or lies in a query longer than `seg` (unit_start): a query of at most `seg` values is left whole to the
// unit that holds its first value, counted by ONE workgroup and written directly.  A longer query is spread over units that
// add their partial counts to its accumulator row.
#pragma once
#include "txq_records.hpp"
#include <stddef.h>

#define TXQ_COUNT_FN TXQ_HOST_DEVICE inline __attribute__((always_inline))

namespace txq {

static constexpr uint64_t kSegMin = 512;        // values per unit of the flat kernel, at least ...
static constexpr uint64_t kTargetUnits = 8192;  // ... and about this many units per call
static constexpr unsigned kCountGrid = 4096;    // waves of a call (persistent: the work is only known on the device)

static constexpr size_t kCountAccBytes = (size_t)256 << 20;  // scratch accumulators of a flat call without counts, at most
static constexpr size_t kHibfCapItems = (size_t)1 << 24;     // (query, IBF) items a level's frontier buffer holds, about

// values per unit of a call of n values
TXQ_COUNT_FN uint64_t seg_len(uint64_t n) {
    const uint64_t s = (n + kTargetUnits - 1) / kTargetUnits;
    return s > kSegMin ? s : kSegMin;
}

// the query that holds value index x (offsets[0] <= x < offsets[nq]): the last q with offsets[q] <= x < offsets[q+1]
TXQ_COUNT_FN uint32_t query_of(const uint64_t* off, uint32_t nq, uint64_t x) {
    uint32_t lo = 1, hi = nq;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid] > x) hi = mid;
        else lo = mid + 1;
    }
    return lo - 1;
}

// where the unit that nominally starts at x really starts: x, unless x falls inside a query of at most `seg` values (that
// query is left whole to the unit before)
TXQ_COUNT_FN uint64_t unit_start(const uint64_t* off, uint32_t nq, uint64_t end, uint64_t seg, uint64_t x) {
    if (x >= end) return end;
    const uint32_t q = query_of(off, nq, x);
    const uint64_t a = off[q], b = off[q + 1];
    return a == x || b - a > seg ? x : b;
}

// Queries per device call of a flat call WITHOUT counts: long queries add their partial counts to a scratch row of
// row_u32 = 64 W u32 each, and the scratch holds kCountAccBytes.  (With counts the caller's array is the scratch: one call.)
TXQ_COUNT_FN size_t count_flat_per_call(size_t nq, size_t row_u32) {
    const size_t fit = kCountAccBytes / (row_u32 * 4);
    const size_t n = nq < fit ? nq : fit;
    return n > 1 ? n : 1;
}

// Queries per device call of an HIBF call: a (query, IBF) pair occurs at most once, so level l holds at most
// chunk * (IBFs on level l) items, and chunk * max_level_width is what a frontier buffer must hold.
TXQ_COUNT_FN size_t count_hibf_chunk(size_t nq, size_t max_level_width) {
    const size_t fit = kHibfCapItems / max_level_width;
    const size_t c = fit > 1 ? fit : 1;
    return c < nq ? c : nq;
}

}  // namespace txq
