// The host's half of the flat probe's domain table (txq_probe.hip probe_flat), and the one piece of arithmetic its kernels
// share: plain C++ on numbers (no HIP call, no Index, no Knobs), so that a CPU program can check it
// (tests/native/probe_plan_dump.cpp).
//   table_capacity   rows a call of n k-mers may give the table (0: the plain kernel)
//   table_rows       [lo, rows) = what the build writes, rows = what the answer reads from the table; both kernels call it
//   extend_rows      a one-launch (kept, fused) call: the rows valid after it, from the rows valid before it and the exact
//                    statistics the call before left
//   probe_slots      which state words call number c reads, adds into, writes and zeroes
//   plan_probe_call  is the table's content still the masks of the index's bits (keep), or does this call start over (fresh)?
#pragma once
#include "txq_records.hpp"
#include <algorithm>
#include <cstddef>

namespace txq {

static constexpr uint32_t kTableRatio = 4;     // n / D at which the table pays: (h + 1) / (h - 1) = 2 at h = 3, with margin
static constexpr uint32_t kDomainSample = 16;  // the domain pass reads 1 k-mer of 16
static constexpr uint32_t kTableMinRows = 1 << 14;
static constexpr size_t kBuildBlocks = 2048;    // most blocks of a build's grid (256 rows each before they grid-stride)

// Rows a call of n k-mers may give the table, 0: the plain path (the host's half of the gate; the device decides from D).
// probe_table: TXQ_PROBE_TABLE (0 never, 1 whenever it fits, -1 where it pays); table_mb: TXQ_KMER_TABLE_MB.
inline size_t table_capacity(int probe_table, long long table_mb, uint64_t bin_size, uint32_t stride, uint32_t hash_funs, size_t n) {
    if (probe_table == 0 || table_mb <= 0 || (bin_size >> 32) || stride < 2 || (stride & 1) || hash_funs < 2) return 0;
    const size_t budget = ((size_t)table_mb << 20) / ((size_t)stride * 8);
    size_t cap = probe_table == 1 ? std::max<size_t>(n, 1 << 16) : n / kTableRatio;
    cap = std::min(cap, budget) & ~(size_t)63;
    if (probe_table != 1 && cap < kTableMinRows) return 0;  // a batch this small does not pay for three launches
    return cap;
}

// What one call does with the table.  `built` = rows [0, built) hold the masks of the current bits (the device's word, as the
// last call left it), `top` / `count` = this call's sample: 1 + the largest sampled value below the call's capacity, and how
// many sampled values lie below it.  The domain D = top pays when the batch holds about ratio * D k-mers below D,
// count * sample >= ratio * D (ratio 0: whenever D != 0).  The build probes the values [lo, rows) into the table, the answer
// reads T[v] for v < rows.  A call's capacity may be smaller than an earlier call's (lo > top: nothing to build, the
// rows stay) but never exceeds the table's `cap_rows`; a D beyond it is not believed.
struct ProbeRows { uint32_t lo, rows; };
TXQ_HOST_DEVICE inline ProbeRows table_rows(bool fresh, uint32_t built, uint32_t top, uint32_t count, uint32_t ratio, uint32_t sample, uint32_t cap_rows) {
    const uint32_t lo = fresh ? 0u : built < cap_rows ? built : cap_rows;
    const bool pays = top != 0 && top <= cap_rows && (uint64_t)count * sample >= (uint64_t)ratio * top;
    return ProbeRows{lo, pays && top > lo ? top : lo};
}

// A kept call that is ONE launch (the answer kernel also extends the table) has no sample.  It reads `valid` = the rows all
// of which were written by launches before it, and the statistics the call before left: `top` = 1 + the largest k-mer of
// THAT call's batch that lay at or above the rows valid after it and below its capacity, `count` = how many such k-mers it
// held (exact, not sampled).  The rows [V, E) are built by this launch and read from the next call on; k-mers below V read
// their row, all others gather.  The extension pays when the batch before held at least ratio k-mers per new row
// (ratio 0: whenever top > V).  A top beyond the table (it never is) is not believed, as in table_rows.
// (count is a 32-bit sum that wraps for a batch of 2^32 k-mers or more at or above V: that moves this gate, never a mask.)
struct ProbeExtend { uint32_t valid, rows; };  // V, E
TXQ_HOST_DEVICE inline ProbeExtend extend_rows(uint32_t valid, uint32_t top, uint32_t count, uint32_t ratio, uint32_t cap_rows) {
    const uint32_t V = valid < cap_rows ? valid : cap_rows;
    const bool pays = top > V && top <= cap_rows && (uint64_t)count >= (uint64_t)ratio * (uint64_t)(top - V);
    return ProbeExtend{V, pays ? top : V};
}

// The words the kernels keep beside the table, in one allocation.
//   kStateAcc    two sample accumulators {top, count} of the domain pass, used alternately (call c adds into slot c & 1, the
//                answer of call c zeroes slot (c + 1) & 1 whether or not call c had a sample)
//   kStateValid  two copies of "rows [0, valid) hold the masks of the current bits": call c reads copy c & 1 and one thread of
//                its answer stores copy (c + 1) & 1.  One word would do for a call whose build is a launch of its own (every
//                wave computes the same rows from the old and from the new value); a one-launch call writes the rows [V, E)
//                in the launch that publishes E, and a wave that read E there would read rows not yet written.
//   kStateStat   three exact statistics {top, count}: the answer of call c adds into slot c % 3, reads slot (c + 2) % 3 (what
//                call c - 1 added) and zeroes slot (c + 1) % 3 for call c + 1.
// No word is read by the waves of a launch and written in the same launch.
enum : uint32_t { kStateAcc = 0, kStateValid = 4, kStateStat = 6, kStateWords = 12 };
struct ProbeSlots {
    uint32_t acc, acc_zero;                  // word offsets of this call's sample accumulator and the next call's
    uint32_t valid_read, valid_write;        // the copy of `valid` this call reads / stores
    uint32_t stat_add, stat_read, stat_zero;
};
// c: the call's number since the state words were last zeroed (ProbeKeep::calls before plan_probe_call counted it)
inline ProbeSlots probe_slots(uint64_t c) {
    const uint32_t p = (uint32_t)(c & 1), t = (uint32_t)(c % 3);
    return ProbeSlots{kStateAcc + 2u * p, kStateAcc + 2u * (p ^ 1u), kStateValid + p, kStateValid + (p ^ 1u),
                      kStateStat + 2u * t, kStateStat + 2u * ((t + 2u) % 3u), kStateStat + 2u * ((t + 1u) % 3u)};
}

// Is the table's content still valid?  Decided by API call order on the host: the index's generation counts the calls that
// changed its bits (txq_emplace_device), the table remembers the one it was built for.  Called under ProbeTable::mutex.
struct ProbeKeep {
    uint64_t generation = 0;  // of the index, when the table's rows were last started over
    uint64_t calls = 0;       // table calls since the state words were last zeroed
    bool valid = false;       // the state words are zeroed and `generation` means something
};
struct ProbeCall {
    bool fresh;       // the build starts at row 0 and `built` is not read
    bool zero_state;  // the state words must be zeroed before the sample (first call, or a call before this one failed)
    uint32_t parity;  // the sample accumulator of this call
};
// reallocated: the table's memory is new (first call, growth); keep: TXQ_PROBE_TABLE_KEEP (false: every call starts over)
inline ProbeCall plan_probe_call(ProbeKeep& k, uint64_t index_generation, bool reallocated, bool keep) {
    ProbeCall c;
    c.zero_state = !k.valid;
    if (c.zero_state) k.calls = 0;
    c.fresh = !k.valid || reallocated || !keep || k.generation != index_generation;
    c.parity = (uint32_t)(k.calls++ & 1);
    k.generation = index_generation;
    k.valid = true;
    return c;
}

}  // namespace txq
