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
//   kStateOutside  two flags "a k-mer of the batch lies at or above `valid`" of the sorted answer (plan_probe_sort below): the
//                count kernel of call c sets flag c & 1, its answer reads it and zeroes flag (c + 1) & 1 (every answer does)
//   kStateSorted   how many answers ran in sorted mode since the state was zeroed (one thread adds; tests read it)
enum : uint32_t { kStateAcc = 0, kStateValid = 4, kStateStat = 6, kStateOutside = 12, kStateSorted = 14, kStateWords = 16 };
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

// The sorted answer of a large kept call: the batch is partitioned into value buckets v >> shift in front of the answer
// (count, scan, scatter: records (v << 32 | position) in bucket order), and a workgroup on XCD x answers the x-th eighth of
// the records, so that the table rows an XCD reads at any one time are about one bucket's, which its L2 holds.
//   shift          a bucket's rows take about bucket_kb KiB (a power of two of rows, at least one), and at most
//                  kSortMaxBuckets buckets cover the table's cap_rows rows
//   chunks         workgroups of count and scatter: kSortChunk k-mers each
//   tiles_per_xcd  workgroup b of the answer (four waves, workgroups are dealt round-robin over the 8 XCDs) takes the tiles
//                  sort_tile(b, wave): XCD x walks the tiles [x * tiles_per_xcd, (x + 1) * tiles_per_xcd)
//   blocks         workgroups b the answer has to walk (a multiple of 8; its grid is one too, so b % 8 stays with a workgroup)
static constexpr uint32_t kSortChunk = 4096, kSortMaxBuckets = 256, kSortXcds = 8;
// TXQ_PROBE_SORT_MIN unset: the smallest batch that gained at both domains measured, 2^18 and 2^20 values (2^22 k-mers gained 16 us
// at the one and lost 14 us at the other, 2^20 lost 3 us: profiles/probe_sorted_ab.txt)
static constexpr long long kSortMinDefault = 1 << 23;
static constexpr long long kSortBucketKbDefault = 1024;
struct ProbeSort {
    bool on = false;
    uint32_t shift = 0, buckets = 0, chunks = 0;
    uint64_t n_tiles = 0, tiles_per_xcd = 0, blocks = 0;
};
inline uint64_t sort_tile(const ProbeSort& p, uint64_t block, uint32_t wave) {
    return (block % kSortXcds) * p.tiles_per_xcd + (block / kSortXcds) * 4u + wave;
}
// kept_fused: the call is one launch on kept rows; lpk: lanes per k-mer of the kernel instance (pow2 >= stride / 2);
// sort: TXQ_PROBE_SORT (0 never); sort_min: TXQ_PROBE_SORT_MIN; bucket_kb: TXQ_PROBE_SORT_BUCKET_KB.
// The scratch (8 bytes of records per k-mer of the largest batch, kept with the index) is bounded twice: rows of 16 or 32
// words only (LPK 8 and 16, the widths that were measured: at most 1/16 of the caller's masks), and at most scratch_mb MiB
// (TXQ_KMER_TABLE_MB, the budget of the table itself).
inline ProbeSort plan_probe_sort(bool kept_fused, bool has_alive, bool has_root, uint32_t lpk, uint32_t stride, uint32_t shard_words, uint64_t n,
                                 size_t cap_rows, bool sort, long long sort_min, long long bucket_kb, long long scratch_mb) {
    ProbeSort p;
    const bool whole = stride / 2 == lpk && !(stride & 1) && !(shard_words & 1) && shard_words == stride;
    if (!sort || !kept_fused || has_alive || has_root || lpk < 8 || lpk > 16 || !whole || n == 0 || (n >> 32) || cap_rows == 0 || (cap_rows >> 32) ||
        sort_min < 1 || n < (uint64_t)sort_min || scratch_mb < 0 || n * 8 > ((uint64_t)scratch_mb << 20))
        return p;
    const uint64_t row_bytes = (uint64_t)stride * 8;
    const uint64_t bucket_rows = std::max<uint64_t>(((uint64_t)std::max(bucket_kb, 1LL) << 10) / row_bytes, 1);
    while ((2ull << p.shift) <= bucket_rows) ++p.shift;
    while ((((uint64_t)cap_rows - 1) >> p.shift) + 1 > kSortMaxBuckets) ++p.shift;
    p.buckets = (uint32_t)((((uint64_t)cap_rows - 1) >> p.shift) + 1);
    p.chunks = (uint32_t)((n + kSortChunk - 1) / kSortChunk);
    p.n_tiles = (n + 63) >> 6;
    p.tiles_per_xcd = ((p.n_tiles + kSortXcds - 1) / kSortXcds + 3) & ~(uint64_t)3;
    p.blocks = kSortXcds * (p.tiles_per_xcd / 4);
    p.on = true;
    return p;
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
