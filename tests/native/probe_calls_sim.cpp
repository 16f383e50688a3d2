// Sequences of flat-probe calls on one domain table without a GPU, played with the functions of
// tetrex_amd/csrc/txq_probe_plan.hpp themselves (plan_probe_call, probe_slots, table_rows, extend_rows) in the order
// txq_probe.hip probe_flat and its kernels use them.  The table is modelled as "row v written since the last fresh call:
// yes / no", the state words as an array; tests/test_probe_calls.py holds the cases.  Commands on stdin, one per line:
//   ext    valid top count ratio cap_rows     -> "V E" of extend_rows
//   slots  c                                  -> "acc acc_zero valid_read valid_write stat_add stat_read stat_zero" of probe_slots
//   sim    seed sequences calls               -> "ok <sequences>" after that many random sequences, or the first violation (exit 1)
//   steady seed sequences                     -> "ok <sequences>": a steady batch after a random prefix reaches V >= its domain within
//                                                three calls, and no later call builds or counts anything
//
// A batch is (domain, n, cap): k-mer i has the value i % domain, the domain pass sees the first ceil(n / 16) k-mers.
#include "../../tetrex_amd/csrc/txq_probe_plan.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

using namespace txq;

static uint64_t g_rng;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (g_rng += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
static uint64_t below(uint64_t n) { return rnd() % n; }

struct Batch { uint64_t domain, n, cap; };
// how many of the first `m` k-mers have a value below x
static uint64_t count_below(const Batch& b, uint64_t m, uint64_t x) {
    x = std::min(x, b.domain);
    return m / b.domain * x + std::min(m % b.domain, x);
}
// {top, count} of the first m k-mers over the values in [lo, hi)
static void stats_of(const Batch& b, uint64_t m, uint64_t lo, uint64_t hi, uint32_t& top, uint32_t& count) {
    const uint64_t present = std::min(b.domain, m);  // the values 0 .. present - 1 occur
    const uint64_t end = std::min(present, hi);
    top = end > lo ? (uint32_t)end : 0u;
    count = hi > lo ? (uint32_t)(count_below(b, m, hi) - count_below(b, m, lo)) : 0u;
}

struct Table {
    std::vector<uint32_t> state = std::vector<uint32_t>(kStateWords, 0xdeadbeefu);  // (device memory: anything until it is zeroed)
    std::vector<char> written;  // row v written since the last fresh call
    size_t cap_rows = 0;
    ProbeKeep keep;
    uint64_t generation = 0;
};
struct Outcome { bool fresh, sampled; uint32_t valid, rows, built, counted; };

#define CHECK(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); return false; } } while (0)

// one call as probe_flat and its launches make it; what = for messages
static bool play(Table& t, const Batch& b, bool keep_knob, bool fused_knob, bool fail, uint32_t ratio, Outcome& out, const char* what) {
    bool reallocated = false;
    if (t.cap_rows < b.cap) {  // growth: new memory
        t.cap_rows = b.cap;
        t.written.assign(t.cap_rows, 0);
        reallocated = true;
    }
    const ProbeCall call = plan_probe_call(t.keep, t.generation, reallocated, keep_knob);
    t.keep.valid = false;
    if (call.zero_state) std::fill(t.state.begin(), t.state.end(), 0u);
    const ProbeSlots s = probe_slots(t.keep.calls - 1);
    const bool sampled = call.fresh || !fused_knob;
    if (fail) {  // the launches failed somewhere: the state words and the rows may be anything
        for (auto& w : t.state) w = (uint32_t)rnd();
        std::fill(t.written.begin(), t.written.end(), 0);
        return true;
    }
    CHECK(call.parity == (s.acc - kStateAcc) / 2, "%s: the sample slot is not the call's parity", what);
    // the slots
    const std::set<uint32_t> stat{s.stat_add, s.stat_read, s.stat_zero};
    CHECK(stat.size() == 3, "%s: statistics slots add %u read %u zero %u are not three", what, s.stat_add, s.stat_read, s.stat_zero);
    CHECK(s.valid_read != s.valid_write, "%s: the word read as V is the word written", what);
    CHECK(s.acc != s.acc_zero, "%s: sample slots", what);
    std::set<uint32_t> reads{s.valid_read}, writes{s.valid_write, s.stat_add, s.stat_add + 1, s.stat_zero, s.stat_zero + 1, s.acc_zero, s.acc_zero + 1};
    if (sampled) { reads.insert(s.acc); reads.insert(s.acc + 1); }  // (written by the domain pass, a launch of its own, before they are read)
    else { reads.insert(s.stat_read); reads.insert(s.stat_read + 1); }
    for (uint32_t w : reads) CHECK(!writes.count(w) && w < kStateWords, "%s: state word %u is read and written by one launch", what, w);
    for (uint32_t w : writes) CHECK(w < kStateWords, "%s: state word %u out of range", what, w);
    CHECK(t.state[s.stat_add] == 0 && t.state[s.stat_add + 1] == 0, "%s: the statistics slot the call adds into is not zero", what);

    if (call.fresh) std::fill(t.written.begin(), t.written.end(), 0);  // the rows start over
    ProbeExtend ex;
    if (sampled) {
        CHECK(t.state[s.acc] == 0 && t.state[s.acc + 1] == 0, "%s: the sample slot the call adds into is not zero", what);
        stats_of(b, (b.n + kDomainSample - 1) / kDomainSample, 0, b.cap, t.state[s.acc], t.state[s.acc + 1]);  // probe_domain_kernel
        const ProbeRows tr = table_rows(call.fresh, t.state[s.valid_read], t.state[s.acc], t.state[s.acc + 1], ratio, kDomainSample, (uint32_t)t.cap_rows);
        CHECK(tr.rows <= t.cap_rows && tr.lo <= tr.rows, "%s: build [%u, %u) beyond the table of %zu", what, tr.lo, tr.rows, t.cap_rows);
        for (uint32_t v = tr.lo; v < tr.rows; ++v) t.written[v] = 1;  // the build, a launch before the answer
        out.built = tr.rows - tr.lo;
        ex = ProbeExtend{tr.rows, tr.rows};
    } else {
        ex = extend_rows(t.state[s.valid_read], t.state[s.stat_read], t.state[s.stat_read + 1], ratio, (uint32_t)t.cap_rows);
        CHECK(ex.rows <= t.cap_rows && ex.valid <= ex.rows, "%s: extension [%u, %u) beyond the table of %zu", what, ex.valid, ex.rows, t.cap_rows);
        out.built = ex.rows - ex.valid;
    }
    // the answer: reads the rows below V, counts [E, cap), builds [V, E), leaves the next call's words behind
    for (uint32_t v = 0; v < ex.valid; ++v)
        CHECK(t.written[v], "%s: row %u of V = %u is read, but no earlier call wrote it since the last fresh one", what, v, ex.valid);
    uint32_t top = 0, count = 0;
    stats_of(b, b.n, ex.rows, b.cap, top, count);
    t.state[s.stat_add] = std::max(t.state[s.stat_add], top);
    t.state[s.stat_add + 1] += count;
    for (uint32_t v = ex.valid; v < ex.rows; ++v) t.written[v] = 1;
    t.state[s.valid_write] = ex.rows;
    t.state[s.stat_zero] = t.state[s.stat_zero + 1] = 0;
    t.state[s.acc_zero] = t.state[s.acc_zero + 1] = 0;
    t.keep.valid = true;
    out.fresh = call.fresh; out.sampled = sampled; out.valid = ex.valid; out.rows = ex.rows; out.counted = count;
    return true;
}

static Batch random_batch() {
    Batch b;
    b.cap = 64 * (1 + below(48));                                        // 64 .. 3072 rows
    b.domain = below(4) ? 1 + below(b.cap) : 1 + below(4 * b.cap);       // mostly inside the capacity, sometimes far beyond
    b.n = below(3) ? b.domain * (1 + below(8)) + below(64) : 1 + below(8 * b.cap);
    return b;
}

// one random call on t: fresh / kept by whatever happened before it
static bool random_call(Table& t, uint32_t ratio, const char* what) {
    const uint64_t kind = below(16);
    if (kind == 0) {  // txq_emplace_device: the rows are those of other bits now
        ++t.generation;
        std::fill(t.written.begin(), t.written.end(), 0);
    }
    Batch b = random_batch();
    if (kind == 1) b.cap = t.cap_rows + 64 * (1 + below(8));  // growth
    Outcome o{};
    return play(t, b, below(8) != 0, below(3) != 0, kind == 2, ratio, o, what);
}

static bool sim(uint64_t seed, int sequences, int calls) {
    g_rng = seed;
    char what[64];
    for (int q = 0; q < sequences; ++q) {
        Table t;
        const uint32_t ratio = below(3) ? kTableRatio : 0u;
        for (int c = 0; c < calls; ++c) {
            snprintf(what, sizeof what, "sequence %d call %d", q, c);
            if (!random_call(t, ratio, what)) return false;
        }
    }
    return true;
}

static bool steady(uint64_t seed, int sequences) {
    g_rng = seed;
    char what[64];
    for (int q = 0; q < sequences; ++q) {
        Table t;
        const uint32_t ratio = below(3) ? kTableRatio : 0u;
        const int prefix = (int)below(6);
        for (int c = 0; c < prefix; ++c) {
            snprintf(what, sizeof what, "steady %d prefix %d", q, c);
            if (!random_call(t, ratio, what)) return false;
        }
        Batch b;
        b.cap = std::max<uint64_t>(64 * (1 + below(48)), below(2) ? t.cap_rows : 0);
        b.domain = 1 + below(b.cap);
        b.n = b.domain * (kTableRatio + below(8)) + below(b.domain);  // every value at least `ratio` times: the domain pays
        for (int c = 0; c < 8; ++c) {
            snprintf(what, sizeof what, "steady %d call %d", q, c);
            Outcome o{};
            if (!play(t, b, true, true, false, ratio, o, what)) return false;
            if (c >= 2) CHECK(o.valid >= b.domain, "%s: V = %u below the domain %" PRIu64, what, o.valid, b.domain);
            if (c >= 3) CHECK(!o.fresh && !o.sampled && o.built == 0 && o.counted == 0, "%s: builds %u rows, counts %u k-mers", what, o.built, o.counted);
        }
    }
    return true;
}

int main() {
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        unsigned long long a[5] = {0, 0, 0, 0, 0};
        const int want = !strcmp(cmd, "ext") ? 5 : !strcmp(cmd, "slots") ? 1 : !strcmp(cmd, "sim") ? 3 : !strcmp(cmd, "steady") ? 2 : -1;
        if (want < 0) { fprintf(stderr, "probe_calls_sim: unknown command %s\n", cmd); return 2; }
        for (int i = 0; i < want; ++i)
            if (scanf("%llu", &a[i]) != 1) { fprintf(stderr, "probe_calls_sim: short input\n"); return 2; }
        if (!strcmp(cmd, "ext")) {
            const ProbeExtend e = extend_rows((uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2], (uint32_t)a[3], (uint32_t)a[4]);
            printf("%" PRIu32 " %" PRIu32 "\n", e.valid, e.rows);
        } else if (!strcmp(cmd, "slots")) {
            const ProbeSlots s = probe_slots(a[0]);
            printf("%u %u %u %u %u %u %u\n", s.acc, s.acc_zero, s.valid_read, s.valid_write, s.stat_add, s.stat_read, s.stat_zero);
        } else if (!strcmp(cmd, "sim")) {
            if (!sim(a[0], (int)a[1], (int)a[2])) return 1;
            printf("ok %llu\n", a[1]);
        } else {
            if (!steady(a[0], (int)a[1])) return 1;
            printf("ok %llu\n", a[1]);
        }
    }
    return 0;
}
