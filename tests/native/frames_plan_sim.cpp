// Stand-alone check of csrc/txq_frames_plan.hpp: the pass of frames_kernel (txq_translate.hip) run on the CPU — the bytes of a
// batch cut into units and steps as the kernel cuts them, the step's bytes read through load_block, the six runs of a step
// staged at their address modulo 16 and stored through store_block — into a guarded buffer at every alignment 0 .. 15.
// Every store must lie inside the frames (and below the capacity), be aligned to its width, and no byte may be stored twice;
// afterwards every frame byte has been stored exactly once and equals translate_frame of host/encoder.cpp.
// Built with sanitizers by tests/test_frames_plan_sim.py:
//   g++ -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o sim
//       tests/native/frames_plan_sim.cpp tetrex_amd/csrc/host/encoder.cpp && ./sim
// Prints "frames_plan_sim ok: <runs> runs, <bytes> bytes" and exits 0, or names the first difference and exits 1.
#include "../../tetrex_amd/csrc/host/encoder.hpp"
#include "../../tetrex_amd/csrc/txq_frames_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace txq;
using namespace txq::tr;

namespace {

const char kTable1[65] = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
constexpr size_t kGuard = 64;

[[noreturn]] void die(const char* what, uint64_t a = 0, uint64_t b = 0, uint64_t c = 0) {
    std::printf("frames_plan_sim: %s (%llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c);
    std::exit(1);
}

// the output as the kernel's stores see it: [lo, hi) may be written, each byte once, a store of w bytes at a multiple of w
struct CheckedSink {
    uintptr_t lo, hi;
    std::vector<uint8_t>& times;
    void touch(uintptr_t at, size_t w) {
        if (at % w) die("a store that is not aligned to its width", at - lo, w);
        if (at < lo || at + w > hi) die("a store outside the frames", (uint64_t)(at - lo), w, hi - lo);
        for (size_t i = 0; i < w; ++i)
            if (times[at - lo + i]++) die("a byte stored twice", at - lo + i);
    }
    void store16(uintptr_t at, const uint8_t* src) { touch(at, 16); std::memcpy((void*)at, src, 16); }
    void store4(uintptr_t at, const uint8_t* src) { touch(at, 4); std::memcpy((void*)at, src, 4); }
    void store1(uintptr_t at, uint8_t byte) { touch(at, 1); *(uint8_t*)at = byte; }
};

struct Batch {
    std::vector<std::string> records;
    std::string seq;            // `front` bytes that belong to no record, then the records back to back
    std::vector<uint64_t> rec;  // n + 1
    std::vector<uint64_t> off;  // 6 n + 1
    std::string want;           // the frames back to back
};

Batch make_batch(const std::vector<std::string>& records, size_t front) {
    Batch b;
    b.records = records;
    b.seq.assign(front, 'G');
    b.rec.push_back(front);
    b.off.push_back(0);
    for (const std::string& s : records) {
        b.seq += s;
        b.rec.push_back(b.seq.size());
        for (unsigned f = 0; f < 6; ++f) {
            const std::string residues = tetrex::translate_frame(s, f);
            if (residues.size() != frame_len(s.size(), f % 3)) die("frame_len differs from translate_frame", s.size(), f);
            b.want += residues;
            b.off.push_back(b.want.size());
        }
    }
    return b;
}

// frames_kernel, unit by unit; returns the number of runs stored
uint64_t run_kernel(const Batch& b, uint8_t* frames, uint64_t cap, CheckedSink& sink) {
    const uint8_t* seq = (const uint8_t*)b.seq.data();
    const uint64_t* rec = b.rec.data();
    const uint64_t n = b.records.size(), base = rec[0], end = rec[n];
    if (end <= base) return 0;
    const uint64_t chunk = chunk_len(end - base);
    const uintptr_t seq_lo = (uintptr_t)(seq + base), seq_hi = (uintptr_t)(seq + end);
    const uintptr_t out_lo = (uintptr_t)frames, out_hi = out_lo + cap;
    uint64_t runs = 0;
    for (uint64_t unit = 0; unit < kUnits; ++unit) {
        const uint64_t ua = base + unit * chunk;
        if (ua >= end) break;
        const uint64_t ub = ua + chunk < end ? ua + chunk : end;
        for (uint64_t r = record_of(rec, 0, n, ua); r < n; ++r) {
            const uint64_t rs = rec[r];
            if (rs >= ub) break;
            const uint64_t re = rec[r + 1], L = re - rs;
            if (L < 3) continue;
            const Owned own = owned_starts(rs, re, ua, ub);
            if (own.lo >= own.hi) continue;
            uint64_t run_org[kRuns], run_a0[kRuns], run_a1[kRuns];
            for (uint32_t c = 0; c < kRuns; ++c) run_org[c] = out_lo + b.off[6 * r + run_frame(L, c)];
            for (uint64_t t0 = own.lo / 3 * 3; t0 < own.hi; t0 += kTile) {
                alignas(16) uint8_t raw[256];
                alignas(16) uint8_t stage[kRuns][kStageRow];
                std::memset(raw, 0xEE, sizeof raw);
                std::memset(stage, 0xEE, sizeof stage);
                const uintptr_t first = (uintptr_t)(seq + rs + t0);
                const uint32_t shift = (uint32_t)(first & 15u);
                const uint64_t left = L - t0;
                const uint32_t nbytes = left < kTile + 2 ? (uint32_t)left : kTile + 2;
                for (uint32_t lane = 0; lane < (shift + nbytes + 15u) / 16u; ++lane) {
                    const TextBlock blk = load_block(first - shift + 16u * lane, seq_lo, seq_hi, 'N');
                    std::memcpy(raw + 16u * lane, &blk.w, 16);
                }
                for (uint32_t c = 0; c < kRuns; ++c) {
                    const Run q = step_run(L, t0, own, c);
                    if (q.count > kTile / 3) die("a run of more than 64 letters", r, t0, c);
                    run_a0[c] = run_org[c] + q.first;
                    run_a1[c] = run_org[c] + q.first + q.count;
                    if (block_floor(run_a0[c]) + 16u * kRunBlocks < run_a1[c]) die("a run of more than kRunBlocks blocks", r, t0, c);
                    runs += q.count != 0;
                }
                for (uint32_t i = 0; i < kTile; ++i) {
                    const uint64_t p = t0 + i;
                    if (p < own.lo || p >= own.hi) continue;
                    const uint32_t j = i % 3;
                    if (fwd_frame(p) != j || rev_frame(L, p) != run_frame(L, 3 + j) || start_of(L, j, fwd_index(p)) != p ||
                        start_of(L, rev_frame(L, p), rev_index(L, p)) != p)
                        die("frame and index of a start position disagree", r, p);
                    uint8_t f, g;
                    codon_letters(kTable1, nucleotide(raw[shift + i]), nucleotide(raw[shift + i + 1]), nucleotide(raw[shift + i + 2]), &f, &g);
                    const uint64_t sf = run_org[j] + fwd_index(p) - block_floor(run_a0[j]);
                    const uint64_t sr = run_org[3 + j] + rev_index(L, p) - block_floor(run_a0[3 + j]);
                    if (sf >= kStageRow || sr >= kStageRow) die("a letter outside its run's staging row", r, p);
                    if (run_org[j] + fwd_index(p) < run_a0[j] || run_org[j] + fwd_index(p) >= run_a1[j] || run_org[3 + j] + rev_index(L, p) < run_a0[3 + j] ||
                        run_org[3 + j] + rev_index(L, p) >= run_a1[3 + j])
                        die("a letter outside its run", r, p);
                    stage[j][sf] = f;
                    stage[3 + j][sr] = g;
                }
                for (uint32_t lane = 0; lane < kRuns * kRunBlocks; ++lane) {
                    const uint32_t c = lane / kRunBlocks, blk_i = lane % kRunBlocks;
                    const uintptr_t a0 = run_a0[c], a1 = run_a1[c] < out_hi ? run_a1[c] : out_hi;
                    const uintptr_t blk = block_floor(a0) + 16u * blk_i;
                    const uint32_t mask = block_mask(a0, a1, blk);
                    if (mask) store_block(mask, blk, &stage[c][16u * blk_i], sink);
                }
            }
        }
    }
    return runs;
}

std::string random_nt(std::mt19937_64& rng, size_t L, double ambiguous, bool lower) {
    static const char acgt[] = "ACGTU", junk[] = "NRYKM-* nx";
    std::string s(L, 'A');
    for (char& c : s) {
        c = acgt[rng() % 5];
        if ((double)(rng() % 10000) < ambiguous * 10000) c = junk[rng() % (sizeof junk - 1)];
        if (lower || rng() % 16 == 0) c = (char)std::tolower((unsigned char)c);
    }
    return s;
}

}  // namespace

int main() {
    std::mt19937_64 rng(20240611);
    std::vector<std::string> records;
    for (size_t L = 0; L <= 40; ++L) records.push_back(random_nt(rng, L, 0.05, L % 5 == 0));
    records.push_back("");
    const size_t unit = (size_t)kMinChunk;
    for (size_t L : {unit - 3, unit - 2, unit - 1, unit, unit + 1, unit + 2, unit + 3, 2 * unit - 2, 2 * unit - 1, 2 * unit, 2 * unit + 1, 2 * unit + 2,
                     (size_t)kTile - 1, (size_t)kTile, (size_t)kTile + 1, (size_t)kTile + 2, (size_t)kTile + 3}) {
        records.push_back(random_nt(rng, L, 0.01, false));
        if (L % 2) records.push_back("");
    }
    records.push_back("");
    records.push_back("");
    records.push_back(random_nt(rng, 20011, 0.002, false));
    records.push_back("");
    records.push_back("ac");
    records.push_back(std::string(100, 'N'));
    records.push_back("TAATAGTGA");
    records.push_back(random_nt(rng, 301, 0.3, true));
    records.push_back("");
    uint64_t runs = 0, bytes = 0;
    for (size_t front : {(size_t)0, (size_t)5}) {
        const Batch b = make_batch(records, front);
        const uint64_t bound = b.want.size();
        {
            uint64_t sum = 0;
            for (const std::string& s : records)
                for (uint32_t o = 0; o < 3; ++o) sum += 2 * frame_len(s.size(), o);
            if (sum != bound) die("the bound is not the sum of the frames", sum, bound);
        }
        for (size_t align = 0; align < 16; ++align) {
            for (const uint64_t cap : {bound, bound / 2 + align, (uint64_t)0}) {
                const size_t total = kGuard + 16 + bound + kGuard;
                uint8_t* mem = (uint8_t*)std::aligned_alloc(16, (total + 15) / 16 * 16);
                std::memset(mem, 0xA5, total);
                uint8_t* frames = mem + kGuard + align;
                std::vector<uint8_t> times(cap, 0);
                CheckedSink sink{(uintptr_t)frames, (uintptr_t)frames + cap, times};
                runs += run_kernel(b, frames, cap, sink);
                for (uint64_t i = 0; i < cap; ++i) {
                    if (times[i] != 1) die("a frame byte that was not stored", i, align, cap);
                    if (frames[i] != (uint8_t)b.want[i]) die("a frame byte differs from translate_frame", i, align, cap);
                }
                for (size_t i = 0; i < total; ++i)
                    if ((mem + i < frames || mem + i >= frames + cap) && mem[i] != 0xA5) die("a byte outside the frames was written", i, align, cap);
                bytes += cap;
                std::free(mem);
            }
        }
    }
    std::printf("frames_plan_sim ok: %llu runs, %llu bytes\n", (unsigned long long)runs, (unsigned long long)bytes);
    return 0;
}
