// Stand-alone check of csrc/txq_frame_windows_plan.hpp: the window pass of translate_windows_kernel (txq_translate.hip) run on
// the CPU — the bytes of a batch cut into units and steps of kTile start positions as the kernel cuts them, a count pass that
// leaves each unit's tails, a fill pass in which the lane of start position p holds the rank of its k-mer position in its
// forward and in its reverse frame (the values before this step, carried over units by the tails, plus the valid lanes
// below) and stores it into the window slots codon_slots names, and window_finish_kernel's pass over the windows.
// Every slot must be written exactly once (the end slot of a frame's last window by the finishing pass alone), no write may
// leave the frame's slots, and every window's (begin, len) must equal a brute-force count over the frame's residues
// (translate_frame of host/encoder.cpp) with the windows cut by a restatement of `tetrex search --window`.
// Built with sanitizers by tests/test_frame_windows_sim.py:
//   g++ -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o sim
//       tests/native/frame_windows_sim.cpp tetrex_amd/csrc/host/encoder.cpp && ./sim
// Prints "frame_windows_sim ok: <batches> batches, <windows> windows, <empty> empty" and exits 0, or names the first
// difference and exits 1.
#include "../../tetrex_amd/csrc/host/encoder.hpp"
#include "../../tetrex_amd/csrc/txq_frame_windows_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <utility>
#include <vector>

using namespace txq;
using namespace txq::tr;

namespace {

[[noreturn]] void die(const char* what, uint64_t a = 0, uint64_t b = 0, uint64_t c = 0, uint64_t d = 0) {
    std::printf("frame_windows_sim: %s (%llu, %llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c,
                (unsigned long long)d);
    std::exit(1);
}

// `tetrex search --window` on R letters, restated: (begin, len)
std::vector<std::pair<uint64_t, uint64_t>> windows_of(uint64_t R, uint32_t k, uint32_t W, uint32_t S) {
    std::vector<std::pair<uint64_t, uint64_t>> out;
    if (R < k) return out;
    if (R <= W) {
        out.push_back({0, R});
        return out;
    }
    uint64_t at = 0;
    for (; at + W <= R; at += S) out.push_back({at, W});
    if (out.back().first + W < R) out.push_back({R - W, W});
    return out;
}

struct Batch {
    std::vector<std::string> records;
    std::vector<uint64_t> rec;                // n + 1
    std::vector<std::vector<uint8_t>> valid;  // frame q: k-mer position c is stop-free
    std::vector<uint64_t> off, woff;          // 6 n + 1: values, windows
};

Batch make_batch(const std::vector<std::string>& records, size_t front, uint32_t k, uint32_t W, uint32_t S) {
    Batch b;
    b.records = records;
    b.rec.push_back(front);
    b.off.push_back(0);
    b.woff.push_back(0);
    for (const std::string& s : records) {
        b.rec.push_back(b.rec.back() + s.size());
        for (unsigned f = 0; f < 6; ++f) {
            const std::string residues = tetrex::translate_frame(s, f);
            if (residues.size() != frame_len(s.size(), f % 3)) die("frame_len differs from translate_frame", s.size(), f);
            std::vector<uint8_t> v;
            uint64_t n = 0;
            for (size_t c = 0; c + k <= residues.size(); ++c) {
                v.push_back(residues.find('*', c) >= c + k);
                n += v.back();
            }
            b.valid.push_back(std::move(v));
            b.off.push_back(b.off.back() + n);
            b.woff.push_back(b.woff.back() + fw::window_count(residues.size(), k, W, S));
        }
    }
    return b;
}

// translate_kernel<false>, translate_windows_kernel and window_finish_kernel; returns (windows, empty windows)
std::pair<uint64_t, uint64_t> run_kernels(const Batch& b, uint32_t k, uint32_t W, uint32_t S) {
    const uint64_t* rec = b.rec.data();
    const uint64_t n = b.records.size(), base = rec[0], end = rec[n], total = b.woff.back(), span = 3ull * k;
    std::vector<uint64_t> begin(total, 0xAAAAAAAAAAAAAAAAull);
    std::vector<uint32_t> len(total, 0xAAAAAAAAu);
    std::vector<uint8_t> begin_times(total, 0), end_times(total, 0);
    if (end > base) {
        const uint64_t chunk = chunk_len(end - base);
        std::vector<uint32_t> tails((size_t)kUnits * 6, 0);
        for (int pass = 0; pass < 2; ++pass) {
            for (uint64_t unit = 0; unit < kUnits; ++unit) {
                const uint64_t ua = base + unit * chunk;
                if (ua >= end) break;
                const uint64_t ub = ua + chunk < end ? ua + chunk : end;
                uint32_t cnt[6] = {0, 0, 0, 0, 0, 0};
                bool runs_on = false;
                for (uint64_t r = record_of(rec, 0, n, ua); r < n; ++r) {
                    const uint64_t rs = rec[r];
                    if (rs >= ub) break;
                    const uint64_t re = rec[r + 1], L = re - rs;
                    for (uint32_t& c : cnt) c = 0;
                    runs_on = re > ub;
                    if (L < span) continue;
                    const uint64_t lo = (ua > rs ? ua : rs) - rs, fit = L - span + 1, cut = (ub < re ? ub : re) - rs, hi = cut < fit ? cut : fit;
                    if (lo >= hi) continue;
                    uint32_t rframe[3];
                    uint64_t run[6] = {0, 0, 0, 0, 0, 0}, wbase[6], rcount[3];
                    fw::Frame wplan[6];
                    for (uint32_t j = 0; j < 3; ++j) {
                        rframe[j] = 3u + (uint32_t)((L - span + 3u - j) % 3u);
                        wplan[j] = fw::frame_plan(frame_len(L, j), k, W, S);
                        wplan[3 + j] = fw::frame_plan(frame_len(L, rframe[j] - 3u), k, W, S);
                        wbase[j] = b.woff[6 * r + j];
                        wbase[3 + j] = b.woff[6 * r + rframe[j]];
                        rcount[j] = b.off[6 * r + rframe[j] + 1] - b.off[6 * r + rframe[j]];
                    }
                    if (pass == 1 && lo > 0)
                        for (uint64_t u = (rs - base) / chunk; u < unit; ++u)
                            for (int c = 0; c < 6; ++c) run[c] += tails[u * 6 + c];
                    for (uint64_t t0 = lo / 3 * 3; t0 < hi; t0 += kTile) {
                        for (uint32_t j = 0; j < 3; ++j) {
                            uint64_t bf = 0, br = 0;
                            bool okf[64], okr[64], mine[64];
                            for (uint32_t lane = 0; lane < 64; ++lane) {
                                const uint64_t p = t0 + 3u * lane + j;
                                mine[lane] = p >= lo && p < hi;
                                okf[lane] = okr[lane] = false;
                                if (!mine[lane]) continue;
                                const uint64_t cr = fw::rev_kmer_index(L, p, k);
                                if (fw::rev_kmer_frame(L, p, k) != rframe[j]) die("the reverse frame of a start position disagrees", r, p);
                                if (p / 3 >= wplan[j].M || cr >= wplan[3 + j].M) die("a k-mer position outside its frame", r, p);
                                okf[lane] = b.valid[6 * r + j][p / 3];
                                okr[lane] = b.valid[6 * r + rframe[j]][cr];
                                bf |= (uint64_t)okf[lane] << lane;
                                br |= (uint64_t)okr[lane] << lane;
                            }
                            if (pass == 1)
                                for (uint32_t lane = 0; lane < 64; ++lane) {
                                    if (!mine[lane]) continue;
                                    const uint64_t p = t0 + 3u * lane + j, below = (1ull << lane) - 1;
                                    const auto put = [&](uint32_t c, const fw::Slots s, uint64_t v) {
                                        const uint64_t q = 6 * r + (c < 3 ? c : rframe[c - 3]);
                                        if (s.begin != fw::kNone) {
                                            if (s.begin >= b.woff[q + 1] - b.woff[q]) die("a begin slot outside the frame's windows", r, p, c, s.begin);
                                            if (begin_times[wbase[c] + s.begin]++) die("a begin slot written twice", r, p, c, s.begin);
                                            begin[wbase[c] + s.begin] = v;
                                        }
                                        if (s.end != fw::kNone) {
                                            if (s.end + 1 >= b.woff[q + 1] - b.woff[q]) die("an end slot outside the frame's windows, or its last", r, p, c, s.end);
                                            if (end_times[wbase[c] + s.end]++) die("an end slot written twice", r, p, c, s.end);
                                            len[wbase[c] + s.end] = (uint32_t)v;
                                        }
                                    };
                                    put(j, fw::codon_slots(wplan[j], p / 3), run[j] + (uint64_t)__builtin_popcountll(bf & below));
                                    put(3 + j, fw::codon_slots(wplan[3 + j], fw::rev_kmer_index(L, p, k)),
                                        rcount[j] - (run[3 + j] + (uint64_t)__builtin_popcountll(br & below) + (okr[lane] ? 1u : 0u)));
                                }
                            run[j] += (uint64_t)__builtin_popcountll(bf);
                            run[3 + j] += (uint64_t)__builtin_popcountll(br);
                            cnt[j] += (uint32_t)__builtin_popcountll(bf);
                            cnt[3 + j] += (uint32_t)__builtin_popcountll(br);
                        }
                    }
                }
                if (pass == 0)
                    for (int c = 0; c < 6; ++c) tails[unit * 6 + c] = runs_on ? cnt[c] : 0u;
            }
        }
    }
    // window_finish_kernel
    const uint64_t m = 6 * n;
    for (uint64_t j = 0; j < total; ++j) {
        uint64_t lo = 0, hi = m;
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (b.woff[mid] <= j) lo = mid;
            else hi = mid;
        }
        const bool last = j + 1 == b.woff[lo + 1];
        if (begin_times[j] != 1) die("a begin slot that was not written", j, lo);
        if (end_times[j] != (last ? 0 : 1)) die("an end slot that was not written, or the last window's that was", j, lo);
        const uint64_t bg = begin[j];
        const uint32_t e = last ? (uint32_t)(b.off[lo + 1] - b.off[lo]) : len[j];
        begin[j] = b.off[lo] + bg;
        len[j] = e - (uint32_t)bg;
    }
    // against the brute-force count
    uint64_t empty = 0;
    for (uint64_t q = 0; q < m; ++q) {
        const uint64_t L = b.records[q / 6].size(), R = frame_len(L, (uint32_t)(q % 3));
        const auto wins = windows_of(R, k, W, S);
        const fw::Frame f = fw::frame_plan(R, k, W, S);
        if (wins.size() != b.woff[q + 1] - b.woff[q]) die("the window count differs from windows_of", q, R, wins.size(), f.count);
        for (size_t j = 0; j < wins.size(); ++j) {
            const fw::Window w = fw::window_at(f, j);
            if (w.a != wins[j].first || w.len != wins[j].second) die("window_at differs from windows_of", q, j, w.a, w.len);
            uint64_t v0 = 0, v1 = 0;
            for (uint64_t c = 0; c < w.a + w.len - k + 1; ++c) {
                v0 += c < w.a && b.valid[q][c];
                v1 += b.valid[q][c];
            }
            const uint64_t at = b.woff[q] + j;
            if (begin[at] != b.off[q] + v0 || len[at] != v1 - v0) die("a window differs from the brute-force count", q, j, begin[at], len[at]);
            if (at && (begin[at] < begin[at - 1] || begin[at] + len[at] < begin[at - 1] + len[at - 1])) die("the windows do not slide", q, j);
            empty += v1 == v0;
            // the nucleotides of the window's residues: inside the record, 3 per residue, codon-aligned to the frame
            const fw::Span sp = fw::residues_on_record(L, (uint32_t)(q % 6), w.a, w.a + w.len);
            if (sp.begin < 1 || sp.end > L || sp.end - sp.begin + 1 != 3 * w.len) die("a window's nucleotides leave the record", q, j, sp.begin, sp.end);
            const uint64_t o = q % 3, lead = q % 6 < 3 ? sp.begin - 1 : L - sp.end;
            if (lead < o || (lead - o) % 3 || (lead - o) / 3 != w.a) die("a window's nucleotides are not its residues' codons", q, j, sp.begin, sp.end);
        }
    }
    return {total, empty};
}

std::string random_nt(std::mt19937_64& rng, size_t L, double ambiguous) {
    static const char acgt[] = "ACGTU", junk[] = "NRYKM-* nx";
    std::string s(L, 'A');
    for (char& c : s) {
        c = acgt[rng() % 5];
        if ((double)(rng() % 10000) < ambiguous * 10000) c = junk[rng() % (sizeof junk - 1)];
        if (rng() % 16 == 0) c = (char)std::tolower((unsigned char)c);
    }
    return s;
}

// a record whose frame +(o + 1) has R residues without a stop but at the codons in `stops`; the other frames are as they fall
std::string planted(std::mt19937_64& rng, uint64_t R, uint32_t o, const std::vector<uint64_t>& stops) {
    static const char* const sense[] = {"GCT", "AAA", "GGC", "CTG", "TTC", "ACC", "CAG", "GAT"};
    std::string s = random_nt(rng, o, 0);
    for (uint64_t c = 0; c < R; ++c) s += sense[rng() % 8];
    for (const uint64_t c : stops)
        if (c < R) s.replace(o + 3 * c, 3, c % 2 ? "TAG" : "TAA");
    return s;
}

}  // namespace

int main() {
    std::mt19937_64 rng(20241020);
    uint64_t batches = 0, windows = 0, empty = 0;
    for (const uint32_t k : {1u, 6u, 12u}) {
        const std::vector<std::pair<uint32_t, uint32_t>> shapes = {{k, 1},          {k + 1, k + 1}, {2 * k + 3, 1},     {2 * k + 3, k + 1}, {2 * k + 3, 2 * k + 3},
                                                                   {40, 7},         {40, 10},       {40, 20},           {40, 40},           {25, 9}};
        for (const auto& [W, S] : shapes) {
            if (W < k || S > W) continue;
            std::vector<std::string> records;
            // the R shapes, for each of the three offsets: random letters, then the same with a stop-free planted frame
            for (const uint64_t R : {(uint64_t)k - 1, (uint64_t)k, (uint64_t)W - 1, (uint64_t)W, (uint64_t)W + 1, (uint64_t)W + S - 1, (uint64_t)W + S,
                                     (uint64_t)W + S + 1, (uint64_t)W + 3 * S + 2})
                for (uint32_t o = 0; o < 3; ++o) {
                    records.push_back(random_nt(rng, 3 * R + o, 0.02));
                    records.push_back(planted(rng, R, o, {}));
                    // stops at the first and the last codon, and on the boundaries of the windows
                    records.push_back(planted(rng, R, o, {0, R - 1}));
                    records.push_back(planted(rng, R, o, {S, S - 1, (uint64_t)W - k, (uint64_t)W - k + 1, (uint64_t)W, (uint64_t)W - 1, R - W, R - k}));
                    records.push_back("");
                }
            // a stop in every k-mer of the second window (len 0), and of every window
            {
                std::vector<uint64_t> some, all;
                for (uint64_t c = S + k - 1; c < (uint64_t)S + W; c += k) some.push_back(c);
                for (uint64_t c = k - 1; c < 4ull * W; c += k) all.push_back(c);
                if (k > 1) {
                    records.push_back(planted(rng, 3ull * W, 1, some));
                    records.push_back(planted(rng, 3ull * W + 1, 2, all));
                } else {  // (k = 1: a k-mer is a residue, so the stops are the residues themselves)
                    for (uint64_t c = S; c < (uint64_t)S + W; ++c) some.push_back(c);
                    records.push_back(planted(rng, 3ull * W, 1, some));
                }
            }
            // a record across three units (at the minimum chunk), stop-free across each unit boundary in frame +2
            records.push_back(planted(rng, (3 * kMinChunk + 100) / 3, 1, {5, 400, 401}));
            records.push_back(random_nt(rng, 3 * kMinChunk + 100, 0.01));
            // many short records inside one unit
            for (int i = 0; i < 300; ++i) records.push_back(random_nt(rng, 30 + rng() % 31, 0.03));
            records.push_back("");
            for (const size_t front : {(size_t)0, (size_t)5}) {
                const Batch b = make_batch(records, front, k, W, S);
                const auto [n, e] = run_kernels(b, k, W, S);
                ++batches;
                windows += n;
                empty += e;
            }
        }
    }
    std::printf("frame_windows_sim ok: %llu batches, %llu windows, %llu empty\n", (unsigned long long)batches, (unsigned long long)windows,
                (unsigned long long)empty);
    return 0;
}
