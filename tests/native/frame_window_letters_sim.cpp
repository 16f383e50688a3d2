// Stand-alone check of the letters part of csrc/txq_frame_windows_plan.hpp: what frame_window_letters_kernel
// (txq_frame_letters.hip) does for a window, run on the CPU — the frame found by binary search in the window offsets, the
// residue range through frame_plan / window_at, the letters read as clipped 16-byte blocks with head and tail masks, the
// byte-compare popcount, the threshold — over batches that hold a record of every length 0 .. 120 nt.  Every window's begin,
// length and stops must equal a byte-by-byte count over translate_frame's letters (host/encoder.cpp) with the windows cut
// by a restatement of `tetrex search --window`, and its threshold the rule of DESIGN.md §20 restated.  The frames lie in a
// heap block that ends exactly at frames_bytes, at every alignment 0 .. 15, so a load at or behind frames_bytes is a heap
// overflow under the address sanitizer; the loader also checks every whole-block load against the buffer's bounds itself.
// A second pass gives the walk a buffer cut short in the middle of a window: nothing at or behind the cut may be read, and the
// windows that leave it must be found outside.
// Built with sanitizers by tests/test_verify_frame_windows_cpu.py:
//   g++ -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o sim
//       tests/native/frame_window_letters_sim.cpp tetrex_amd/csrc/host/encoder.cpp && ./sim
// Prints "frame_window_letters_sim ok: <batches> batches, <windows> windows, <stops> stops, <loads> loads, <unsearched> not searched"
// and exits 0, or names the first difference and exits 1.
#include "../../tetrex_amd/csrc/host/encoder.hpp"
#include "../../tetrex_amd/csrc/txq_frame_windows_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <utility>
#include <vector>

using namespace txq;

namespace {

[[noreturn]] void die(const char* what, uint64_t a = 0, uint64_t b = 0, uint64_t c = 0, uint64_t d = 0) {
    std::printf("frame_window_letters_sim: %s (%llu, %llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c,
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

uint64_t n_loads = 0;
struct CheckedLoad {
    text4 operator()(uintptr_t blk, uintptr_t lo, uintptr_t hi) const {
        if (blk % 16) die("a block that is not aligned", blk);
        if (blk + 16 <= lo || blk >= hi) die("a block with no byte of the buffer", blk - lo, hi - lo);
        const TextBlock b = load_block(blk, lo, hi, 0);
        if (b.whole && (blk < lo || blk + 16 > hi)) die("a whole load that leaves the buffer", blk - lo, hi - lo);
        ++n_loads;
        return b.w;
    }
};

struct Totals {
    uint64_t batches = 0, windows = 0, stops = 0, unsearched = 0;
};

void run_batch(const std::vector<std::string>& records, uint32_t k, uint32_t W, uint32_t S, uint32_t E, size_t align, Totals& tot) {
    const size_t n = records.size(), m = 6 * n;
    std::vector<uint64_t> rec{7}, foff{0}, woff{0};  // (the record offsets need not begin at 0: only their differences count)
    std::string frames;
    struct Want { uint64_t begin, len, stops, w; };
    std::vector<Want> want;
    for (const std::string& s : records) {
        rec.push_back(rec.back() + s.size());
        for (unsigned f = 0; f < 6; ++f) {
            const std::string residues = tetrex::translate_frame(s, f);
            for (const auto& [a, len] : windows_of(residues.size(), k, W, S)) {
                uint64_t stops = 0, w = 0;
                for (uint64_t i = a; i < a + len; ++i) stops += residues[i] == '*';
                for (uint64_t c = a; c + k <= a + len; ++c) w += residues.find('*', c) >= c + k;
                want.push_back({frames.size() + a, len, stops, w});
            }
            frames += residues;
            foff.push_back(frames.size());
            woff.push_back(want.size());
            if (woff.back() - woff[woff.size() - 2] != fw::window_count(residues.size(), k, W, S)) die("window_count differs from the restatement", residues.size(), f);
        }
    }
    std::vector<uint32_t> wlen;
    for (const Want& x : want) wlen.push_back((uint32_t)x.w);
    // pass 0: the buffer holds all frames and ends with them; pass 1: it is cut short inside the last third of the letters
    for (int pass = 0; pass < 2; ++pass) {
        const uint64_t bytes = pass == 0 ? frames.size() : frames.size() - frames.size() / 3;
        if (pass == 1 && bytes == frames.size()) continue;
        uint8_t* block = (uint8_t*)std::malloc(align + bytes + (align + bytes == 0));
        uint8_t* buf = block + align;
        std::memset(block, '*', align);  // (stops in front of the buffer: counting one of them is a difference)
        std::memcpy(buf, frames.data(), bytes);
        const uintptr_t lo = (uintptr_t)buf, hi = lo + bytes;
        for (uint64_t j = 0; j < want.size() + 3; ++j) {  // (+3: window indexes behind the last are answered too)
            const fw::Letters at = fw::window_letters(rec.data(), foff.data(), woff.data(), m, j, k, W, S);
            if (j >= want.size()) {
                if (at.len != 0 || fw::letters_inside(at, bytes)) die("a window behind the last one", j);
                continue;
            }
            const Want& x = want[j];
            if (at.begin != x.begin || at.len != x.len) die("begin or length differs", j, at.begin, x.begin, at.len);
            const bool inside = fw::letters_inside(at, bytes);
            if (inside != (x.begin + x.len <= bytes)) die("inside differs", j, x.begin, x.len, bytes);
            if (!inside) {
                // what the kernel does not do, done here all the same: the walk over a window that leaves the buffer reads nothing behind it
                (void)fw::count_stops(lo, hi, lo + at.begin, lo + at.begin + at.len, CheckedLoad{});
                ++tot.unsearched;
                continue;
            }
            const uint32_t s = fw::count_stops(lo, hi, lo + at.begin, lo + at.begin + at.len, CheckedLoad{});
            if (s != x.stops) die("stops differ", j, s, x.stops, align);
            const uint32_t t = fw::stop_threshold(wlen[j], s, k, E);
            const int64_t plain = (int64_t)x.w - (int64_t)k * ((int64_t)E - (int64_t)x.stops);
            const uint32_t t_want = x.stops > E || plain <= 0 ? 0xFFFFFFFFu : (uint32_t)plain;
            if (t != t_want) die("threshold differs", j, t, t_want);
            ++tot.windows;
            tot.stops += s;
            tot.unsearched += t == fw::kNotSearched;
        }
        std::free(block);
    }
    ++tot.batches;
}

}  // namespace

int main() {
    std::mt19937_64 rng(20);
    Totals tot;
    const uint32_t shapes[][3] = {{3, 8, 3}, {3, 8, 1}, {3, 8, 8}, {6, 8, 3}, {6, 40, 10}, {6, 6, 1}, {1, 17, 5}, {12, 33, 16}};  // k, W, S
    size_t align = 0;
    for (const auto& sh : shapes)
        for (int kind = 0; kind < 3; ++kind) {
            // a record of every length 0 .. 120: random letters; stop-dense (TAA, TGA and TAG repeats with a few other letters); mixed
            // case with U and N
            std::vector<std::string> records;
            for (size_t L = 0; L <= 120; ++L) {
                std::string s;
                while (s.size() < L) {
                    if (kind == 1 && rng() % 4) s += (rng() % 2 ? "TAA" : rng() % 2 ? "TGA" : "TAG");
                    else s += "ACGT"[rng() % 4];
                }
                s.resize(L);
                if (kind == 2)
                    for (char& c : s) {
                        if (rng() % 3 == 0) c = (char)(c | 0x20);
                        if ((c == 'T' || c == 't') && rng() % 2) c = (char)(c + 1);
                        if (rng() % 40 == 0) c = 'N';
                    }
                records.push_back(s);
            }
            for (uint32_t E = 0; E <= 3; ++E) run_batch(records, sh[0], sh[1], sh[2], E, align++ % 16, tot);
        }
    // every alignment of the buffer with one shape, and batches of one and of no record
    {
        std::vector<std::string> records;
        for (size_t L = 60; L <= 90; ++L) {
            std::string s;
            while (s.size() < L) s += rng() % 3 ? "ACGT"[rng() % 4] : 'T', s += rng() % 2 ? "AA" : "CG";
            s.resize(L);
            records.push_back(s);
        }
        for (size_t a = 0; a < 16; ++a) run_batch(records, 3, 8, 3, 1, a, tot);
        run_batch({records[30]}, 6, 8, 1, 2, 5, tot);
        run_batch({}, 6, 8, 1, 2, 0, tot);
        run_batch({"", "AC", ""}, 3, 8, 3, 2, 3, tot);
    }
    if (tot.stops == 0 || tot.unsearched == 0) die("no stops or nothing unsearched: the inputs check nothing");
    std::printf("frame_window_letters_sim ok: %llu batches, %llu windows, %llu stops, %llu loads, %llu not searched\n", (unsigned long long)tot.batches,
                (unsigned long long)tot.windows, (unsigned long long)tot.stops, (unsigned long long)n_loads, (unsigned long long)tot.unsearched);
    return 0;
}
