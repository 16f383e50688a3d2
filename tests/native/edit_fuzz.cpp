// Stand-alone check of host/edit_distance.hpp (multiword Myers) against the plain O(mn) table of Sellers' recurrence.
// Built with sanitizers on the CPU:
//   g++ -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/native/edit_fuzz.cpp -o edit_fuzz && ./edit_fuzz
// Prints "edit_fuzz ok: <cases> cases" and exits 0, or names the first case that differs and exits 1.
#include "../../tetrex_amd/csrc/host/edit_distance.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

using namespace tetrex;

namespace {

// the table itself: least D[m][j] over j and the lowest such j
void table(const std::vector<uint8_t>& p, const uint8_t* t, size_t n, const uint8_t* codes, uint32_t& best, size_t& at) {
    const size_t m = p.size();
    std::vector<uint32_t> prev(n + 1, 0), row(n + 1);
    for (size_t i = 1; i <= m; ++i) {
        row[0] = (uint32_t)i;
        const uint8_t c = codes[p[i - 1]];
        for (size_t j = 1; j <= n; ++j) {
            const uint8_t d = codes[t[j - 1]];
            const bool match = c == d && c != 255;
            row[j] = std::min({prev[j - 1] + (match ? 0u : 1u), prev[j] + 1, row[j - 1] + 1});
        }
        prev.swap(row);
    }
    best = prev[0], at = 0;
    for (size_t j = 1; j <= n; ++j)
        if (prev[j] < best) best = prev[j], at = j;
}

}  // namespace

int main(int argc, char** argv) {
    const unsigned rounds = argc > 1 ? (unsigned)std::atoi(argv[1]) : 600;
    std::mt19937_64 rng(20240607);
    size_t cases = 0;
    const size_t lengths[] = {1, 2, 3, 31, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 700};
    for (unsigned round = 0; round < rounds; ++round) {
        const unsigned letters = round % 3 == 0 ? 2 : round % 3 == 1 ? 4 : 20;
        uint8_t codes[256];
        for (unsigned b = 0; b < 256; ++b) codes[b] = 255;
        for (unsigned l = 0; l < letters; ++l) codes['A' + l] = codes['a' + l] = (uint8_t)l;
        const auto letter = [&]() -> uint8_t {
            const unsigned x = (unsigned)(rng() % (letters + 1));
            if (x == letters) return rng() % 2 ? (uint8_t)'#' : (uint8_t)(rng() % 256);  // mostly class 255
            return (uint8_t)((rng() % 2 ? 'A' : 'a') + x);
        };
        const size_t m = round < 2 * std::size(lengths) ? lengths[round % std::size(lengths)] : 1 + (size_t)(rng() % 140);
        std::vector<uint8_t> p(m);
        for (uint8_t& c : p) c = letter();
        // records: empty, one byte, m - 1, m, random, and one with an edited copy of the pattern inside
        std::vector<uint8_t> text;
        std::vector<uint64_t> rec{0};
        const size_t shapes[] = {0, 1, m - 1, m, (size_t)(rng() % 300), 0, (size_t)(rng() % 3000)};
        for (size_t len : shapes) {
            for (size_t i = 0; i < len; ++i) text.push_back(letter());
            rec.push_back(text.size());
        }
        {
            std::vector<uint8_t> copy = p;
            for (unsigned e = (unsigned)(rng() % 5); e > 0 && !copy.empty(); --e) {
                const size_t at = (size_t)(rng() % copy.size());
                switch (rng() % 3) {
                    case 0: copy[at] = letter(); break;
                    case 1: copy.insert(copy.begin() + (long)at, letter()); break;
                    default: copy.erase(copy.begin() + (long)at); break;
                }
            }
            for (size_t i = rng() % 50; i > 0; --i) text.push_back(letter());
            text.insert(text.end(), copy.begin(), copy.end());
            for (size_t i = rng() % 50; i > 0; --i) text.push_back(letter());
            rec.push_back(text.size());
        }
        text.push_back(0);  // (so that text.data() is valid for an all-empty text; not part of any record)
        EditPattern pat(p.data(), m, codes);
        const size_t R = rec.size() - 1;
        uint32_t group_best = kEditNone, group_rec = kEditNone, group_end = kEditNone;
        for (size_t r = 0; r < R; ++r) {
            uint32_t want, got;
            size_t want_at, got_at;
            table(p, text.data() + rec[r], (size_t)(rec[r + 1] - rec[r]), codes, want, want_at);
            pat.scan(text.data() + rec[r], (size_t)(rec[r + 1] - rec[r]), got, got_at);
            ++cases;
            if (want != got || want_at != got_at) {
                std::printf("edit_fuzz: round %u, m = %zu, record %zu of %zu bytes: table (%u, %zu), Myers (%u, %zu)\n", round, m, r,
                            (size_t)(rec[r + 1] - rec[r]), want, want_at, got, got_at);
                return 1;
            }
            if (want < group_best) group_best = want, group_rec = (uint32_t)r, group_end = (uint32_t)want_at;
        }
        for (uint32_t cap : {0u, 1u, 3u, (uint32_t)m - 1, (uint32_t)m, (uint32_t)m + 5}) {
            for (uint64_t r0 : {(uint64_t)0, (uint64_t)R}) {  // the whole group, and a group of no records
                const EditResult res = edit_search_group(pat, text.data(), rec.data(), r0, R, cap);
                const bool hit = r0 == 0 && group_best <= cap;
                const EditResult want = hit ? EditResult{group_best, group_rec, group_end} : EditResult{};
                ++cases;
                if (res.distance != want.distance || res.record != want.record || res.end != want.end) {
                    std::printf("edit_fuzz: round %u, m = %zu, cap %u: group gives (%u, %u, %u), the table (%u, %u, %u)\n", round, m, cap,
                                res.distance, res.record, res.end, want.distance, want.record, want.end);
                    return 1;
                }
            }
        }
    }
    std::printf("edit_fuzz ok: %zu cases\n", cases);
    return 0;
}
