// Differential test of the exported automaton (Matcher::export_dfa, include/txq_regex.h) — native, no GPU, no Python:
//   regex_filter_fuzz [seed] [cases]
// Random patterns of the grammar matcher_fuzz.cpp generates (plus `^` / `$` now and then) x random texts: the blob's inline
// interpreter txq_regex_record_matches against Matcher::contains, under both semantics; the reversed automaton with the
// complement as byte map against contains() on the reverse complement; and find_all reporting a match exactly where the
// automaton accepts.  Texts include empty ones, bytes outside the alphabet and lower case.
//   g++ -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/native/regex_filter_fuzz.cpp \
//       tetrex_amd/csrc/host/matcher.cpp -o regex_filter_fuzz && ./regex_filter_fuzz
// Prints "regex_filter_fuzz ok: <comparisons> comparisons" and exits 0, or names the first cases that differ and exits 1.
#include "../../include/txq_regex.h"
#include "../../tetrex_amd/csrc/host/matcher.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

using tetrex::Matcher;

static std::mt19937_64 rng;
static int pick(int n) { return (int)(rng() % (uint64_t)n); }

struct Gen { std::string s; bool nullable; };

static Gen gen(const std::string& alphabet, int depth) {
    const int r = pick(depth > 0 ? 10 : 4);
    auto letter = [&]() { return std::string(1, alphabet[pick((int)alphabet.size())]); };
    switch (r) {
        case 0: case 1: return {letter(), false};
        case 2: return {".", false};
        case 3: {
            std::string s = pick(4) == 0 ? "[^" : "[";
            const int n = 1 + pick(3);
            for (int i = 0; i < n; ++i) s += letter();
            return {s + "]", false};
        }
        case 4: case 5: { const Gen a = gen(alphabet, depth - 1), b = gen(alphabet, depth - 1); return {a.s + b.s, a.nullable && b.nullable}; }
        case 6: { const Gen a = gen(alphabet, depth - 1), b = gen(alphabet, depth - 1); return {"(" + a.s + "|" + b.s + ")", a.nullable || b.nullable}; }
        case 7: {
            const char op = "*+?"[pick(3)];
            Gen a = gen(alphabet, depth - 1);
            while (op != '?' && a.nullable) a = gen(alphabet, depth - 1);
            return {"(" + a.s + ")" + op, op != '+'};
        }
        case 8: {
            const int lo = pick(3), hi = lo + pick(3);
            Gen a = gen(alphabet, depth - 1);
            while (a.nullable) a = gen(alphabet, depth - 1);
            char buf[32];
            const bool exact = pick(3) == 0;
            if (exact) std::snprintf(buf, sizeof buf, "{%d}", lo + 1);
            else std::snprintf(buf, sizeof buf, "{%d,%d}", lo, hi + (hi == 0));
            return {"(" + a.s + ")" + buf, !exact && lo == 0};
        }
        default: { const Gen a = gen(alphabet, depth - 1), b = gen(alphabet, depth - 1), c = gen(alphabet, depth - 1); return {a.s + b.s + c.s, a.nullable && b.nullable && c.nullable}; }
    }
}

static char complement(char c) {
    switch (c) {
        case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A';
        case 'a': return 't'; case 'c': return 'g'; case 'g': return 'c'; case 't': return 'a';
        default: return c;
    }
}

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    const int cases = argc > 2 ? std::atoi(argv[2]) : 1500;
    rng.seed(seed);
    uint8_t comp[256];
    for (unsigned b = 0; b < 256; ++b) comp[b] = (uint8_t)complement((char)b);
    size_t compared = 0;
    int bad = 0;
    for (int c = 0; c < cases && bad < 10; ++c) {
        const bool dna = pick(2) == 0;
        const std::string alphabet = dna ? "ACGT" : "ACDEKL";
        std::string pattern = gen(alphabet, 3).s;
        if (pick(6) == 0) pattern = "^" + pattern;
        if (pick(6) == 0) pattern += "$";
        pattern = "(" + pattern + ")";
        for (int posix = 0; posix < 2; ++posix) {
            const Matcher m(pattern, posix ? Matcher::Semantics::LeftmostLongest : Matcher::Semantics::LeftmostFirst);
            Matcher::Cache cache;
            std::vector<uint8_t> fwd, rev;
            if (!m.export_dfa(false, nullptr, fwd) || !m.export_dfa(true, comp, rev)) {
                std::printf("regex_filter_fuzz: %s does not export\n", pattern.c_str());
                ++bad;
                continue;
            }
            txq_regex_view v;
            if (!txq_regex_open(fwd.data(), fwd.size(), &v) || !txq_regex_open(rev.data(), rev.size(), &v)) {
                std::printf("regex_filter_fuzz: the blob of %s does not open\n", pattern.c_str());
                ++bad;
                continue;
            }
            for (int t = 0; t < 8; ++t) {
                std::string text(t == 0 ? 0 : pick(48), 'A');
                for (char& ch : text) {
                    ch = alphabet[pick((int)alphabet.size())];
                    if (pick(24) == 0) ch = "\n*xn\xff"[pick(5)];
                    else if (pick(24) == 0) ch = (char)(ch | 0x20);
                }
                const auto bytes = reinterpret_cast<const uint8_t*>(text.data());
                const bool want = m.contains(text, cache);
                size_t n_found = 0;
                m.find_all(text, cache, [&](size_t, size_t) { ++n_found; });
                const bool got = txq_regex_record_matches(fwd.data(), bytes, text.size());
                std::string rc(text.rbegin(), text.rend());
                for (char& ch : rc) ch = complement(ch);
                const bool want_rc = m.contains(rc, cache);
                const bool got_rc = txq_regex_record_matches(rev.data(), bytes, text.size());
                compared += 3;
                if (got != want || (n_found > 0) != want || got_rc != want_rc) {
                    ++bad;
                    std::printf("MISMATCH %s pattern %s text \"%s\": automaton %d, contains %d, find_all %zu; reverse strand automaton %d, contains %d\n",
                                posix ? "posix" : "perl", pattern.c_str(), text.c_str(), (int)got, (int)want, n_found, (int)got_rc, (int)want_rc);
                }
            }
        }
    }
    if (bad) return 1;
    std::printf("regex_filter_fuzz ok: %zu comparisons\n", compared);
    return 0;
}
