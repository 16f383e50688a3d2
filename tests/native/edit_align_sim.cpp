// Stand-alone check of csrc/txq_edit_align_plan.hpp: the lane schedule of the alignment kernel (txq_edit_align.hip) run on the
// CPU — the 64 lanes as arrays, a cross-lane move as an index into one, a ballot as a loop over them, rows in blocks of 64 with the
// block's bytes fetched as the kernel fetches them — against edit_align_pair of host/edit_distance.hpp, word for word.
// Built with sanitizers by tests/test_edit_align_sim.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/edit_align_sim.cpp -o sim && ./sim
// Prints "edit_align_sim ok: <cases> cases ..." and exits 0, or names the first case that differs and exits 1.
#include "../../tetrex_amd/csrc/host/edit_distance.hpp"
#include "../../tetrex_amd/csrc/txq_edit_align_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

using namespace txq;

namespace {

constexpr uint32_t kFill = 0xA5A5A5A5u;

// One pair as a wave of the kernel answers it.  pattern / text are exact-size heap arrays: a byte read outside them stops the
// program.  Returns what the wave did: 'n' none, 'r' refused, 'd' declined, 'a' aligned.
char sim_pair(const std::vector<uint8_t>& pattern, const std::vector<uint8_t>& text, const std::vector<uint64_t>& rec, uint64_t r0, uint64_t r1,
              const uint32_t* result, const uint8_t* codes, uint32_t max_errors, uint32_t* out) {
    const uint32_t run_words = 2 * max_errors + 1;
    const uint32_t d = result[0], r = result[1], j = result[2], m = (uint32_t)pattern.size();
    const AlignKind kind = align_kind(d, r, j, m, max_errors, rec.data(), r0, r1, rec[r0], rec[r1]);
    if (kind == AlignKind::Declined) {
        out[0] = kAlignDeclined;
        return 'd';
    }
    if (kind != AlignKind::Run) {
        out[0] = kAlignNone, out[1] = kind == AlignKind::Refused ? kAlignDeclined : 0u;
        for (uint32_t x = 0; x < run_words; ++x) out[2 + x] = 0;
        return kind == AlignKind::Refused ? 'r' : 'n';
    }
    const AlignBand b{m, d, j};
    const uint8_t* const rtext = text.data() + rec[r];
    std::vector<uint64_t> dir(2 * (size_t)m);
    uint32_t prev[64], val[64], x[64], up[64], op[64], pc[64], ta[64], tb[64];
    bool match[64], in_band[64];
    int64_t col[64];
    for (uint32_t k = 0; k < 64; ++k) prev[k] = align_row0(b, k);
    for (uint32_t i0 = 0; i0 < m; i0 += 64) {
        for (uint32_t l = 0; l < 64; ++l) {
            pc[l] = ta[l] = tb[l] = 31;
            if (i0 + l < m) pc[l] = codes[pattern[i0 + l]];
            const int64_t xa = align_text_index(b, i0, l), xb = xa + 64;
            if (xa >= 0 && xa < (int64_t)j) ta[l] = codes[rtext[xa]];
            if (xb >= 0 && xb < (int64_t)j) tb[l] = codes[rtext[xb]];
        }
        const uint32_t rows = m - i0 < 64 ? m - i0 : 64;
        for (uint32_t ii = 0; ii < rows; ++ii) {
            const uint32_t i = i0 + ii + 1;
            for (uint32_t k = 0; k < 64; ++k) {
                const uint32_t p = pc[ii], src = ii + k;
                match[k] = p < 31 && p == (src < 64 ? ta[src & 63] : tb[src & 63]);
                up[k] = k < 2 * d && k < 63 ? prev[k + 1] : kAlignInf;  // (the last lane has no lane above)
                col[k] = align_column(b, i, k);
                in_band[k] = align_in_band(b, k, col[k]);
                x[k] = align_scan_bias(align_cell(in_band[k], col[k], i, up[k], prev[k], match[k]), k);
            }
            for (uint32_t s = 1; s <= 2 * d; s <<= 1)
                for (uint32_t k = 64; k-- > 0;) x[k] = align_scan_step(x[k], k >= s ? x[k - s] : kAlignInf);  // (descending: x[k - s] is the old one)
            uint64_t lo = 0, hi = 0;
            for (uint32_t k = 0; k < 64; ++k) {
                val[k] = align_scan_value(in_band[k], x[k], k);
                op[k] = align_op(col[k], val[k], up[k], prev[k], match[k]);
                lo |= (uint64_t)(op[k] & 1) << k;
                hi |= (uint64_t)(op[k] >> 1) << k;
            }
            dir[2 * (i - 1)] = lo, dir[2 * (i - 1) + 1] = hi;
            memcpy(prev, val, sizeof prev);
        }
    }
    bool lost = prev[d] != d;
    AlignWalk w = align_walk_begin(b);
    uint32_t mine[64] = {};
    while (!lost && w.i > 0) {
        const uint32_t closed = align_walk_step(w, dir[2 * (w.i - 1)], dir[2 * (w.i - 1) + 1]);
        if (closed) mine[w.n_runs - 1] = closed;
        lost = align_walk_lost(w, b) || w.n_runs > 2 * d;
    }
    const int64_t start = align_column(b, 0, w.k);
    if (lost || start < 0) {
        out[0] = kAlignDeclined;
        return 'd';
    }
    const uint32_t last = align_walk_end(w);
    mine[w.n_runs - 1] = last;
    out[0] = (uint32_t)start, out[1] = w.n_runs;
    for (uint32_t q = 0; q < w.n_runs; ++q) out[2 + align_run_slot(w.n_runs, q)] = mine[q];
    for (uint32_t q = w.n_runs; q < run_words; ++q) out[2 + q] = 0;
    return 'a';
}

std::mt19937_64 rng(20240611);
uint32_t below(uint32_t n) { return (uint32_t)(rng() % n); }

std::vector<uint8_t> random_text(const std::string& letters, size_t n, bool junk) {
    std::vector<uint8_t> t(n);
    for (uint8_t& c : t) c = junk && below(25) == 0 ? (uint8_t)'#' : (uint8_t)letters[below((uint32_t)letters.size())];
    return t;
}

// a letter of the alphabet that is not c
uint8_t another(const std::string& letters, uint8_t c) {
    const size_t at = letters.find((char)c);
    return (uint8_t)letters[(at == std::string::npos ? 0 : at + 1) % letters.size()];
}

size_t cases = 0, aligned = 0, declined = 0, clipped = 0, at_31 = 0;

int check(const std::vector<uint8_t>& pattern, const std::vector<uint8_t>& text, const std::vector<uint64_t>& rec, const uint32_t* result,
          const uint8_t* codes, uint32_t max_errors, const char* what) {
    const uint64_t r0 = 0, r1 = rec.size() - 1;
    const size_t stride = 2 * (size_t)max_errors + 3;
    std::vector<uint32_t> got(stride, kFill), want(stride, kFill);
    const char did = sim_pair(pattern, text, rec, r0, r1, result, codes, max_errors, got.data());
    tetrex::edit_align_pair(pattern.data(), pattern.size(), text.data(), rec.data(), r0, r1, result, codes, max_errors, want.data());
    ++cases;
    const bool over = result[0] != kAlignNone && (result[0] > kAlignMaxDistance || pattern.size() > kAlignMaxPattern);
    if (over) {  // the device's own limits: declined whatever the host twin says, and nothing else written
        ++declined;
        if (did == 'd' && got[0] == kAlignDeclined && std::all_of(got.begin() + 1, got.end(), [](uint32_t v) { return v == kFill; })) return 0;
    } else if (got == want) {
        if (did == 'a') {
            ++aligned;
            if ((int64_t)result[2] - (int64_t)pattern.size() - (int64_t)result[0] < 0) ++clipped;
            if (result[0] == kAlignMaxDistance) ++at_31;
        }
        return 0;
    }
    fprintf(stderr, "%s: m = %zu, (d, r, j) = (%u, %u, %u), max_errors %u: the schedule '%c' gives start %u, %u runs; the host twin start %u, %u runs\n", what,
            pattern.size(), result[0], result[1], result[2], max_errors, did, got[0], got[1], want[0], want[1]);
    return 1;
}

}  // namespace

int main() {
    const std::string dna = "ACGT", amino = "ACDEFGHIKLMNPQRSTVWY";
    for (const std::string* letters : {&dna, &amino}) {
        uint8_t codes[256];
        memset(codes, 255, sizeof codes);
        for (size_t c = 0; c < letters->size(); ++c) codes[(uint8_t)(*letters)[c]] = codes[(uint8_t)((*letters)[c] | 0x20)] = (uint8_t)c;
        for (const uint32_t m : {1u, 2u, 3u, 31u, 32u, 63u, 64u, 65u, 127u, 128u, 129u, 300u, 511u, 512u, 513u, 1025u, 4095u, 4096u, 4097u}) {
            for (const uint32_t edits : {0u, 1u, 2u, 5u, 31u, 32u, 33u}) {
                for (int where = 0; where < 3; ++where) {  // the copy at the record's start (the window is clipped), inside, at its end
                    std::vector<uint8_t> p = random_text(*letters, m, m > 8);
                    std::vector<uint8_t> copy = p;
                    // substitutions at distinct places far apart give d = edits where m allows; otherwise a mix of all three kinds
                    for (uint32_t e = 0; e < edits && !copy.empty(); ++e) {
                        const uint32_t kind = m >= 40 * edits ? 0 : below(3);
                        const size_t at = m >= 40 * edits ? (size_t)e * (m / edits) + 3 : below((uint32_t)copy.size());
                        if (kind == 0) copy[at] = another(*letters, copy[at]);
                        else if (kind == 1) copy.insert(copy.begin() + (long)at, (uint8_t)(*letters)[below((uint32_t)letters->size())]);
                        else copy.erase(copy.begin() + (long)at);
                    }
                    const std::vector<uint8_t> left = random_text(*letters, where == 0 ? 0 : 1 + below(90), true);
                    const std::vector<uint8_t> right = random_text(*letters, where == 2 ? 0 : 1 + below(90), true);
                    // the group: an empty record, one of a few letters, the target, an empty record
                    std::vector<uint8_t> text = random_text(*letters, 5, false);
                    std::vector<uint64_t> rec{0, 0, text.size()};
                    text.insert(text.end(), left.begin(), left.end());
                    text.insert(text.end(), copy.begin(), copy.end());
                    text.insert(text.end(), right.begin(), right.end());
                    rec.push_back(text.size());
                    rec.push_back(text.size());
                    text.shrink_to_fit();
                    tetrex::EditPattern ep(p.data(), p.size(), codes);
                    const tetrex::EditResult found = tetrex::edit_search_group(ep, text.data(), rec.data(), 0, rec.size() - 1, 0xFFFFFFFEu);
                    const uint32_t result[3] = {found.distance, found.record, found.end};
                    for (const uint32_t max_errors : {found.distance, 40u, found.distance ? found.distance - 1 : 0u})
                        if (check(p, text, rec, result, codes, max_errors, "planted")) return 1;
                    // triples that are no cell of this matrix: marked by both
                    const uint32_t odd[6][3] = {{found.distance + 1, found.record, found.end}, {found.distance, 9, found.end}, {found.distance, found.record, 0xFFFFFFF0u},
                                                {found.distance, 0, found.end}, {m + 1, found.record, found.end}, {kAlignNone, kAlignDeclined, kAlignDeclined}};
                    for (const auto& t : odd)
                        if (check(p, text, rec, t, codes, 40, "odd triple")) return 1;
                    const uint32_t none[3] = {kAlignNone, kAlignNone, kAlignNone};
                    if (check(p, text, rec, none, codes, 3, "none")) return 1;
                }
            }
        }
    }
    if (aligned < 500 || declined < 50 || clipped < 50 || at_31 < 5) {
        fprintf(stderr, "too few cases of a kind: %zu aligned, %zu declined, %zu clipped, %zu at d = 31\n", aligned, declined, clipped, at_31);
        return 1;
    }
    printf("edit_align_sim ok: %zu cases, %zu aligned, %zu over the device's limits, %zu clipped windows, %zu at d = 31\n", cases, aligned, declined, clipped, at_31);
    return 0;
}
