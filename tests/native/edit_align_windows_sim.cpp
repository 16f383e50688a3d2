// Stand-alone check of the window form of csrc/txq_edit_align_plan.hpp (txq_edit_align_windows_device): what a
// wave of the kernel does for a pair (window, view, cap) — align_window_ok over the window arrays, the view read once,
// align_window_kind on the triple, then the lane schedule of the alignment kernel with the 64 lanes as arrays — run on the CPU
// over one letter buffer and a table of three views, against edit_align_pair of host/edit_distance.hpp on the window written
// out, word for word.  Every array is an exact-size heap array and the answers lie between guard words: a byte read or written
// outside stops the program.  Built with sanitizers by tests/test_edit_align_windows_sim.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/edit_align_windows_sim.cpp -o sim && ./sim
// Prints "edit_align_windows_sim ok: ..." and exits 0, or names the first case that differs and exits 1.
#include "../../tetrex_amd/csrc/host/edit_distance.hpp"
#include "../../tetrex_amd/csrc/txq_edit_align_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

using namespace txq;

namespace {

constexpr uint32_t kFill = 0xA5A5A5A5u, kGuard = 8;

// what the call is given; every vector is exactly as long as the call is told
struct Call {
    std::vector<uint8_t> letters;
    std::vector<uint64_t> win_begin;
    std::vector<uint32_t> win_len;
    std::vector<std::vector<uint8_t>> texts;
    std::vector<std::vector<uint64_t>> recs;
    std::vector<AlignTextView> views;
    uint64_t n_windows, n_views;  // what the call is told (the arrays may be longer in a test of the index checks)
    uint8_t codes[256];
};

// The lane schedule of edit_align_kernel for a pair that runs: m pattern bytes at ptext, bytes [0, j) of the record at rtext.
// Returns false where the wave declines (the band does not hold d at (m, j), or the walk leaves it).
bool sim_schedule(const uint8_t* ptext, uint32_t m, const uint8_t* rtext, uint32_t d, uint32_t j, const uint8_t* codes, uint32_t run_words, uint32_t* out) {
    const AlignBand b{m, d, j};
    std::vector<uint64_t> dir(2 * (size_t)m);
    uint32_t prev[64], val[64], x[64], up[64], op[64], pc[64], ta[64], tb[64];
    bool match[64], in_band[64];
    int64_t col[64];
    for (uint32_t k = 0; k < 64; ++k) prev[k] = align_row0(b, k);
    for (uint32_t i0 = 0; i0 < m; i0 += 64) {
        for (uint32_t l = 0; l < 64; ++l) {
            pc[l] = ta[l] = tb[l] = 31;
            if (i0 + l < m) pc[l] = codes[ptext[i0 + l]];
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
                up[k] = k < 2 * d && k < 63 ? prev[k + 1] : kAlignInf;
                col[k] = align_column(b, i, k);
                in_band[k] = align_in_band(b, k, col[k]);
                x[k] = align_scan_bias(align_cell(in_band[k], col[k], i, up[k], prev[k], match[k]), k);
            }
            for (uint32_t s = 1; s <= 2 * d; s <<= 1)
                for (uint32_t k = 64; k-- > 0;) x[k] = align_scan_step(x[k], k >= s ? x[k - s] : kAlignInf);
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
    if (lost || start < 0) return false;
    const uint32_t last = align_walk_end(w);
    mine[w.n_runs - 1] = last;
    out[0] = (uint32_t)start, out[1] = w.n_runs;
    for (uint32_t q = 0; q < w.n_runs; ++q) out[2 + align_run_slot(w.n_runs, q)] = mine[q];
    for (uint32_t q = w.n_runs; q < run_words; ++q) out[2 + q] = 0;
    return true;
}

// One pair as a wave answers it: admit() of the kernel for the window form, then the markers or the schedule.
// 'n' none, 'r' refused, 'd' declined, 'a' aligned.
char sim_pair(const Call& c, const uint32_t* pair, const uint32_t* result, uint32_t max_errors, uint32_t* out) {
    const uint32_t run_words = 2 * max_errors + 1;
    const uint32_t p = pair[0], g = pair[1], d = result[0], r = result[1], j = result[2];
    AlignKind kind = AlignKind::Refused;
    uint32_t m = 0;
    AlignTextView v{};
    if (align_window_ok(p, g, c.n_windows, c.n_views, c.win_begin.data(), c.win_len.data(), c.letters.size())) {
        v = c.views[g];
        m = c.win_len[p];
        kind = align_window_kind(d, r, j, m, max_errors, v);
    }
    if (kind == AlignKind::Run && !sim_schedule(c.letters.data() + c.win_begin[p], m, v.text + v.rec[r], d, j, c.codes, run_words, out)) kind = AlignKind::Declined;
    if (kind == AlignKind::Run) return 'a';
    if (kind == AlignKind::Declined) {
        out[0] = kAlignDeclined;
        return 'd';
    }
    out[0] = kAlignNone, out[1] = kind == AlignKind::Refused ? kAlignDeclined : 0u;
    for (uint32_t x = 0; x < run_words; ++x) out[2 + x] = 0;
    return kind == AlignKind::Refused ? 'r' : 'n';
}

std::mt19937_64 rng(20250317);
uint32_t below(uint32_t n) { return (uint32_t)(rng() % n); }

std::vector<uint8_t> random_text(const std::string& letters, size_t n, bool junk) {
    std::vector<uint8_t> t(n);
    for (uint8_t& c : t) c = junk && below(25) == 0 ? (uint8_t)'#' : (uint8_t)letters[below((uint32_t)letters.size())];
    return t;
}
uint8_t another(const std::string& letters, uint8_t c) {
    const size_t at = letters.find((char)c);
    return (uint8_t)letters[(at == std::string::npos ? 0 : at + 1) % letters.size()];
}

size_t cases = 0, aligned = 0, declined = 0, refused = 0, none = 0, clipped = 0, at_31 = 0, long_windows = 0;

// `expect`: 0 compare with the host twin; 'r' / 'd': this outcome with exactly its words written (what the host twin cannot be
// asked: an index outside an array, offsets that leave the text, the device's own limits)
int check(const Call& c, const uint32_t* pair, const uint32_t* result, uint32_t max_errors, char expect, const char* what) {
    const size_t stride = 2 * (size_t)max_errors + 3;
    std::vector<uint32_t> got(kGuard + stride + kGuard, kFill), want(stride, kFill);
    const char did = sim_pair(c, pair, result, max_errors, got.data() + kGuard);
    ++cases;
    bool ok = std::all_of(got.begin(), got.begin() + kGuard, [](uint32_t v) { return v == kFill; }) &&
              std::all_of(got.end() - kGuard, got.end(), [](uint32_t v) { return v == kFill; });
    const uint32_t* o = got.data() + kGuard;
    if (expect == 'd') ok = ok && did == 'd' && o[0] == kAlignDeclined && std::all_of(o + 1, o + stride, [](uint32_t v) { return v == kFill; });
    else if (expect == 'r') ok = ok && did == 'r' && o[0] == kAlignNone && o[1] == kAlignDeclined && std::all_of(o + 2, o + stride, [](uint32_t v) { return v == 0; });
    else {
        const std::vector<uint8_t> written(c.letters.begin() + (long)c.win_begin[pair[0]], c.letters.begin() + (long)(c.win_begin[pair[0]] + c.win_len[pair[0]]));
        const auto& rec = c.recs[pair[1]];
        tetrex::edit_align_pair(written.data(), written.size(), c.texts[pair[1]].data(), rec.data(), 0, rec.size() - 1, result, c.codes, max_errors, want.data());
        ok = ok && std::equal(want.begin(), want.end(), o);
    }
    if (ok) {
        if (did == 'a') {
            ++aligned;
            if ((int64_t)result[2] - (int64_t)c.win_len[pair[0]] - (int64_t)result[0] < 0) ++clipped;
            if (result[0] == kAlignMaxDistance) ++at_31;
        }
        declined += did == 'd', refused += did == 'r', none += did == 'n';
        return 0;
    }
    fprintf(stderr, "%s: pair (%u, %u), (d, r, j) = (%u, %u, %u), max_errors %u: the schedule '%c' gives %u, %u; expected '%c' %u, %u\n", what, pair[0], pair[1],
            result[0], result[1], result[2], max_errors, did, o[0], o[1], expect ? expect : '=', want[0], want[1]);
    return 1;
}

void finish(Call& c) {
    c.views.clear();
    for (size_t g = 0; g < c.texts.size(); ++g) {
        c.texts[g].shrink_to_fit();
        c.views.push_back({c.texts[g].data(), c.recs[g].data(), c.recs[g].size() - 1, c.texts[g].size()});
    }
    c.n_windows = c.win_begin.size(), c.n_views = c.views.size();
}

}  // namespace

int main() {
    const std::string dna = "ACGT", amino = "ACDEFGHIKLMNPQRSTVWY";
    for (const std::string* letters : {&dna, &amino}) {
        Call c;
        memset(c.codes, 255, sizeof c.codes);
        for (size_t x = 0; x < letters->size(); ++x) c.codes[(uint8_t)(*letters)[x]] = c.codes[(uint8_t)((*letters)[x] | 0x20)] = (uint8_t)x;
        for (const uint32_t m : {1u, 2u, 3u, 31u, 63u, 64u, 65u, 127u, 128u, 129u, 300u, 511u, 512u, 513u, 700u}) {
            for (const uint32_t edits : {0u, 1u, 2u, 5u, 31u, 32u}) {
                // the letters: three windows of m letters that overlap in all but one, in descending order, the last one ending at the
                // buffer's last byte; window 3 is window 1 again
                c.letters = random_text(*letters, m + 2 + below(40), m > 8);
                const uint64_t last = c.letters.size() - m;
                c.letters.shrink_to_fit();
                c.win_begin = {last, last - 1, last - 2, last - 1};
                c.win_len = {m, m, m, m};
                // view 0: one record, the copy of window 0 at its very end (the match ends at the last text byte);
                // view 1: seven records, empty ones in front, the copy of window 1 at byte 0 of the text (the band is clipped there);
                // view 2: no records
                std::vector<uint8_t> copy[2];
                for (int w = 0; w < 2; ++w) {
                    copy[w].assign(c.letters.begin() + (long)c.win_begin[w], c.letters.begin() + (long)c.win_begin[w] + m);
                    for (uint32_t e = 0; e < edits && !copy[w].empty(); ++e) {
                        const bool apart = m >= 16 * edits;
                        const uint32_t kind = apart ? 0 : below(3);
                        const size_t at = apart ? (size_t)e * (m / edits) + 3 % m : below((uint32_t)copy[w].size());
                        if (kind == 0) copy[w][at % copy[w].size()] = another(*letters, copy[w][at % copy[w].size()]);
                        else if (kind == 1) copy[w].insert(copy[w].begin() + (long)at, (uint8_t)(*letters)[below((uint32_t)letters->size())]);
                        else copy[w].erase(copy[w].begin() + (long)at);
                    }
                }
                c.texts.assign(3, {});
                c.recs.assign(3, {});
                c.texts[0] = random_text(*letters, 1 + below(90), true);
                c.texts[0].insert(c.texts[0].end(), copy[0].begin(), copy[0].end());
                c.recs[0] = {0, c.texts[0].size()};
                c.texts[1] = copy[1];
                const std::vector<uint8_t> right = random_text(*letters, 1 + below(90), true), more = random_text(*letters, 9, false);
                c.texts[1].insert(c.texts[1].end(), right.begin(), right.end());
                const uint64_t e1 = c.texts[1].size();
                c.texts[1].insert(c.texts[1].end(), more.begin(), more.end());
                c.recs[1] = {0, 0, 0, e1, e1, e1 + 4, e1 + 4, e1 + 9};
                c.recs[2] = {0};
                finish(c);
                for (uint32_t w = 0; w < 4; ++w) {
                    for (uint32_t g = 0; g < 2; ++g) {
                        const std::vector<uint8_t> written(c.letters.begin() + (long)c.win_begin[w], c.letters.begin() + (long)c.win_begin[w] + m);
                        tetrex::EditPattern ep(written.data(), written.size(), c.codes);
                        const tetrex::EditResult found = tetrex::edit_search_group(ep, c.texts[g].data(), c.recs[g].data(), 0, c.recs[g].size() - 1, 0xFFFFFFFEu);
                        const uint32_t pair[3] = {w, g, 40}, result[3] = {found.distance, found.record, found.end};
                        const bool over = m > kAlignMaxWindow || found.distance > kAlignMaxDistance;
                        long_windows += m > kAlignMaxWindow;
                        for (const uint32_t max_errors : {found.distance, 40u, found.distance ? found.distance - 1 : 0u})
                            if (check(c, pair, result, max_errors, over ? 'd' : 0, "planted")) return 1;
                        if (m > kAlignMaxWindow) continue;
                        // triples that are no cell of this matrix
                        const uint32_t n_rec = (uint32_t)c.recs[g].size() - 1;
                        const uint32_t odd[6][3] = {{found.distance + 1, found.record, found.end}, {found.distance, n_rec, found.end},
                                                    {found.distance, 0xFFFFFFF0u, found.end},      {found.distance, found.record, 0xFFFFFFF0u},
                                                    {m + 1, found.record, found.end},              {found.distance, found.record, found.end + 1 + (uint32_t)c.texts[g].size()}};
                        for (const auto& t : odd)
                            if (check(c, pair, t, 40, t[1] >= n_rec || t[0] > kAlignMaxDistance ? 'd' : 0, "odd triple")) return 1;
                    }
                    // view 2 has no records: "none" is what a search answers, and any record index is outside it
                    const uint32_t pair[3] = {w, 2, 40}, nothing[3] = {kAlignNone, kAlignNone, kAlignNone}, marker[3] = {kAlignNone, kAlignDeclined, kAlignDeclined},
                                   zero[3] = {0, 0, 0};
                    if (check(c, pair, nothing, 3, 0, "none") || check(c, pair, marker, 3, 0, "marker") || check(c, pair, zero, 3, 'd', "record of an empty view")) return 1;
                }
                // refusals: a window index, a view index out of range (the arrays end where the call is told they end), an empty window, a
                // window that leaves the letters — by its length, by its begin, by a begin near 2^64
                const uint32_t good[3] = {0, 0, m};
                const uint32_t bad_window[3] = {4, 0, 40}, huge_window[3] = {0xFFFFFFFFu, 0, 40}, bad_view[3] = {0, 3, 40}, huge_view[3] = {0, 0xFFFFFFFFu, 40};
                for (const auto* pr : {bad_window, huge_window, bad_view, huge_view})
                    if (check(c, pr, good, 40, 'r', "index out of range")) return 1;
                Call b = c;
                b.win_len[0] = 0, b.win_len[1] = m + 3, b.win_begin[2] = b.letters.size() + 1, b.win_begin[3] = ~0ULL - 2;
                finish(b);
                for (uint32_t w = 0; w < 4; ++w) {
                    const uint32_t pair[3] = {w, 0, 40};
                    if (check(b, pair, good, 40, 'r', "window outside the letters")) return 1;
                }
                if (m > kAlignMaxWindow) continue;
                // views whose offsets are wrong: they leave the text, they descend; the table says fewer records than the offsets hold
                Call o = c;
                o.recs[0] = {0, o.texts[0].size() + 1};
                o.recs[1] = {0, 0, 9, 5, 5, 5, 5, 5};
                finish(o);
                const uint32_t p0[3] = {0, 0, 40}, p1[3] = {1, 1, 40}, leaves[3] = {0, 0, 1}, descends[3] = {0, 2, 1};
                if (check(o, p0, leaves, 40, 'd', "offsets that leave the text") || check(o, p1, descends, 40, 'd', "offsets that descend")) return 1;
            }
        }
    }
    if (aligned < 400 || declined < 200 || refused < 200 || none < 100 || clipped < 50 || at_31 < 4 || long_windows < 20) {
        fprintf(stderr, "too few cases of a kind: %zu aligned, %zu declined, %zu refused, %zu none, %zu clipped, %zu at d = 31, %zu long windows\n", aligned, declined,
                refused, none, clipped, at_31, long_windows);
        return 1;
    }
    printf("edit_align_windows_sim ok: %zu cases, %zu aligned, %zu declined, %zu refused, %zu none, %zu clipped windows, %zu at d = 31\n", cases, aligned, declined,
           refused, none, clipped, at_31);
    return 0;
}
