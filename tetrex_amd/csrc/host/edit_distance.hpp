// Host side: approximate matching of a pattern against the records of a bin by edit distance (`tetrex search --verify`,
// DESIGN.md §12; the semantics are spelled out in include/txq.h at txq_edit_search_device).  Myers' bit-parallel form of
// Sellers' recurrence with the pattern as ONE integer of ceil(m / 64) words: the addition carries and the shifts run over
// all words, so there is no limit on m.  This is the host twin of the kernel in txq_edit.hip: it answers patterns longer
// than TXQ_EDIT_MAX_PATTERN and it is what the kernel is measured against.  Header only, no dependencies.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace tetrex {

constexpr uint32_t kEditNone = 0xFFFFFFFFu;
struct EditResult {
    uint32_t distance = kEditNone, record = kEditNone, end = kEditNone;  // all kEditNone: nothing within the cap
};

// One pattern, prepared: its match vectors by class.  codes[256] maps a byte to a class 0..30; any other value is
// "matches nothing, not even itself" (row 31 stays zero, and such a pattern byte sets no bit anywhere).
class EditPattern {
  public:
    EditPattern(const uint8_t* pattern, size_t m, const uint8_t* codes) : m_(m), words_((m + 63) / 64), codes_(codes) {
        peq_.assign(32 * words_, 0);
        for (size_t i = 0; i < m; ++i) {
            const uint8_t c = codes[pattern[i]];
            if (c < 31) peq_[c * words_ + (i >> 6)] |= 1ULL << (i & 63);
        }
        pv_.resize(words_);
        mv_.resize(words_);
    }
    size_t length() const { return m_; }

    // min over j = 0..n of D[m][j] for the record text[0 .. n), and the lowest j that reaches it (j = 0: D = m)
    void scan(const uint8_t* text, size_t n, uint32_t& distance, size_t& end) {
        if (words_ == 1) return scan_one(text, n, distance, end);
        const size_t W = words_, hw = (m_ - 1) >> 6;
        const unsigned hs = (unsigned)((m_ - 1) & 63);
        for (size_t w = 0; w < W; ++w) pv_[w] = ~0ULL, mv_[w] = 0;
        uint32_t score = (uint32_t)m_, best = (uint32_t)m_;
        size_t at = 0;
        for (size_t j = 0; j < n; ++j) {
            const uint8_t c = codes_[text[j]];
            const uint64_t* eqrow = &peq_[(c < 31 ? c : 31) * W];
            uint64_t carry = 0, ph_in = 0, mh_in = 0;
            for (size_t w = 0; w < W; ++w) {
                const uint64_t eq = eqrow[w], pv = pv_[w], mv = mv_[w];
                const uint64_t xv = eq | mv, a = eq & pv;
                const uint64_t s1 = a + pv, s2 = s1 + carry;
                carry = (uint64_t)(s1 < a) | (uint64_t)(s2 < s1);
                const uint64_t xh = (s2 ^ pv) | eq;
                uint64_t ph = mv | ~(xh | pv), mh = pv & xh;
                if (w == hw) score += (uint32_t)((ph >> hs) & 1) - (uint32_t)((mh >> hs) & 1);
                const uint64_t ph_out = ph >> 63, mh_out = mh >> 63;
                ph = (ph << 1) | ph_in;
                mh = (mh << 1) | mh_in;
                ph_in = ph_out;
                mh_in = mh_out;
                pv_[w] = mh | ~(xv | ph);
                mv_[w] = ph & xv;
            }
            if (score < best) best = score, at = j + 1;
        }
        distance = best;
        end = at;
    }

  private:
    void scan_one(const uint8_t* text, size_t n, uint32_t& distance, size_t& end) const {
        const unsigned hs = (unsigned)(m_ - 1);
        uint64_t pv = ~0ULL, mv = 0;
        uint32_t score = (uint32_t)m_, best = (uint32_t)m_;
        size_t at = 0;
        for (size_t j = 0; j < n; ++j) {
            const uint8_t c = codes_[text[j]];
            const uint64_t eq = peq_[c < 31 ? c : 31];
            const uint64_t xv = eq | mv;
            const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
            uint64_t ph = mv | ~(xh | pv), mh = pv & xh;
            score += (uint32_t)((ph >> hs) & 1) - (uint32_t)((mh >> hs) & 1);
            ph <<= 1;
            mh <<= 1;
            pv = mh | ~(xv | ph);
            mv = ph & xv;
            if (score < best) best = score, at = j + 1;
        }
        distance = best;
        end = at;
    }

    size_t m_, words_;
    const uint8_t* codes_;
    std::vector<uint64_t> peq_, pv_, mv_;
};

// One pair: the pattern against records [r0, r1) of `text` (record r is text[rec[r] .. rec[r+1])), cap e.  The lowest
// record that reaches the least distance, and the lowest end position in it.
inline EditResult edit_search_group(EditPattern& p, const uint8_t* text, const uint64_t* rec, uint64_t r0, uint64_t r1, uint32_t cap) {
    EditResult out;
    uint32_t best = kEditNone;
    for (uint64_t r = r0; r < r1; ++r) {
        uint32_t d;
        size_t j;
        p.scan(text + rec[r], (size_t)(rec[r + 1] - rec[r]), d, j);
        if (d < best) {
            best = d;
            out.record = (uint32_t)r;
            out.end = (uint32_t)j;
            if (d == 0) break;
        }
    }
    if (best <= cap) out.distance = best;
    else out = EditResult{};
    return out;
}

// One pair, every target (include/txq.h at txq_edit_targets_device): each record of [r0, r1) whose least
// distance is within the cap, in record order, appended to `hits` as (pair, d, r, j), j the lowest end that reaches d.  The
// least (d, r, j) of what is appended is what edit_search_group answers for the pair.
inline void edit_targets_group(EditPattern& p, const uint8_t* text, const uint64_t* rec, uint64_t r0, uint64_t r1, uint32_t cap, uint32_t pair,
                               std::vector<uint32_t>& hits) {
    for (uint64_t r = r0; r < r1; ++r) {
        uint32_t d;
        size_t j;
        p.scan(text + rec[r], (size_t)(rec[r + 1] - rec[r]), d, j);
        if (d <= cap) hits.insert(hits.end(), {pair, d, (uint32_t)r, (uint32_t)j});
    }
}

// ---- where a match begins, and its alignment (include/txq.h at txq_edit_align_device) -------------------
// The host twin of the kernel in txq_edit_align.hip, with no limit on m or d: it answers the pairs the device declines and is
// what the kernel is compared with.  Sellers' matrix on the 2 d + 1 diagonals around the one through (m, j) — row by row,
// cell (i, k) being column j - m + i + k - d —, two bits of direction per cell, then the walk back by the three rules.
constexpr uint32_t kEditNotAligned = 0xFFFFFFFEu;
constexpr uint32_t kEditOpMatch = 0, kEditOpMismatch = 1, kEditOpInsert = 2, kEditOpDelete = 3;  // = X I D
struct EditAlignment {
    uint32_t start = kEditNone;   // bytes of the record in front of the match
    std::vector<uint32_t> runs;   // (length << 2) | op, from the pattern's first letter to its last
};

// The alignment that ends in cell (m, j) of the pattern against the record text[0 .. n), whose value the caller says is d.
// false: it is not (j > n, d > m, or the band's value there differs from d) — nothing can be said.
inline bool edit_align(const uint8_t* pattern, size_t m, const uint8_t* text, size_t n, uint32_t d, size_t j, const uint8_t* codes, EditAlignment& out) {
    if (m == 0 || j > n || d > m) return false;
    constexpr uint32_t kInf = 1u << 30;
    const size_t width = 2 * (size_t)d + 1;
    const int64_t base = (int64_t)j - (int64_t)m - (int64_t)d;  // the column of cell (i, k) is base + i + k
    std::vector<uint32_t> above(width + 1, kInf), row(width + 1, kInf);  // ([width]: the diagonal beyond the band)
    std::vector<uint8_t> ops((m * width + 3) / 4, 0);
    for (size_t k = 0; k < width; ++k) {
        const int64_t col = base + (int64_t)k;
        if (col >= 0 && col <= (int64_t)j) above[k] = 0;
    }
    for (size_t i = 1; i <= m; ++i) {
        const uint8_t pc = codes[pattern[i - 1]];
        for (size_t k = 0; k < width; ++k) {
            const int64_t col = base + (int64_t)i + (int64_t)k;
            uint32_t v = kInf, op = kEditOpInsert;
            if (col == 0) v = (uint32_t)i;  // D[i][0] = i, from D[i - 1][0]
            else if (col > 0 && col <= (int64_t)j) {
                const bool match = pc < 31 && pc == codes[text[col - 1]];
                const uint32_t diag = above[k] + (match ? 0u : 1u), up = above[k + 1] + 1, left = (k ? row[k - 1] : kInf) + 1;
                v = std::min(diag, std::min(up, left));
                op = diag == v ? (match ? kEditOpMatch : kEditOpMismatch) : up == v ? kEditOpInsert : kEditOpDelete;
            }
            row[k] = v;
            const size_t cell = (i - 1) * width + k;
            ops[cell >> 2] |= (uint8_t)(op << (2 * (cell & 3)));
        }
        above.swap(row);
        above[width] = kInf;
    }
    if (above[d] != d) return false;
    out.runs.clear();
    size_t i = m, k = d;
    while (i > 0) {
        if (k >= width) return false;  // (cannot happen where the band's value is d: the path stays inside)
        const size_t cell = (i - 1) * width + k;
        const uint32_t op = (ops[cell >> 2] >> (2 * (cell & 3))) & 3u;
        if (!out.runs.empty() && (out.runs.back() & 3u) == op) out.runs.back() += 4;
        else out.runs.push_back(4 | op);
        if (op == kEditOpDelete) --k;  // (k = 0 wraps and is caught above)
        else {
            --i;
            if (op == kEditOpInsert) ++k;
        }
    }
    const int64_t start = base + (int64_t)k;
    if (start < 0) return false;
    out.start = (uint32_t)start;
    std::reverse(out.runs.begin(), out.runs.end());
    return true;
}

// One pair in the layout of txq_edit_align_device: out[0 .. 2 max_errors + 3) from the search result (d, r, j) of the pattern
// against records [r0, r1).  A result that is "none" or the refusal marker is passed on as the device passes it on; start =
// kEditNotAligned (and nothing else written) where d > max_errors — the runs might not fit — or the triple is not a cell.
inline void edit_align_pair(const uint8_t* pattern, size_t m, const uint8_t* text, const uint64_t* rec, uint64_t r0, uint64_t r1, const uint32_t* result,
                            const uint8_t* codes, uint32_t max_errors, uint32_t* out) {
    const uint32_t d = result[0], r = result[1], j = result[2];
    const size_t run_words = 2 * (size_t)max_errors + 1;
    if (d == kEditNone) {
        out[0] = kEditNone;
        out[1] = r == kEditNotAligned ? kEditNotAligned : 0;
        std::fill(out + 2, out + 2 + run_words, 0u);
        return;
    }
    EditAlignment a;
    if (d > max_errors || r < r0 || r >= r1 || rec[r + 1] < rec[r] ||
        !edit_align(pattern, m, text + rec[r], (size_t)(rec[r + 1] - rec[r]), d, j, codes, a) || a.runs.size() > run_words) {
        out[0] = kEditNotAligned;
        return;
    }
    out[0] = a.start;
    out[1] = (uint32_t)a.runs.size();
    std::copy(a.runs.begin(), a.runs.end(), out + 2);
    std::fill(out + 2 + a.runs.size(), out + 2 + run_words, 0u);
}

}  // namespace tetrex
