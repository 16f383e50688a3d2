// Host side: approximate matching of a pattern against the records of a bin by edit distance (`tetrex search --verify`,
// DESIGN.md §12; the semantics are spelled out in include/txq.h at txq_edit_search_device).  Myers' bit-parallel form of
// Sellers' recurrence with the pattern as ONE integer of ceil(m / 64) words: the addition carries and the shifts run over
// all words, so there is no limit on m.  This is the host twin of the kernel in txq_edit.hip: it answers patterns longer
// than TXQ_EDIT_MAX_PATTERN and it is what the kernel is measured against.  Header only, no dependencies.
#pragma once
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

}  // namespace tetrex
