#include "encoder.hpp"

#include <stdexcept>

namespace tetrex {

namespace {
// residue -> 5-bit code, letters A..Z (include/peptide_decomposer.h:59-151)
constexpr uint8_t kBaseCodes[26] = {0, 2, 1, 2, 3, 4, 5, 6, 7, 9, 8, 9, 10, 11, 20, 12, 13, 14, 15, 16, 20, 17, 18, 20, 19, 3};
constexpr uint8_t kMurphyCodes[26] = {0, 1, 2, 1, 1, 3, 4, 5, 6, 6, 7, 6, 6, 1, 7, 8, 1, 7, 9, 9, 2, 6, 3, 9, 3, 1};
constexpr uint8_t kLiCodes[26] = {0, 1, 2, 1, 1, 3, 4, 5, 6, 7, 8, 7, 7, 5, 8, 9, 1, 8, 0, 0, 2, 6, 3, 0, 3, 1};
// residue -> representative letter of its reduced class, letters A..Z
// (include/peptide_decomposer.h:155-213; the non-Murphy branch is the Li table)
constexpr char kMurphyLetters[27] = "ABCBBFGHIIKIIBKPBKSSCIFSFB";
constexpr char kLiLetters[27] = "ABCBBFGHIJKJJHKPBKAACIFAFB";
}  // namespace

KmerEncoder::KmerEncoder(Molecule mol, unsigned k, Alphabet alphabet) : mol_(mol), alphabet_(alphabet), k_(k) {
    bits_ = mol == Molecule::DNA ? 2u : 5u;
    const unsigned total = bits_ * k_;
    kmer_mask_ = (k_ >= 32 || total >= 64) ? ~0ULL : ((1ULL << total) - 1ULL);
    const unsigned sfx = k_ ? bits_ * (k_ - 1) : 0;
    suffix_mask_ = sfx >= 64 ? ~0ULL : ((1ULL << sfx) - 1ULL);
    if (mol == Molecule::Peptide) {
        const uint8_t* codes = alphabet == Alphabet::Murphy ? kMurphyCodes : alphabet == Alphabet::Li ? kLiCodes : kBaseCodes;
        const char* letters = alphabet == Alphabet::Murphy ? kMurphyLetters : kLiLetters;
        for (int i = 0; i < 26; ++i) {
            aa_code_[(unsigned)('A' + i)] = codes[i];
            reduce_[(unsigned)('A' + i)] = letters[i];
        }
    }
}

uint64_t KmerEncoder::canonical(uint64_t forward) const {
    // reverse complement under A0 C1 T2 G3: complement = code ^ 2
    uint64_t rc = 0, f = forward;
    for (unsigned i = 0; i < k_; ++i) {
        rc = (rc << 2) | ((f & 3u) ^ 2u);
        f >>= 2;
    }
    return forward <= rc ? forward : rc;
}

void KmerEncoder::record_values(std::string_view seq, bool wraparound, std::vector<uint64_t>& out) const {
    if (seq.size() < k_ || k_ == 0) return;
    uint64_t fwd = 0;
    for (unsigned i = 0; i < k_; ++i) fwd = (fwd << bits_) | code((unsigned char)seq[i]);
    if (mol_ == Molecule::Peptide) {
        out.push_back(fwd);
        for (size_t i = k_; i < seq.size(); ++i) {
            fwd = ((fwd << 5) & kmer_mask_) | aa_code_[(unsigned char)seq[i]];
            out.push_back(fwd);
        }
        return;
    }
    out.push_back(canonical(fwd));
    for (size_t i = wraparound ? 0 : k_; i < seq.size(); ++i) {
        fwd = ((fwd << 2) & kmer_mask_) | (((unsigned char)seq[i] >> 1) & 3u);
        out.push_back(canonical(fwd));
    }
}

namespace {
// NCBI translation table 1, codon index 16 a + 4 b + c with T = 0, C = 1, A = 2, G = 3
constexpr char kTable1[65] = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";

unsigned nucleotide(unsigned char c) {
    switch (c) {
        case 'T': case 't': case 'U': case 'u': return 0;
        case 'C': case 'c': return 1;
        case 'A': case 'a': return 2;
        case 'G': case 'g': return 3;
        default: return 4;
    }
}
}  // namespace

std::string translate_frame(std::string_view seq, unsigned frame) {
    if (frame > 5) throw std::invalid_argument("frame must be 0..5");
    const size_t L = seq.size(), o = frame % 3;
    std::string out;
    // base i of the strand that is read: S[i], or the complement (code ^ 2) of S[L - 1 - i]; an ambiguous byte stays ambiguous
    auto base = [&](size_t i) {
        if (frame < 3) return nucleotide((unsigned char)seq[i]);
        const unsigned n = nucleotide((unsigned char)seq[L - 1 - i]);
        return n < 4 ? n ^ 2u : n;
    };
    for (size_t p = o; p + 3 <= L; p += 3) {
        const unsigned c[3] = {base(p), base(p + 1), base(p + 2)};
        out.push_back((c[0] | c[1] | c[2]) & 4u ? 'X' : kTable1[16 * c[0] + 4 * c[1] + c[2]]);
    }
    return out;
}

void translated_values(const KmerEncoder& enc, std::string_view seq, std::vector<uint64_t>& out, std::array<uint64_t, 7>& offsets) {
    if (enc.molecule() != Molecule::Peptide || enc.k() < 1 || enc.k() > 12)
        throw std::invalid_argument("translated k-mers need a peptide encoder with k in 1..12");
    const size_t start = out.size();
    offsets[0] = 0;
    for (unsigned f = 0; f < 6; ++f) {
        const std::string residues = translate_frame(seq, f);
        size_t a = 0;
        while (a <= residues.size()) {  // maximal stop-free runs
            size_t b = residues.find('*', a);
            if (b == std::string::npos) b = residues.size();
            enc.record_values(std::string_view(residues).substr(a, b - a), false, out);
            a = b + 1;
        }
        offsets[f + 1] = out.size() - start;
    }
}

}  // namespace tetrex
