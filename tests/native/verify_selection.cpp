// Verification with "records to look at" against verification without (host/verify.hpp RecordSelection; `tetrex query
// --gpu-verify`) — native, no GPU:
//   verify_selection <dna 0|1> <reduction 0|1|2> <threads> <motifs file: one per line> <fasta files...>
// Every motif selects every bin.  The selection is made the way RecordFilter makes it, with the host's interpreter in the
// kernel's place: the motif exported as an automaton (both strands on a nucleotide library, the reduction or the complement
// folded in), run over the raw records of each bin.  The last motif gets no selection (the "too large" path) and every
// seventh pair none either (a refused pair).  verify_batch and verify_bins must write the same bytes with and without it.
//   g++ -std=c++20 -O1 -g -fsanitize=address,undefined -fopenmp tests/native/verify_selection.cpp tetrex_amd/csrc/host/{verify,fasta,matcher,
//       encoder,regex_front}.cpp -lz -o verify_selection
// Prints "verify_selection ok: <rows> rows, <listed> of <records> records listed" and exits 0, or says what differs and exits 1.
#include "../../include/txq_regex.h"
#include "../../tetrex_amd/csrc/host/fasta.hpp"
#include "../../tetrex_amd/csrc/host/matcher.hpp"
#include "../../tetrex_amd/csrc/host/regex_front.hpp"
#include "../../tetrex_amd/csrc/host/verify.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

using namespace tetrex;

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    const bool dna = std::atoi(argv[1]) != 0;
    const unsigned reduction = (unsigned)std::atoi(argv[2]);
    const VerifyOptions opt{std::atoi(argv[3])};
    std::vector<std::string> motifs, paths;
    {
        std::ifstream in(argv[4]);
        for (std::string line; std::getline(in, line);)
            if (!line.empty()) motifs.push_back(line);
    }
    for (int i = 5; i < argc; ++i) paths.push_back(argv[i]);
    const KmerEncoder enc(dna ? Molecule::DNA : Molecule::Peptide, 3, (Alphabet)reduction);
    const bool reduced = !dna && reduction != 0;
    const uint64_t bins = paths.size();
    std::vector<uint64_t> all((bins + 63) / 64, ~0ULL);
    std::vector<const uint64_t*> masks(motifs.size(), all.data());

    uint8_t fwd_map[256], rev_map[256];
    for (unsigned b = 0; b < 256; ++b) {
        fwd_map[b] = reduced ? (uint8_t)enc.reduce((unsigned char)b) : (uint8_t)b;
        rev_map[b] = (uint8_t)complement_base((char)b);
    }
    RecordSelection sel;
    size_t listed = 0, records = 0, pair = 0;
    for (size_t q = 0; q + 1 < motifs.size(); ++q) {
        std::string pattern = motifs[q];
        if (reduced) pattern = reduce_query_alphabet(pattern, enc.reduce_table());
        const Matcher m("(" + pattern + ")", dna ? Matcher::Semantics::LeftmostFirst : Matcher::Semantics::LeftmostLongest);
        std::vector<uint8_t> blob[2];
        if (!m.export_dfa(false, fwd_map, blob[0]) || (dna && !m.export_dfa(true, rev_map, blob[1]))) continue;
        for (uint64_t b = 0; b < bins; ++b) {
            if (++pair % 7 == 0) continue;
            RecordSelection::Lists& l = sel.pairs[RecordSelection::key(q, b)];
            uint32_t r = 0;
            for_each_record(paths[b], [&](const FastaRecord& rec) {
                for (int s = 0; s < (dna ? 2 : 1); ++s) {
                    ++records;
                    if (txq_regex_record_matches(blob[s].data(), (const uint8_t*)rec.seq.data(), rec.seq.size())) { l.strand[s].push_back(r); ++listed; }
                }
                ++r;
            });
        }
    }
    std::vector<std::string> f0, r0, f1, r1;
    const size_t n0 = verify_batch(masks, bins, paths, motifs, enc, &f0, &r0, opt);
    const size_t n1 = verify_batch(masks, bins, paths, motifs, enc, &f1, &r1, opt, &sel);
    if (n0 != n1 || f0 != f1 || r0 != r1) {
        for (size_t q = 0; q < motifs.size(); ++q)
            if (f0[q] != f1[q] || r0[q] != r1[q]) std::printf("verify_batch differs for motif %zu %s: %zu / %zu forward bytes, %zu / %zu reverse bytes\n", q, motifs[q].c_str(), f0[q].size(), f1[q].size(), r0[q].size(), r1[q].size());
        return 1;
    }
    // the single-query path: verify_bins reads the selection of query 0
    std::vector<uint64_t> every(bins);
    for (uint64_t b = 0; b < bins; ++b) every[b] = b;
    for (size_t q = 0; q < motifs.size(); ++q) {
        RecordSelection one;
        for (uint64_t b = 0; b < bins; ++b)
            if (const RecordSelection::Lists* l = sel.find(q, b)) one.pairs[RecordSelection::key(0, b)] = *l;
        std::ostringstream a, ar, c, cr;
        const size_t m0 = verify_bins(every, paths, motifs[q], enc, a, ar, opt);
        const size_t m1 = verify_bins(every, paths, motifs[q], enc, c, cr, opt, &one);
        if (m0 != m1 || a.str() != c.str() || ar.str() != cr.str() || a.str() != f0[q] || ar.str() != r0[q]) {
            std::printf("verify_bins differs for motif %zu %s\n", q, motifs[q].c_str());
            return 1;
        }
    }
    std::printf("verify_selection ok: %zu rows, %zu of %zu records listed\n", n0, listed, records);
    return 0;
}
