// Host side: verification of candidate bins — product code, CPU/IO stage downstream of the GPU
// (SURVEY.md §8f item 1).  Mirrors the observable behaviour of the reference's
//   iter_disk_search          include/query.h:97-188
//   verify_fasta_hit          src/query.cpp:194-237   "binpath\t>name\tmatch\tstart,end"
//   reverse_verify_fasta_hit  src/query.cpp:167-191   "binpath\t>name\tmatch\tREVERSE STRAND HIT"
//   verify_reduced_fasta_hit  src/query.cpp:240-315   (sequence mapped through the reduction first)
//   verify_fasta_set          src/query.cpp:318-339   (-c conjunction)
// The reference matches with RE2 (absent here); this build has its own linear-time matcher (matcher.hpp):
// leftmost-longest for peptides (RE2::POSIX), leftmost-first for DNA (RE2 default syntax).
#pragma once
#include "encoder.hpp"

#include <ostream>
#include <string>
#include <unordered_map>
#include <vector>

namespace tetrex {

struct VerifyOptions {
    int threads = 1;
};

// comp_tab of src/query.cpp:7-16 restricted to the IUPAC letters: what the reverse strand's text is made with
inline char complement_base(char c) {
    switch (c) {
        case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; case 'U': return 'A';
        case 'a': return 't'; case 'c': return 'g'; case 'g': return 'c'; case 't': return 'a'; case 'u': return 'a';
        case 'M': return 'K'; case 'K': return 'M'; case 'R': return 'Y'; case 'Y': return 'R';
        case 'V': return 'B'; case 'B': return 'V'; case 'H': return 'D'; case 'D': return 'H';
        default: return c;
    }
}

// "Records to look at" (`tetrex query --gpu-verify`): for a (query, bin) pair the records of the bin — by
// their index in the file, ascending — in which the pattern matches somewhere, per strand (0 forward, 1 reverse complement;
// a reverse-strand record index is the record's index, not its position in reversed text).  Verification then runs find_all
// on those records only; a pair that is not listed is verified as without a selection.  A list may name a record without a
// match (find_all then reports none), never omit one with a match.
struct RecordSelection {
    struct Lists { std::vector<uint32_t> strand[2]; };
    std::unordered_map<uint64_t, Lists> pairs;  // key(query, bin)
    static uint64_t key(uint64_t query, uint64_t bin) { return query << 40 | bin; }
    const Lists* find(uint64_t query, uint64_t bin) const {
        const auto it = pairs.find(key(query, bin));
        return it == pairs.end() ? nullptr : &it->second;
    }
};

// Scan the FASTA files of `bins` for `regex`; rows go to `out` in bin order (DNA reverse-strand
// rows go to `reverse_out`, which the reference always sends to stdout).  Returns matches found.
size_t verify_bins(const std::vector<uint64_t>& bins, const std::vector<std::string>& bin_paths, const std::string& regex,
                   const KmerEncoder& enc, std::ostream& out, std::ostream& reverse_out, const VerifyOptions& opt,
                   const RecordSelection* selection = nullptr);  // selection: of query 0

// A batch of queries (-f), verified BIN-MAJOR: the reference verifies motif by motif (include/query.h:329-346 over
// :126-138), so a batch re-opens, re-inflates and re-parses a FASTA bin once per motif that selected it.  Here every
// candidate bin is read ONCE and all the motifs that selected it run over its records (OpenMP over the bins, like the
// reference's loop over one motif's bins); a thread keeps its lazily built automata from bin to bin.  masks[q] = the
// candidate-bin mask of query q (mask_words words; nullptr: the query is skipped).  forward[q] / reverse[q] receive exactly
// the rows verify_bins(set_bins(masks[q]), ...) writes to `out` / `reverse_out` — same bytes, same order, with or without a
// selection.
// Returns the matches found.
size_t verify_batch(const std::vector<const uint64_t*>& masks, uint64_t bins, const std::vector<std::string>& bin_paths,
                    const std::vector<std::string>& regexes, const KmerEncoder& enc, std::vector<std::string>* forward,
                    std::vector<std::string>* reverse, const VerifyOptions& opt, const RecordSelection* selection = nullptr);

// -c: records that match EVERY query
size_t verify_conjunction(const std::vector<uint64_t>& bins, const std::vector<std::string>& bin_paths,
                          const std::vector<std::string>& queries, std::ostream& out, const VerifyOptions& opt);

}  // namespace tetrex
