// Host side: `tetrex query --gpu-verify`, the record filter in front of verification, through the C-ABI (include/txq.h,
// include/txq_regex.h).  Product code; requires a gfx950 GPU.
#pragma once
#include "bin_verifier.hpp"
#include "encoder.hpp"
#include "verify.hpp"

#include <string>
#include <vector>

namespace tetrex {

// `tetrex query --gpu-verify`: which records of its candidate bins does a motif match at all?  Answered on the
// device (txq_regex_filter_device, include/txq.h) for a batch of motifs and their candidate masks, so that verification runs
// the matcher's find_all on those records only.  Each motif is exported once as an automaton (Matcher::export_dfa: the pattern
// as verification hands it to the matcher, the index's reduction folded into the class table; on a nucleotide index a second
// automaton for the reverse strand, the complement folded in), candidate bins become resident (ResidentBins), one filter call
// per bin is queued and the bitmaps come back once per block of bins.  A motif whose automaton is too large, and a pair the
// device refused, are not in the selection: verification takes them the way it does without the flag.  Needs txq_init.
class RecordFilter {
  public:
    RecordFilter(const std::vector<std::string>& bin_paths, const KmerEncoder& enc, int threads);
    struct Stats {
        uint64_t pairs_device = 0, pairs_host = 0;         // (motif, bin) pairs answered by the device / left to the host
        uint64_t records_flagged = 0, records_total = 0;   // over the device's pairs and strands
        uint64_t automata_lds = 0, automata_l2 = 0, automata_host = 0;  // automata by table tier; motifs too large to export
        double export_seconds = 0, upload_seconds = 0, filter_seconds = 0, copy_seconds = 0;
    };
    // masks[q]: the candidate-bin mask of motif q (nullptr: skipped); the selection receives every pair the device answered
    void run(const std::vector<const uint64_t*>& masks, uint64_t bins, const std::vector<std::string>& regexes, RecordSelection& out);
    const Stats& stats() const { return stats_; }

  private:
    ResidentBins bins_;
    KmerEncoder enc_;
    int threads_;
    Stats stats_;
};

}  // namespace tetrex
