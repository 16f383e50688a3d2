// Host side: an index resident on the GPU, and its construction/query through the C-ABI
// (include/txq.h).  This is the host mirror of the reference's TetrexIndex façade for the
// query path: spawn_agent() -> upload, query() -> probe / run_programs
// (reference include/index_base.h:104-107,145-148).  Product code; requires a gfx950 GPU.
#pragma once
#include "compiler.hpp"
#include "encoder.hpp"
#include "index_file.hpp"
#include "layout.hpp"
#include "verify.hpp"
#include "../../../include/txq.h"

#include <functional>
#include <string>
#include <vector>

namespace tetrex {

// Throws std::runtime_error carrying txq_last_error() when a txq call fails.
void txq_check(int rc, const char* what);

// StageExecutor over a txq session: slot masks stay in HBM between stages.
class TxqStageExecutor final : public StageExecutor {
  public:
    TxqStageExecutor(txq_index* ix, size_t n_programs, txq_index* aux = nullptr);
    ~TxqStageExecutor() override;
    void stage(const uint8_t* blob, size_t blob_bytes, const std::vector<uint32_t>& query_program,
               const std::vector<uint32_t>& query_slot, std::vector<uint8_t>& alive) override;
    // copies every program's RESULT mask (n_programs x shard_words words) and ends the session
    void finish(uint64_t* masks);

  private:
    txq_session* session_ = nullptr;
};

// StageExecutor over the column shards of one index, each with its own txq session (and, with several GPUs, its own
// device — include/txq.h txq_init).  ONE frontier expansion feeds all shards: a stage's blob goes to every session at the
// same time (one host thread per shard), and a waiting state counts as alive when any shard says so (the reference's
// path_.none() over the whole mask, include/otf_collector.h:383).  This is the seam of run_collection /
// run_multiple_queries (reference include/query.h:250-290,329-346) for a bin-sharded index.
class ShardedStageExecutor final : public StageExecutor {
  public:
    ShardedStageExecutor(const std::vector<txq_index*>& shards, size_t n_programs, const std::vector<txq_index*>& aux = {});
    ~ShardedStageExecutor() override;
    void stage(const uint8_t* blob, size_t blob_bytes, const std::vector<uint32_t>& query_program,
               const std::vector<uint32_t>& query_slot, std::vector<uint8_t>& alive) override;
    // ends the sessions and joins the shards' RESULT masks: n_programs x mask_words words
    std::vector<uint64_t> finish();

  private:
    std::vector<txq_session*> sessions_;
    std::vector<txq_index_info> info_;
    size_t n_programs_ = 0;
};

// Whole queries on an uploaded index: staged expansion + device execution.
std::vector<uint64_t> run_queries(txq_index* ix, const KmerEncoder& enc, const std::vector<std::string>& regexes,
                                  std::vector<int>* status, std::vector<std::string>* messages, StagedStats* stats,
                                  const StagedOptions* options, txq_index* aux = nullptr, uint64_t* into = nullptr);
// ... on all column shards of an index: full-width masks (n x mask_words)
std::vector<uint64_t> run_queries_sharded(const std::vector<txq_index*>& shards, const KmerEncoder& enc, const std::vector<std::string>& regexes,
                                          std::vector<int>* status, std::vector<std::string>* messages, StagedStats* stats,
                                          const StagedOptions* options, const std::vector<txq_index*>& aux = {});

// what BinVerifier (below) says about one candidate pair
struct VerifiedHit {
    uint32_t distance = 0xFFFFFFFFu;  // 0xFFFFFFFF: not within `errors` of any record of the bin
    uint32_t end = 0;                 // 1-based position of the match's last letter in the target, 0 for an empty match
    char strand = '+';                // '-': the reverse complement matched better (on equal distance + wins)
    const std::string* target = nullptr;  // the target record's name (valid as long as the verifier)
    // with BinVerifier::set_align (include/txq.h at txq_edit_align_device): the letters of the target in front of the match, and
    // the alignment's runs as (length << 2) | op, op 0 '=', 1 'X', 2 'I', 3 'D', from the pattern's first letter to its last
    uint32_t start = 0;
    std::vector<uint32_t> runs;
};
class BinVerifier;

class DeviceIndex {
  public:
    DeviceIndex() = default;
    DeviceIndex(const DeviceIndex&) = delete;
    DeviceIndex& operator=(const DeviceIndex&) = delete;
    ~DeviceIndex();

    // txq_init alone (HIP start-up costs ~0.5 s): `tetrex query` runs it on a helper thread while the index file is mapped and parsed
    static void warm_up(const std::vector<int>& devices);
    // txq_init + txq_index_upload of a parsed index file: ONE shard (shard_rank of n_shards) on one device
    void upload(const IndexImage& image, int device = 0, int shard_rank = 0, int n_shards = 1);
    // ... ALL n_shards column shards, dealt round-robin over `devices` (`tetrex query --gpus N`); queries then run on
    // every shard at once and query_masks returns full-width masks
    void upload_sharded(const IndexImage& image, const std::vector<int>& devices, int n_shards);
    size_t n_shards_held() const { return shards_.size(); }
    // words per mask that query_masks returns (the shard's words for upload(), the full mask for upload_sharded())
    uint64_t result_words() const { return shards_.size() > 1 ? info_.mask_words : info_.shard_words; }
    const txq_index_info& info() const { return info_; }
    KmerEncoder encoder() const { return enc_; }
    uint64_t bins() const { return info_.user_bins; }

    // candidate-bin masks for a batch of queries: n x shard_words words
    // status[i] != 0: query i could not be compiled (its mask is zero); messages[i] says why
    // Staged execution (compiler.hpp run_staged): the frontier is expanded on the host and
    // streamed to the device piecewise, with dead-state feedback between stages.
    std::vector<uint64_t> query_masks(const std::vector<std::string>& regexes, std::vector<int>* status = nullptr,
                                      std::vector<std::string>* messages = nullptr, StagedStats* stats = nullptr,
                                      const StagedOptions* options = nullptr);
    // threshold membership of value sets (txq_count, `tetrex search`) on the uploaded shard: query q owns
    // values[offsets[q] .. offsets[q+1]) and thresholds[q]; hits: n x result_words() words, counts (if not null):
    // n x 64 * result_words() u32.  One shard only (upload()).
    void count(const std::vector<uint64_t>& values, const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& thresholds,
               std::vector<uint64_t>& hits, std::vector<uint32_t>* counts);
    // `tetrex search --translate`: nucleotide records against this peptide index, all on the device.  Record r is
    // seq[rec_offsets[r] .. rec_offsets[r+1]); its six frames are queries 6 r + f (f = 0..5: +1 +2 +3 -1 -2 -3).  The bytes
    // are uploaded and translated there (txq_translate_device), n_of[q] comes back, thresholds[q] = threshold_of(n_of[q]) (0
    // where n_of[q] = 0), a query with threshold 0 is not searched, the others are counted (txq_count_device on the device's
    // values) and only the list of their hits comes back (txq_hit_list_device), in (query, bin) order.  Records are batched
    // by txq_translate_bound to at most 2^24 values a batch (one larger record: a batch of its own).  One shard only.
    // With a verifier (`--verify-frames`) every hit is a candidate: for a batch with at least one hit the
    // frames of its records become letters on the device (txq_translate_frames_device on the batch's bytes, which are still
    // there), the verifier compares frame `query` with bin `bin` by edit distance and confirmed[i] answers hits[i].
    // TETREX_VERIFY_FRAMES=host: the candidate frames are translated on the host (translate_frame) and verified as strings.
    // all_targets (`--all-targets`): all_targets->at(i) receives every target of hits[i]; confirmed[i] then says nothing.
    struct TranslatedHit { uint32_t query, bin, count; };  // count: 0 unless with_counts
    void search_translated(std::string_view seq, const std::vector<uint64_t>& rec_offsets,
                           const std::function<uint64_t(uint64_t)>& threshold_of, bool with_counts, std::vector<uint64_t>& n_of,
                           std::vector<uint64_t>& thresholds, std::vector<TranslatedHit>& hits, BinVerifier* verifier = nullptr,
                           std::vector<VerifiedHit>* confirmed = nullptr, std::vector<std::vector<VerifiedHit>>* all_targets = nullptr);
    // `tetrex search --window`: sliding windows over one value array.  Window j owns
    // values[begins[j] .. begins[j] + lens[j]) and thresholds[j]; begins and begins + lens do not decrease.  A window with
    // threshold 0 is not searched and has no hits.  Windows go to the device in batches that end at a window boundary: at most
    // 2^24 values (the values a batch's last windows share with the next batch's first are sent again), at most 256 MiB of hit
    // words / counts, and at most TETREX_SEARCH_BATCH_WINDOWS windows where that is set (for tests: the hits are the same for
    // every value).  The hit and count matrices stay on the device (txq_count_windows_device); only the list of
    // (window, bin, count) comes back (txq_hit_list_device), in (window, bin) order.  One shard only.
    void search_windows(const std::vector<uint64_t>& values, const std::vector<uint64_t>& begins, const std::vector<uint32_t>& lens,
                        const std::vector<uint32_t>& thresholds, bool with_counts, std::vector<TranslatedHit>& hits);
    // `tetrex search --translate --frame-window`: the six frames of nucleotide records cut into windows of
    // `window` residues, `step` apart, all on the device.  Record r is seq[rec_offsets[r] .. rec_offsets[r+1]); the windows of
    // its frame f are win_offsets[6 r + f] .. win_offsets[6 r + f + 1] (csrc/txq_frame_windows_plan.hpp gives window j's
    // residues).  Records are batched as search_translated batches them; a batch is uploaded and one
    // txq_translate_windows_device call leaves its values and window arrays on the device.  lens[j] — the window's stop-free
    // k-mers — comes back, thresholds[j] = threshold_of(lens[j]) (0 where lens[j] = 0), a window with threshold 0 is not
    // searched, and the others are counted by sliding (txq_count_windows_device) over sub-ranges of the batch's windows: at
    // most 256 MiB of hit words / counts, and TETREX_SEARCH_BATCH_WINDOWS windows where set (for tests: the hits are the same
    // for every value).  No value is sent twice.  Only the list of (window, bin, count) comes back, in (window, bin) order.
    // One shard only; flat and hierarchical indexes alike.
    void search_translated_windows(std::string_view seq, const std::vector<uint64_t>& rec_offsets, uint32_t window, uint32_t step,
                                   const std::function<uint64_t(uint64_t)>& threshold_of, bool with_counts, std::vector<uint64_t>& win_offsets,
                                   std::vector<uint32_t>& lens, std::vector<uint32_t>& thresholds, std::vector<TranslatedHit>& hits);
    // `tetrex query -g`: upload the d-gram index next to the main index (same device, same shard)
    void attach_dgram(const DgramImage& dgram);
    bool has_dgram() const { return aux_ != nullptr; }
    uint64_t dgram_min_gap() const { return dgram_min_; }
    uint64_t dgram_max_gap() const { return dgram_max_; }

  private:
    txq_index* upload_one(const IndexImage& image, int shard_rank, int n_shards);
    std::vector<txq_index*> shards_;      // upload_sharded: all shards (shards_[0] == ix_); upload: just ix_
    std::vector<txq_index*> aux_shards_;  // the d-gram index, sharded the same way
    txq_index* ix_ = nullptr;
    txq_index* aux_ = nullptr;
    uint64_t dgram_min_ = 0, dgram_max_ = 0;
    int shard_rank_ = 0, n_shards_ = 1;
    txq_index_info info_{};
    KmerEncoder enc_;
};

// The records of bins' FASTA files, resident on the device: what `tetrex search --verify` and `tetrex query --gpu-verify` run
// their kernels over.  A bin's file (plain or gzip) is read when it is first asked for; its records go to the device once —
// the bytes back to back, their n + 1 offsets, and behind those the offsets {0, n} of the one group they form — and stay
// there, at most TETREX_VERIFY_TEXT_MB MiB of them (default 4096; the bin used longest ago leaves first; a fraction is
// allowed).  Needs txq_init (DeviceIndex::upload).
class ResidentBins {
  public:
    // `who` begins the message of the std::runtime_error that names a bin file which cannot be read
    ResidentBins(const std::vector<std::string>& bin_paths, std::string who);
    ResidentBins(const ResidentBins&) = delete;
    ResidentBins& operator=(const ResidentBins&) = delete;
    ~ResidentBins();
    struct Bin {
        std::vector<std::string> names;  // kept once read
        void* d_text = nullptr;          // device: the records back to back, their n + 1 offsets, and {0, n}
        void* d_rec = nullptr;
        uint64_t n_records = 0, text_bytes = 0, device_bytes = 0, last_use = 0;
    };
    // the bin's records as the device gets them (rec: n + 1 offsets)
    void read(uint32_t bin, std::string& text, std::vector<uint64_t>& rec, std::vector<std::string>& names) const;
    Bin& resident(uint32_t bin);  // reads and uploads the bin unless it is on the device
    // the same with the file already read (text, rec, names as read() gives them; names are moved from)
    Bin& resident(uint32_t bin, const std::string& text, std::vector<uint64_t>& rec, std::vector<std::string>& names);
    bool is_resident(uint32_t bin) const { return bins_[bin].d_rec != nullptr; }
    Bin& at(uint32_t bin) { return bins_[bin]; }
    size_t size() const { return bins_.size(); }

  private:
    void drop(Bin& b);
    const std::vector<std::string>& paths_;
    std::string who_;
    std::vector<Bin> bins_;
    uint64_t limit_bytes_, held_bytes_ = 0, clock_ = 0;
};

// `tetrex search --verify`: candidate (record, bin) pairs confirmed by edit distance on the bins' raw letters
// (txq_edit_search_device, include/txq.h, where the semantics are).  Comparison is case-insensitive whatever reduction the
// index uses: on a peptide index every letter is a class of its own, on a nucleotide index A, C, G and T = U are, every
// other byte matches nothing; a nucleotide record is tried on both strands (its reverse complement is a second pattern, in
// which an ambiguous byte stays one).  A bin's FASTA is read when it is first a candidate and its records stay on the device
// (ResidentBins).  Records of up to TXQ_EDIT_MAX_PATTERN letters go to txq_edit_search_device, those of up to
// TXQ_EDIT_LONG_MAX_PATTERN to txq_edit_search_long_device (TETREX_VERIFY_LONG=0: to the host, as before that kernel
// existed), one call per candidate bin each, all queued before the one copy back.  Longer records and empty ones are
// answered on the host (host/edit_distance.hpp), with OpenMP over the pairs.  n_routed() counts the candidate pairs each of
// the three routes answered.
// set_align (`--align`): every confirmed pair also gets the start and the runs of its alignment.  Behind each
// search call txq_edit_align_device is queued on the same stream, reading the triples where the search call left them, and its
// answers come back in the verifier's one copy; a pair the device declines (more than TXQ_EDIT_ALIGN_MAX_DISTANCE edits), a pair
// of the host route, and with TETREX_VERIFY_ALIGN=host every pair, is aligned by edit_align of host/edit_distance.hpp on the
// bin's letters read once more.  n_aligned() counts the pairs each of the two routes aligned.  Needs txq_init (DeviceIndex::upload).
// `--all-targets` (verify with `rows`): every record of the bin within E edits is a row of its pair, in the
// order of the bin's file — on a nucleotide index a target's better strand, + on equal distance.  The routes are the same,
// with txq_edit_targets_device / txq_edit_targets_long_device in place of the search calls and edit_targets_group on the host.
// A call's slots — its pairs times the bin's records — are bounded by TETREX_VERIFY_TARGET_SLOTS (default 2^20): a bin
// whose pairs need more is answered in several calls, a bin with more records than that on the host, and the calls are
// queued in rounds of at most eight times that many slots; a round waits once, for its totals, and copies its rows back — the
// whole row area in one copy where that is at most 4 MiB, else only the rows written, call by call.  TETREX_VERIFY_TARGETS=host sends every pair
// to the host.  With set_align the rows that were kept are aligned by one txq_edit_align_device call per bin on pair and triple
// arrays built after the copy back (one more round trip a batch), the rest on the host as above.
class BinVerifier {
  public:
    BinVerifier(const std::vector<std::string>& bin_paths, bool dna, uint32_t errors);
    BinVerifier(const BinVerifier&) = delete;
    BinVerifier& operator=(const BinVerifier&) = delete;
    ~BinVerifier();
    struct Candidate { uint32_t query, bin; };
    using Hit = VerifiedHit;
    // hits[i] answers candidates[i]; queries[c.query] are the batch's records.  Throws std::runtime_error naming the bin file
    // that cannot be read.
    // rows (`--all-targets`, below): rows->at(i) receives every target of candidates[i] instead, and hits stays as assign() left it.
    void verify(const std::vector<std::string>& queries, const std::vector<Candidate>& candidates, std::vector<Hit>& hits,
                std::vector<std::vector<Hit>>* rows = nullptr);
    // The same for patterns that are on the device already (`tetrex search --translate --verify-frames`, DESIGN.md §14: the
    // frames of txq_translate_frames_device).  Pattern p is d_letters[d_offsets[p] .. d_offsets[p+1]), n_patterns + 1 offsets,
    // `bytes` letters in all in a buffer with 16 bytes of slack behind them; candidates[i].query names a pattern,
    // lengths[i] is its length, and letters(p) gives the pattern to the host route (longer than TXQ_EDIT_LONG_MAX_PATTERN).
    // One strand: a pattern is compared as it stands, whatever the index's molecule.
    struct DevicePatterns {
        const uint8_t* d_letters;
        const uint64_t* d_offsets;
        size_t n_patterns, bytes;
    };
    void verify(const DevicePatterns& patterns, const std::vector<Candidate>& candidates, const std::vector<uint64_t>& lengths,
                const std::function<std::string(uint32_t)>& letters, std::vector<Hit>& hits, std::vector<std::vector<Hit>>* rows = nullptr);
    size_t n_candidates() const { return n_candidates_; }
    size_t n_confirmed() const { return n_confirmed_; }
    size_t n_targets() const { return n_targets_; }  // `--all-targets`: the rows of all confirmed pairs
    struct Routed { size_t device, device_long, host; };
    Routed n_routed() const { return {n_device_, n_device_long_, n_host_}; }
    void set_align(bool on) { align_ = on; }
    struct Aligned { size_t device, host; };
    Aligned n_aligned() const { return {n_align_device_, n_align_host_}; }

  private:
    // what both entries share: candidate i compares `strands` consecutive patterns from pattern_of[i] (lengths[i] letters each)
    // with its bin — routing by length, the pairs, one call per bin and kernel, the one copy back, the host route, settle
    void run(const DevicePatterns& patterns, size_t strands, const std::vector<Candidate>& candidates, const std::vector<uint32_t>& pattern_of,
             const std::vector<uint64_t>& lengths, const std::function<std::string(size_t, size_t)>& letters, std::vector<Hit>& hits,
             std::vector<std::vector<Hit>>* rows);
    // `--all-targets`: the same routing with txq_edit_targets*_device and edit_targets_group in place of the search calls
    void run_targets(const DevicePatterns& patterns, size_t strands, const std::vector<Candidate>& candidates, const std::vector<uint32_t>& pattern_of,
                     const std::vector<uint64_t>& lengths, const std::function<std::string(size_t, size_t)>& letters,
                     std::vector<std::vector<Hit>>& rows);
    static size_t device_max();  // the longest pattern the device answers (TETREX_VERIFY_LONG)
    ResidentBins bins_;
    bool dna_;
    uint32_t errors_;
    uint8_t codes_[256];
    void* d_codes_ = nullptr;
    size_t n_candidates_ = 0, n_confirmed_ = 0, n_device_ = 0, n_device_long_ = 0, n_host_ = 0;
    bool align_ = false;
    size_t n_align_device_ = 0, n_align_host_ = 0;
    size_t n_targets_ = 0;
};

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

// ascending ids of the set bits (compute_set_bins, reference src/query.cpp:40-75)
std::vector<uint64_t> set_bins(const uint64_t* mask, uint64_t bins);

struct BuildOptions {
    unsigned k = 6;
    float fpr = 0.05f;
    unsigned hash_count = 3;
    bool dna = false;
    bool hibf = true;       // the reference's default flavour
    unsigned reduction = 0; // 0 None, 1 murphy, 2 li
    bool dna_wraparound = true;  // reproduce include/nucleotide_decomposer.h:106-110
    int device = 0;
    // HIBF layout: kUniform, this project's two-level tree (the default); kSized, host/layout.hpp with t_max = tmax
    // (0: default_tmax(B)), built by the kernels of txq_build.hip
    enum Layout { kUniform = 0, kSized = 1 };
    int layout = kUniform;
    uint64_t tmax = 0;
    // kSized only: before the layout, chain similar bins inside intervals of the sorted order (host/layout.hpp
    // rearrange_intervals / rearrange_chain, txq_pair_unions_device).  0: off; else the interval ratio in (0, 1].
    double rearrange_ratio = 0;
};
// `tetrex index`: FASTA files -> index image, bits set on the GPU (txq_emplace_device).
IndexImage build_index(const std::vector<std::string>& bin_files, const BuildOptions& opt, size_t* n_sequences = nullptr);
// `tetrex track`: FASTA files -> d-gram index (reference src/dGramIndex.cpp:22-38, include/dGramIndex.h:105-157)
DgramImage build_dgram_index(const std::vector<std::string>& bin_files, uint64_t min_gap, uint64_t max_gap, unsigned hash_count,
                             float fpr, int device = 0);

}  // namespace tetrex
