// Host side: an index resident on the GPU, and its construction/query through the C-ABI
// (include/txq.h).  This is the host mirror of the reference's TetrexIndex façade for the
// query path: spawn_agent() -> upload, query() -> probe / run_programs
// (reference include/index_base.h:104-107,145-148).  Product code; requires a gfx950 GPU.
#pragma once
#include "compiler.hpp"
#include "device_buffer.hpp"  // (txq_check)
#include "encoder.hpp"
#include "index_file.hpp"
#include "layout.hpp"
#include "verify.hpp"
#include "../../../include/txq.h"
// (BinVerifier, BuildOptions / build_index and RecordFilter: whoever includes this file gets the whole host side)
#include "bin_verifier.hpp"
#include "index_build.hpp"
#include "record_filter.hpp"

#include <functional>
#include <string>
#include <vector>

namespace tetrex {

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
    // With `verified` (`--verify-frame-windows`) every hit is a candidate.  Behind the translation of a batch its
    // frames become letters on the device (txq_translate_frames_device on the same bytes) and txq_frame_window_letters_device
    // writes, per window, where its letters lie, its stops s and its threshold — not searched where s > edits, else
    // w - k (edits - s), not searched where that is not above 0 — straight into what the count takes; lens and stops come
    // back, thresholds[j] is that threshold (0: not searched) and threshold_of is not asked.  TETREX_FRAME_WINDOW_THRESHOLD=plain
    // (an A/B run): threshold_of as without `verified`, windows of any number of stops searched.  After the batch's counts its
    // hits go to BinVerifier::verify_windows with the letters where they are; confirmed[i] answers hits[i].
    struct VerifiedWindows {
        BinVerifier* verifier = nullptr;
        uint32_t edits = 0;
        std::vector<uint32_t> stops;         // out: the stops of every window
        std::vector<VerifiedHit> confirmed;  // out: confirmed[i] answers hits[i]
        // `--align-windows`, optional: called after the verification of every device batch with the batch's range
        // [h0, h1) of hits — whole records —, it returns the indexes of the confirmed hits to align; those get start and runs
        // (BinVerifier::align_windows) before the batch's letters are overwritten by the next one
        std::function<std::vector<size_t>(size_t, size_t)> select;
        // `--window-targets`: targets[i] receives every target of hits[i] (BinVerifier::verify_windows with rows) and
        // confirmed stays empty of answers; select_rows then takes select's place and returns (hit, row of its targets) pairs
        bool all_targets = false;
        std::vector<std::vector<VerifiedHit>> targets;
        std::function<std::vector<std::pair<size_t, size_t>>(size_t, size_t)> select_rows;
    };
    void search_translated_windows(std::string_view seq, const std::vector<uint64_t>& rec_offsets, uint32_t window, uint32_t step,
                                   const std::function<uint64_t(uint64_t)>& threshold_of, bool with_counts, std::vector<uint64_t>& win_offsets,
                                   std::vector<uint32_t>& lens, std::vector<uint32_t>& thresholds, std::vector<TranslatedHit>& hits,
                                   VerifiedWindows* verified = nullptr);
    // `tetrex query -g`: upload the d-gram index next to the main index (same device, same shard)
    void attach_dgram(const DgramImage& dgram);
    bool has_dgram() const { return aux_ != nullptr; }
    uint64_t dgram_min_gap() const { return dgram_min_; }
    uint64_t dgram_max_gap() const { return dgram_max_; }

  private:
    txq_index* upload_one(const IndexImage& image, int shard_rank, int n_shards);
    void release();  // frees every shard of the index and of the d-gram index
    std::vector<txq_index*> shards_;      // upload_sharded: all shards (shards_[0] == ix_); upload: just ix_
    std::vector<txq_index*> aux_shards_;  // the d-gram index, sharded the same way
    txq_index* ix_ = nullptr;
    txq_index* aux_ = nullptr;
    uint64_t dgram_min_ = 0, dgram_max_ = 0;
    int shard_rank_ = 0, n_shards_ = 1;
    txq_index_info info_{};
    KmerEncoder enc_;
};

// ascending ids of the set bits (compute_set_bins, reference src/query.cpp:40-75)
std::vector<uint64_t> set_bins(const uint64_t* mask, uint64_t bins);

}  // namespace tetrex
