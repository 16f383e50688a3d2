// Host side: the records of bins' FASTA files resident on the GPU, and `tetrex search --verify` on them through the C-ABI
// (include/txq.h).  Product code; requires a gfx950 GPU.
#pragma once
#include "device_buffer.hpp"

#include <cstdint>
#include <functional>
#include <string>
#include <vector>

namespace tetrex {

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
    // the same for a host route: the names stay with the bin unless it has them (they are the same, and hits point into them)
    void read_keeping_names(uint32_t bin, std::string& text, std::vector<uint64_t>& rec);
    Bin& resident(uint32_t bin);  // reads and uploads the bin unless it is on the device
    // the same with the file already read (text, rec, names as read() gives them; names are moved from)
    Bin& resident(uint32_t bin, const std::string& text, std::vector<uint64_t>& rec, std::vector<std::string>& names);
    bool is_resident(uint32_t bin) const { return bins_[bin].d_rec != nullptr; }
    // the device bytes of a bin of n_records records in text_bytes letters, and the most the cache holds (TETREX_VERIFY_TEXT_MB):
    // what a caller needs to plan several bins that must be resident TOGETHER (BinVerifier::align_windows)
    static uint64_t bytes_on_device(uint64_t text_bytes, uint64_t n_records) { return text_bytes + 16 + (n_records + 3) * 8; }
    uint64_t limit_bytes() const { return limit_bytes_; }
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
// `--window --verify-windows` (verify_windows): the patterns are windows of the batch's records.  The letters of
// the records that have a candidate go up once — on a nucleotide index each record's reverse complement behind it, window
// [a, a + l) on strand - being [L - a - l, L - a) of it —, the windows as (begin, length) into them, and the candidates, by bin
// and by window within the bin so that consecutive windows of a record are neighbours, go to txq_edit_windows_device: one
// call per candidate bin on its resident text, all queued before the one copy back; strands are settled as above.  Windows of
// more than TXQ_EDIT_MAX_PATTERN letters, and with TETREX_VERIFY_WINDOWS=written every window, are written out as strings and
// take verify() with its three routes.
// `--align-windows` (align_windows): start and runs of the windows the caller selects after its run merge — one
// per row.  set_align stays off: nothing is aligned during verification.  After keep_windows(true) verify_windows keeps its
// letter and window buffers (and the way to a window's string) until its next call; align_windows cuts the selection into rounds of bins that fit
// TETREX_VERIFY_TEXT_MB together (one bin is always a round), makes a round's bins resident, uploads a table of their views,
// the pairs and the triples, queues ONE txq_edit_align_windows_device and copies back once.  What that call declines (more than
// TXQ_EDIT_ALIGN_MAX_DISTANCE edits), windows that did not take the window kernel (longer than TXQ_EDIT_MAX_PATTERN, the
// `written` routes), a round whose bins did not all stay resident, and with TETREX_VERIFY_ALIGN=host every pair, go to the host
// twin as above.
// `--window-targets` (verify_windows with `rows`): every record of the bin within E edits of a window is a row of
// its candidate, in the order of the bin's file — on a nucleotide index a target's better strand, + on equal distance.  The
// candidates, by bin and by window within the bin, are cut into rounds: a round is a maximal prefix whose bins fit
// TETREX_VERIFY_TEXT_MB together (one bin is always a round) and whose slots — the sum over its pairs of the records of their
// bins — are at most eight times TETREX_VERIFY_TARGET_SLOTS.  A round's bins are made resident, a table of their views and the
// pairs go up (the letters went up once per batch, or are the caller's), ONE txq_edit_window_targets_device is queued over all
// the round's bins, the round waits once, for the total, and copies back the rows written.  Through verify() with rows — the
// windows written out as strings, run_targets and its routes — go: windows of more than TXQ_EDIT_MAX_PATTERN letters, a bin with
// more records than TETREX_VERIFY_TARGET_SLOTS, a round whose bins did not all stay resident, and with
// TETREX_VERIFY_WINDOWS=written / TETREX_VERIFY_FRAME_WINDOWS=written or TETREX_VERIFY_TARGETS=host every candidate.  The rows are
// the same on every route; align_windows takes a selected row as it takes a hit (its target points into the bin's names).
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
    // `--verify-windows`: window w is letters [begin, begin + len) of queries[record]; candidates[i].query names a window.
    struct Window {
        uint32_t record;
        uint64_t begin;
        uint32_t len;
    };
    // rows (`--window-targets`, below): rows->at(i) receives every target of candidates[i] instead, and hits stays as assign() left it.
    void verify_windows(const std::vector<std::string>& queries, const std::vector<Window>& windows, const std::vector<Candidate>& candidates,
                        std::vector<Hit>& hits, std::vector<std::vector<Hit>>* rows = nullptr);
    // `--translate --frame-window --verify-frame-windows`: the windows' letters are on the device already — the
    // frames of txq_translate_frames_device, `bytes` of them with 16 bytes of slack behind, window w being
    // d_letters[d_begin[w] .. d_begin[w] + d_len[w]) as txq_frame_window_letters_device left them.  candidates[i].query names a
    // window, lengths[i] is its length, letters(w) gives the window as a string to verify()'s routes: windows of more than
    // TXQ_EDIT_MAX_PATTERN residues, and with TETREX_VERIFY_FRAME_WINDOWS=written every window.  One strand: the frame fixes it
    // (a verifier made for a nucleotide index is refused).  The others go to txq_edit_windows_device grouped, ordered and
    // queued exactly as above — by bin and by window within the bin, one call per candidate bin, all queued before the one
    // copy back — and count towards n_routed().windows.
    struct DeviceWindows {
        const uint8_t* d_letters;
        size_t bytes;
        const uint64_t* d_begin;
        const uint32_t* d_len;
        size_t n_windows;
    };
    void verify_windows(const DeviceWindows& windows, const std::vector<Candidate>& candidates, const std::vector<uint32_t>& lengths,
                        const std::function<std::string(uint32_t)>& letters, std::vector<Hit>& hits, std::vector<std::vector<Hit>>* rows = nullptr);
    // `--align-windows`: selection[k] names a candidate of the LAST verify_windows call (either form) and the confirmed hit that
    // answers it; the hit gets start and runs (include/txq.h at txq_edit_align_windows_device).  `candidates` are that call's,
    // and what it was given — queries and windows, or the device buffers and `letters` — must still be there.
    struct Selected {
        size_t candidate;
        Hit* hit;
    };
    // (asked for before verify_windows: its first form then keeps its device buffers instead of freeing them on return)
    void keep_windows(bool on) { keep_windows_ = on; }
    void align_windows(const std::vector<Candidate>& candidates, const std::vector<Selected>& selection);
    size_t n_align_windows_calls() const { return n_align_windows_calls_; }  // txq_edit_align_windows_device calls
    size_t n_candidates() const { return n_candidates_; }
    size_t n_confirmed() const { return n_confirmed_; }
    size_t n_targets() const { return n_targets_; }  // `--all-targets`, `--window-targets`: the rows of all confirmed pairs
    // `--window-targets`: the candidates txq_edit_window_targets_device answered, those that took verify()'s routes, and the calls
    struct WindowTargets { size_t device, host, calls; };
    WindowTargets n_window_targets() const { return {n_wt_device_, n_wt_host_, n_wt_calls_}; }
    struct Routed { size_t device, device_long, host, windows; };  // (windows: txq_edit_windows_device)
    Routed n_routed() const { return {n_device_, n_device_long_, n_host_, n_windows_}; }
    void set_align(bool on) { align_ = on; }
    struct Aligned { size_t device, host; };
    Aligned n_aligned() const { return {n_align_device_, n_align_host_}; }

  private:
    using Letters = std::function<std::string(size_t, size_t)>;  // (candidate, strand) -> the pattern, for the host routes
    // what both entries share: candidate i compares `strands` consecutive patterns from pattern_of[i] (lengths[i] letters each)
    // with its bin — routing by length, the pairs, one call per bin and kernel, the one copy back, the host route, settle
    void run(const DevicePatterns& patterns, size_t strands, const std::vector<Candidate>& candidates, const std::vector<uint32_t>& pattern_of,
             const std::vector<uint64_t>& lengths, const Letters& letters, std::vector<Hit>& hits, std::vector<std::vector<Hit>>* rows);
    // what both verify_windows share: the candidates on_kernel, by bin and by window, as `strands` consecutive entries from
    // entry_of(candidate) of window arrays on the device — the pairs, one txq_edit_windows_device call per bin, the one copy
    // back, the better strand (+ on equal distance)
    void run_windows(const DeviceWindows& w, size_t strands, const std::vector<size_t>& on_kernel, const std::function<uint32_t(size_t)>& entry_of,
                     const std::vector<Candidate>& candidates, std::vector<Hit>& hits);
    // `--window-targets`: every target of the candidates on_kernel (by bin and by window), as `strands` consecutive entries from
    // entry_of(candidate) of window arrays on the device — rounds, ONE txq_edit_window_targets_device call each, the better strand
    // per target; what a round cannot answer goes to written_window_targets
    void run_window_targets(const DeviceWindows& w, size_t strands, const std::vector<size_t>& on_kernel, const std::function<uint32_t(size_t)>& entry_of,
                            const std::vector<Candidate>& candidates, size_t n_windows, const std::function<std::string(uint32_t)>& window_string,
                            std::vector<std::vector<Hit>>& rows);
    // the candidates `which` with their windows written out as strings (window_string(window), asked in ascending order): verify()
    // with rows, so run_targets and its three routes
    void written_window_targets(const std::vector<size_t>& which, size_t n_windows, const std::vector<Candidate>& candidates,
                                const std::function<std::string(uint32_t)>& window_string, std::vector<std::vector<Hit>>& rows);
    // `--all-targets`: the same routing with txq_edit_targets*_device and edit_targets_group in place of the search calls
    void run_targets(const DevicePatterns& patterns, size_t strands, const std::vector<Candidate>& candidates, const std::vector<uint32_t>& pattern_of,
                     const std::vector<uint64_t>& lengths, const Letters& letters, std::vector<std::vector<Hit>>& rows);
    // The candidates by bin (`order`), and by route: on_device holds the n_short patterns of up to TXQ_EDIT_MAX_PATTERN letters
    // and behind them those of up to device_max(), which the long-pattern kernels answer; on_host the empty and the longer
    // ones, and with all_on_host every one.
    struct Routes {
        std::vector<size_t> order, on_device, on_host;
        size_t n_short = 0;
    };
    Routes split_routes(const std::vector<Candidate>& candidates, const std::vector<uint64_t>& lengths, bool all_on_host) const;
    static size_t device_max();  // the longest pattern the device answers (TETREX_VERIFY_LONG)
    // --align: on the device unless TETREX_VERIFY_ALIGN=host says otherwise, there with at most device_errors edits (the device
    // declines more anyway) in `stride` words a pair
    struct AlignRoute {
        bool on_device;
        uint32_t device_errors;
        size_t stride;
    };
    AlignRoute align_route() const;
    // a confirmed pair the host aligns: distance d, record r of the bin, end j; the answer goes to *into
    struct PendingAlign {
        size_t candidate, strand;
        uint32_t d, r, j;
        Hit* into;
    };
    // n pairs of one bin on its letters, side by side; throws after all of them where one has no alignment
    void align_on_host(uint32_t bin, const PendingAlign* pairs, size_t n, const std::string& text, const std::vector<uint64_t>& rec, const Letters& letters);
    // alignments the device did not make: a bin's letters are read once more, its pairs run side by side
    void align_rest(std::vector<PendingAlign>& pending, const std::vector<Candidate>& candidates, const Letters& letters);
    ResidentBins bins_;
    bool dna_;
    uint32_t errors_;
    uint8_t codes_[256];
    void* d_codes_ = nullptr;
    size_t n_candidates_ = 0, n_confirmed_ = 0, n_device_ = 0, n_device_long_ = 0, n_host_ = 0, n_windows_ = 0;
    bool align_ = false;
    size_t n_align_device_ = 0, n_align_host_ = 0;
    size_t n_targets_ = 0;
    size_t n_wt_device_ = 0, n_wt_host_ = 0, n_wt_calls_ = 0;
    // what the last verify_windows call left for align_windows: where its windows are on the device (the first form's own
    // buffers, the second form's caller's), `strands` entries from entry_of[candidate] (0xFFFFFFFF: the candidate did not take the
    // window kernel), and the window of (candidate, strand) as a string
    struct KeptWindows {
        DeviceBuffer letters, begin, len;
        DeviceWindows on_device{};
        size_t strands = 1;
        std::vector<uint32_t> entry_of;
        Letters letters_of;
    } kept_;
    size_t n_align_windows_calls_ = 0;
    bool keep_windows_ = false;
};

}  // namespace tetrex
