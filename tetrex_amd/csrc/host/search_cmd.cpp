// `tetrex search` — product code (the command's surface is listed at the top of main.cpp).  Four modes: plain records,
// --translate, --window and --translate --frame-window; what they share is at the top.  Thresholds, window layouts, run
// merges and batch cuts are search_plan.hpp's; the device batchers are DeviceIndex's (search_device.cpp).
#include "cli.hpp"
#include "device_index.hpp"
#include "fasta.hpp"
#include "index_file.hpp"
#include "search_plan.hpp"

#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>

namespace tetrex {

namespace {

const char* const kFrames[6] = {"+1", "+2", "+3", "-1", "-2", "-3"};
using Hit = DeviceIndex::TranslatedHit;

// What every mode begins with: the index on the device, the output open, the flags read.
struct Search {
    const Args& a;
    const IndexImage& image;
    const bool verbose, with_counts;
    const double t_start;
    DeviceIndex dev;
    uint64_t k = 0;
    plan::Threshold threshold;
    std::ofstream file;
    std::ostream* out = &std::cout;
    // --verify / --verify-frames (make_verifier)
    std::unique_ptr<BinVerifier> verifier;
    bool align = false, all_targets = false, windows = false;  // windows: --verify-windows, the candidates are windows
    bool align_windows = false;  // --align-windows: the nearest window of every row is aligned after the run merge
    bool window_targets = false;  // --window-targets: a row per run of windows that hit one target

    Search(const Args& args, const IndexImage& img, unsigned long long errors, double fraction, double started = now())
        : a(args), image(img), verbose(args.has("verbose")), with_counts(args.has("counts")), t_start(started) {
        dev.upload(image, std::atoi(a.get("device", "0").c_str()));
        k = dev.encoder().k();
        threshold = plan::Threshold{a.has("threshold"), fraction, k, errors};
        const std::string dest = a.get("output", "-");
        if (dest != "-") {
            file.open(dest);
            if (!file) throw std::runtime_error("Failed to open output file: " + dest);
            out = &file;
        }
    }
    // `verify`: every row is a candidate pair; only those within E edits are written.  --align: with start and cigar;
    // --all-targets: a row per target, not per bin
    void make_verifier(bool verify, bool dna) {
        if (!verify) return;
        verifier = std::make_unique<BinVerifier>(image.bin_paths, dna, (uint32_t)std::min<uint64_t>(threshold.errors, 0xFFFFFFFEull));
        align = a.has("align");
        if (align) verifier->set_align(true);
        all_targets = a.has("all-targets");
        align_windows = a.has("align-windows");
        if (align_windows) verifier->keep_windows(true);
        window_targets = a.has("window-targets");
    }
    void report_verifier() const {
        if (!verifier) return;
        if (verbose)
            std::cerr << "Verified: " << verifier->n_confirmed() << " of " << verifier->n_candidates() << " candidate " << (windows ? "windows" : "pairs") << std::endl;
        if (verbose && (all_targets || window_targets)) std::cerr << "Targets: " << verifier->n_targets() << std::endl;
        if (!std::getenv("TETREX_TRACE")) return;
        const BinVerifier::Routed n = verifier->n_routed();
        std::cerr << "[tetrex search] verify routes: device " << n.device << ", device-long " << n.device_long << ", host " << n.host;
        if (windows) std::cerr << ", windows " << n.windows;
        std::cerr << std::endl;
        if (window_targets) {
            const BinVerifier::WindowTargets wt = verifier->n_window_targets();
            std::cerr << "[tetrex search] window targets: device " << wt.device << ", host " << wt.host << ", calls " << wt.calls << std::endl;
        }
        const BinVerifier::Aligned al = verifier->n_aligned();
        if (align_windows)
            std::cerr << "[tetrex search] align windows: device " << al.device << ", host " << al.host << ", calls " << verifier->n_align_windows_calls() << std::endl;
        if (!align) return;
        std::cerr << "[tetrex search] align routes: device " << al.device << ", host " << al.host << std::endl;
    }
    // the verified columns behind a confirmed row: distance \t target \t end [\t strand] and, with --align,
    // \t start \t cigar — start 1-based (end + 1 for a match that takes no target letter), the cigar like 12=1X30=2I7= ('I': a
    // query letter with no target letter, 'D': a target letter skipped)
    void append_verified(std::string& row, const VerifiedHit& h, bool with_strand) const {
        row.append("\t").append(std::to_string(h.distance)).append("\t").append(*h.target).append("\t").append(std::to_string(h.end));
        if (with_strand) row.append("\t").append(1, h.strand);
        if (!align) return;
        row.append("\t").append(std::to_string((uint64_t)h.start + 1)).append("\t");
        for (const uint32_t run : h.runs) row.append(std::to_string(run >> 2)).append(1, "=XID"[run & 3]);
    }
    // --align-windows behind those: \t wbegin \t wend \t start \t cigar — the aligned window, which is the run's
    // nearest one, as 1-based inclusive positions on the record as given, then start and cigar as --align writes them
    void append_window_alignment(std::string& row, const VerifiedHit& h, uint64_t wbegin, uint64_t wend) const {
        row.append("\t").append(std::to_string(wbegin)).append("\t").append(std::to_string(wend));
        row.append("\t").append(std::to_string((uint64_t)h.start + 1)).append("\t");
        for (const uint32_t run : h.runs) row.append(std::to_string(run >> 2)).append(1, "=XID"[run & 3]);
    }
    void append_count(std::string& row, uint64_t count, uint64_t of) const {
        if (with_counts) row.append("\t").append(std::to_string(count)).append("/").append(std::to_string(of));
    }
    int finish() {
        out->flush();
        report_verifier();
        if (verbose) std::cerr << "Search time: " << (now() - t_start) << " s" << std::endl;
        return 0;
    }
};

// The query file's records in chunks of their bytes, for the two translating modes: at most 64 MiB of letters and 2^20
// records go to the device at once (DeviceIndex cuts a chunk into batches of values)
struct Chunk {
    std::vector<std::string> names;
    std::string seq;
    std::vector<uint64_t> rec_offsets{0};
};
template <class Flush>
void for_each_chunk(const std::string& path, Flush&& flush) {
    const size_t max_bytes = (size_t)64 << 20, max_records = (size_t)1 << 20;
    Chunk c;
    const auto done = [&]() {
        if (c.names.empty()) return;
        flush(c);
        c.names.clear();
        c.seq.clear();
        c.rec_offsets.assign(1, 0);
    };
    for_each_record(path, [&](const FastaRecord& r) {
        if (!c.names.empty() && (c.seq.size() + r.seq.size() > max_bytes || c.names.size() >= max_records)) done();
        c.names.push_back(r.name);
        c.seq.append(r.seq);
        c.rec_offsets.push_back(c.seq.size());
    });
    done();
}

unsigned long long parse_count(const std::string& text, const char* complaint, unsigned long long least, unsigned long long most) {
    char* end = nullptr;
    const unsigned long long v = std::strtoull(text.c_str(), &end, 10);
    if (text.empty() || *end || text[0] == '-' || v < least || v > most) throw std::runtime_error(complaint);
    return v;
}

// tetrex search --translate: nucleotide records on a peptide index.  Every record is translated in its six
// frames on the device; frame f of a record is a query of its own with n_f values (the k-mers of the frame without a stop)
// and the plain rules with n = n_f: -e E gives t = max(n_f - k E, 0), --threshold F gives t = ceil(F n_f).  A frame with
// n_f = 0 or t = 0 reports nothing (a wrong frame is short and full of stops: "every bin" for it would be noise); a record
// none of whose frames is searched gets a note.  Rows: name \t bin path \t frame [\t count/n_f], by record, frame
// (+1 +2 +3 -1 -2 -3) and bin.  -e E --verify-frames: the rows are candidates; each is confirmed by the edit
// distance of the frame's residue letters to the bin's records (BinVerifier, the frames translated on the device) and only
// those within E edits are written, with distance \t target \t end appended; --align appends \t start \t cigar (append_verified).
int search_translated(const Args& a, const IndexImage& image, unsigned long long errors, double fraction) {
    Search s(a, image, errors, fraction);
    s.make_verifier(a.has("verify-frames"), false);
    const bool verify = s.verifier != nullptr;
    std::string row;
    std::vector<uint64_t> n_of, thresholds;
    std::vector<Hit> hits;
    std::vector<VerifiedHit> confirmed;
    std::vector<std::vector<VerifiedHit>> targets;
    for_each_chunk(a.pos[1], [&](const Chunk& c) {
        s.dev.search_translated(c.seq, c.rec_offsets, [&](uint64_t n) { return s.threshold.of(n); }, s.with_counts, n_of, thresholds, hits, s.verifier.get(),
                                verify ? &confirmed : nullptr, s.all_targets ? &targets : nullptr);
        size_t h = 0;
        for (size_t r = 0; r < c.names.size(); ++r) {
            bool searched = false;
            for (size_t f = 0; f < 6; ++f) searched = searched || thresholds[6 * r + f] > 0;
            if (!searched)
                std::cerr << "[tetrex search] " << c.names[r] << ": no frame with " << s.k << "-mers enough for a threshold above 0, skipped" << std::endl;
            for (; h < hits.size() && hits[h].query < 6 * (r + 1); ++h) {
                const Hit& x = hits[h];
                const auto write = [&](const VerifiedHit* v) {
                    row.assign(c.names[r]).append("\t").append(image.bin_paths[x.bin]).append("\t").append(kFrames[x.query % 6]);
                    s.append_count(row, x.count, n_of[x.query]);
                    if (v) s.append_verified(row, *v, false);
                    *s.out << row << '\n';
                };
                if (s.all_targets) {
                    for (const VerifiedHit& v : targets[h]) write(&v);
                    continue;
                }
                if (verify && confirmed[h].distance == 0xFFFFFFFFu) continue;
                write(verify ? &confirmed[h] : nullptr);
            }
        }
    });
    return s.finish();
}

// tetrex search --window W [--step S]: a local search for records longer than what they match.  A record of
// L letters is cut into windows of W letters at letter offsets 0, S, 2 S, ... while offset + W <= L, and one more at L - W where
// the last of these ends before L (every letter is covered); a record of at most W letters is one window
// (plan::record_windows).  A window of l letters has w = l - k + 1 values and the plain rules with n = w: -e E gives
// t = max(w - k E, 0), --threshold F gives t = ceil(F w).  A window with t = 0 is not searched and reports nothing; a record
// that had such a window gets one note.  All windows of a batch of records are counted on the device by sliding
// (txq_count_windows_device) and only the hit list comes back.  Rows: for each (record, bin) every maximal run of
// consecutive hit windows is one row, name \t bin path \t begin \t end [\t count/w], begin and end the 1-based inclusive
// letter positions of the run's union, count/w those of the run's best window (the highest count, the earliest on a tie);
// by record, bin, begin.
// -e E --verify-windows: every hit (window, bin) is a candidate; a window is confirmed in a bin when its letters
// are within E edits of a substring of one record of the bin (BinVerifier::verify_windows: the comparison of --verify, both
// strands on a nucleotide index).  Rows: one for every maximal run of consecutive CONFIRMED windows of a (record, bin) — on a
// nucleotide index of a (record, bin, strand) —, name \t bin path \t begin \t end [\t count/w] \t distance \t target \t
// target_end [\t strand]: count/w of the run's best confirmed window, distance, target and target_end of its window of
// least distance, the earliest on a tie (plan::confirmed_runs); by record, bin, begin.
int search_windowed(const Args& a, const IndexImage& image, unsigned long long errors, double fraction, uint64_t window, uint64_t step) {
    Search s(a, image, errors, fraction);
    const KmerEncoder enc = s.dev.encoder();
    const uint64_t k = s.k;
    // records are collected up to 2^24 values (one longer record: alone); search_windows cuts their windows into device batches
    const size_t max_values = (size_t)1 << 24, max_windows = (size_t)1 << 22;
    struct Rec { std::string name; size_t w0, w1; };  // its windows [w0, w1)
    std::vector<Rec> recs;
    std::vector<uint64_t> values, begins, letter_at;  // letter_at[j]: the 0-based letter offset of window j in its record
    std::vector<uint32_t> lens, thresholds;
    std::vector<Hit> hits, mine;
    std::string row;
    uint64_t n_searched = 0, n_hit = 0, n_rows = 0;
    const bool dna = enc.molecule() == Molecule::DNA;
    s.make_verifier(a.has("verify-windows"), dna);
    const bool verify = s.verifier != nullptr;
    s.windows = verify;
    std::vector<std::string> seqs;  // --verify-windows: the batch's records themselves, and their windows as letters
    std::vector<BinVerifier::Window> win_table;
    std::vector<BinVerifier::Candidate> candidates;
    std::vector<VerifiedHit> confirmed;
    std::vector<std::vector<VerifiedHit>> targets;  // --window-targets: targets[i] are the rows of hits[i]
    // at: its place in `confirmed`; with --window-targets an item is a target hit: row `row` of targets[at], whose target it names
    struct Confirmed { uint32_t query, bin, count, distance; char strand; size_t at; const std::string* target; size_t row; };
    std::vector<Confirmed> kept;
    const auto hit_of = [&](const Confirmed& x) -> VerifiedHit& { return s.window_targets ? targets[x.at][x.row] : confirmed[x.at]; };
    auto flush = [&]() {
        if (recs.empty()) return;
        s.dev.search_windows(values, begins, lens, thresholds, s.with_counts, hits);
        if (verify) {
            candidates.clear();
            for (const Hit& x : hits) candidates.push_back({x.query, x.bin});
            s.verifier->verify_windows(seqs, win_table, candidates, confirmed, s.window_targets ? &targets : nullptr);
        }
        // the confirmed windows among hits [h0, h1) — one record's — by bin, strand and window, and their runs
        const auto merge = [&](size_t h0, size_t h1) {
            kept.clear();
            if (s.window_targets) {  // the target hits by bin, target, strand and window, and their runs per target
                for (size_t i = h0; i < h1; ++i)
                    for (size_t t = 0; t < targets[i].size(); ++t)
                        kept.push_back({hits[i].query, hits[i].bin, hits[i].count, targets[i][t].distance, targets[i][t].strand, i, targets[i][t].target, t});
                std::stable_sort(kept.begin(), kept.end(), [](const Confirmed& x, const Confirmed& y) {
                    if (x.bin != y.bin) return x.bin < y.bin;
                    if (x.target != y.target) return std::less<const std::string*>()(x.target, y.target);  // (the bin's names: the order of its file)
                    return x.strand != y.strand ? x.strand == '+' : x.query < y.query;
                });
                return plan::target_runs(kept);
            }
            for (size_t i = h0; i < h1; ++i)
                if (confirmed[i].distance != 0xFFFFFFFFu) kept.push_back({hits[i].query, hits[i].bin, hits[i].count, confirmed[i].distance, confirmed[i].strand, i, nullptr, 0});
            std::stable_sort(kept.begin(), kept.end(), [](const Confirmed& x, const Confirmed& y) {
                return x.bin != y.bin ? x.bin < y.bin : x.strand != y.strand ? x.strand == '+' : x.query < y.query;
            });
            return plan::confirmed_runs(kept);
        };
        if (s.align_windows) {  // a first pass over the records: the nearest window of every row, all aligned by one call
            std::vector<BinVerifier::Selected> selection;
            size_t h = 0;
            for (const Rec& r : recs) {
                const size_t h0 = h;
                while (h < hits.size() && hits[h].query < r.w1) ++h;
                for (const plan::WindowRun& run : merge(h0, h)) selection.push_back({kept[run.nearest].at, &hit_of(kept[run.nearest])});
            }
            s.verifier->align_windows(candidates, selection);
        }
        size_t h = 0;
        for (const Rec& r : recs) {
            mine.clear();
            const size_t h0 = h;
            for (; h < hits.size() && hits[h].query < r.w1; ++h) mine.push_back(hits[h]);
            if (s.verbose) {
                for (size_t i = 0; i < mine.size(); ++i) n_hit += i == 0 || mine[i].query != mine[i - 1].query;
            }
            if (verify) {
                for (const plan::WindowRun& run : merge(h0, h)) {
                    const Confirmed &first = kept[run.first], &last = kept[run.last], &best = kept[run.best], &nearest = kept[run.nearest];
                    row.assign(r.name).append("\t").append(image.bin_paths[first.bin]).append("\t").append(std::to_string(letter_at[first.query] + 1));
                    row.append("\t").append(std::to_string(letter_at[last.query] + lens[last.query] + k - 1));
                    s.append_count(row, best.count, lens[best.query]);
                    s.append_verified(row, hit_of(nearest), dna);
                    if (s.align_windows)
                        s.append_window_alignment(row, hit_of(nearest), letter_at[nearest.query] + 1, letter_at[nearest.query] + lens[nearest.query] + k - 1);
                    *s.out << row << '\n';
                    ++n_rows;
                }
                continue;
            }
            std::stable_sort(mine.begin(), mine.end(), [](const Hit& x, const Hit& y) { return x.bin < y.bin; });
            plan::for_each_run(mine, [&](const Hit& first, const Hit& last, const Hit& best) {
                row.assign(r.name).append("\t").append(image.bin_paths[first.bin]).append("\t").append(std::to_string(letter_at[first.query] + 1));
                row.append("\t").append(std::to_string(letter_at[last.query] + lens[last.query] + k - 1));
                s.append_count(row, best.count, lens[best.query]);
                *s.out << row << '\n';
                ++n_rows;
            });
        }
        recs.clear();
        seqs.clear();
        win_table.clear();
        values.clear();
        begins.clear();
        letter_at.clear();
        lens.clear();
        thresholds.clear();
    };
    std::vector<uint64_t> v;
    for_each_record(a.pos[1], [&](const FastaRecord& r) {
        v.clear();
        enc.record_values(r.seq, false, v);
        if (v.empty()) {
            std::cerr << "[tetrex search] " << r.name << ": no k-mer of length " << k << ", skipped" << std::endl;
            return;
        }
        if (!recs.empty() && (values.size() + v.size() > max_values || begins.size() >= max_windows)) flush();
        const uint64_t base = values.size();
        values.insert(values.end(), v.begin(), v.end());
        Rec rec{r.name, begins.size(), 0};
        bool unsearched = false;
        const txq::fw::Frame layout = plan::record_windows(r.seq.size(), (uint32_t)k, (uint32_t)window, (uint32_t)step);
        for (uint64_t j = 0; j < layout.count; ++j) {
            const txq::fw::Window at = txq::fw::window_at(layout, j);
            const uint64_t w = at.len - k + 1, t = s.threshold.of(w);
            unsearched = unsearched || t == 0;
            n_searched += t != 0;
            begins.push_back(base + at.a);
            letter_at.push_back(at.a);
            if (verify) win_table.push_back({(uint32_t)recs.size(), at.a, (uint32_t)at.len});
            lens.push_back((uint32_t)w);
            thresholds.push_back((uint32_t)std::min<uint64_t>(t, 0xFFFFFFFEull));
        }
        rec.w1 = begins.size();
        recs.push_back(std::move(rec));
        if (verify) seqs.push_back(r.seq);
        if (unsearched) std::cerr << "[tetrex search] " << r.name << ": a window with threshold 0 is not searched" << std::endl;
    });
    flush();
    s.out->flush();
    if (s.verbose) std::cerr << "Windows: " << n_searched << " searched, " << n_hit << " hit, " << n_rows << " rows" << std::endl;
    return s.finish();
}

// tetrex search --translate --frame-window W [--frame-step S]: the local search of --window in the six frames
// of nucleotide records.  A frame of R residues is cut like a record of R letters under --window (W and S count residues); a
// window is a query of its own with w = its stop-free k-mers — what n_f is to --translate — and t = max(w - k E, 0) or
// ceil(F w).  A window with t = 0 is not searched and reports nothing; a record none of whose windows is searched gets one
// note (wrong frames are full of stops: a note per window would be noise), a record with no k-mer in any window the note of
// --translate.  Translation, the windows' value ranges and the sliding count all stay on the device
// (DeviceIndex::search_translated_windows); the windows' w and the hit list come back.  Rows: for each (record, frame, bin)
// every maximal run of consecutive hit windows is one row, name \t bin path \t frame \t begin \t end [\t count/w]: begin and end
// the 1-based inclusive nucleotide positions of the run's residues on the record as given (begin <= end; the frame carries
// the strand), count/w those of the run's best window (the highest count, the earliest on a tie); by record, frame
// (+1 +2 +3 -1 -2 -3), bin, begin.
// -e E --verify-frame-windows: a window of w stop-free k-mers and s stops is searched with t = w - k (E - s) where
// s <= E and that is above 0 — every stop costs an edit of its own, so nothing is lost and a window with s > E cannot match —,
// every hit (window, bin) is a candidate, and a window is confirmed in a bin when its residue letters are within E edits of a
// substring of one record of the bin (BinVerifier::verify_windows on the frames' letters where txq_translate_frames_device
// left them: the comparison of --verify-frames, one strand).  Rows: one for every maximal run of consecutive CONFIRMED windows
// of a (record, frame, bin), name \t bin path \t frame \t begin \t end [\t count/w] \t distance \t target \t target_end as
// --verify-windows settles them (plan::confirmed_runs); the same order.
int search_translated_windowed(const Args& a, const IndexImage& image, unsigned long long errors, double fraction, uint32_t window, uint32_t step) {
    Search s(a, image, errors, fraction);
    const uint64_t k = s.k;
    std::string row;
    std::vector<uint64_t> win_offsets;
    std::vector<uint32_t> lens, thresholds;
    std::vector<Hit> hits, mine;
    uint64_t n_searched = 0, n_hit = 0, n_rows = 0;
    s.make_verifier(a.has("verify-frame-windows"), false);
    const bool verify = s.verifier != nullptr;
    s.windows = verify;
    DeviceIndex::VerifiedWindows verified;
    verified.verifier = s.verifier.get();
    verified.edits = (uint32_t)std::min<uint64_t>(errors, 0xFFFFFFFEull);
    verified.all_targets = s.window_targets;
    // at: its place in verified.confirmed; with --window-targets an item is a target hit: row `row` of verified.targets[at]
    struct Confirmed { uint32_t query, bin, count, distance; char strand; size_t at; const std::string* target; size_t row; };
    std::vector<Confirmed> kept;
    const auto hit_of = [&](const Confirmed& x) -> VerifiedHit& { return s.window_targets ? verified.targets[x.at][x.row] : verified.confirmed[x.at]; };
    // the confirmed windows among hits [h0, h1) — one frame's — by bin and window, and their runs: what the rows are written
    // from and, with --align-windows, what the nearest windows are selected from, batch by batch
    const auto merge = [&](size_t h0, size_t h1) {
        kept.clear();
        if (s.window_targets) {  // the target hits by bin, target and window, and their runs per target
            for (size_t i = h0; i < h1; ++i)
                for (size_t t = 0; t < verified.targets[i].size(); ++t)
                    kept.push_back({hits[i].query, hits[i].bin, hits[i].count, verified.targets[i][t].distance, '+', i, verified.targets[i][t].target, t});
            std::stable_sort(kept.begin(), kept.end(), [](const Confirmed& x, const Confirmed& y) {
                if (x.bin != y.bin) return x.bin < y.bin;
                return x.target != y.target ? std::less<const std::string*>()(x.target, y.target) : x.query < y.query;
            });
            return plan::target_runs(kept);
        }
        for (size_t i = h0; i < h1; ++i)
            if (verified.confirmed[i].distance != 0xFFFFFFFFu) kept.push_back({hits[i].query, hits[i].bin, hits[i].count, verified.confirmed[i].distance, '+', i, nullptr, 0});
        std::stable_sort(kept.begin(), kept.end(), [](const Confirmed& x, const Confirmed& y) { return x.bin != y.bin ? x.bin < y.bin : x.query < y.query; });
        return plan::confirmed_runs(kept);
    };
    if (s.align_windows && s.window_targets)
        verified.select_rows = [&](size_t h0, size_t h1) {  // the same over target rows: (hit, row of its targets)
            std::vector<std::pair<size_t, size_t>> nearest;
            for (size_t h = h0; h < h1;) {
                const uint64_t frame_end = *std::upper_bound(win_offsets.begin(), win_offsets.end(), (uint64_t)hits[h].query);
                size_t e = h;
                while (e < h1 && hits[e].query < frame_end) ++e;
                for (const plan::WindowRun& run : merge(h, e)) nearest.push_back({kept[run.nearest].at, kept[run.nearest].row});
                h = e;
            }
            return nearest;
        };
    else if (s.align_windows)
        verified.select = [&](size_t h0, size_t h1) {  // the hits of a device batch: whole records, so whole frames
            std::vector<size_t> nearest;
            for (size_t h = h0; h < h1;) {
                const uint64_t frame_end = *std::upper_bound(win_offsets.begin(), win_offsets.end(), (uint64_t)hits[h].query);
                size_t e = h;
                while (e < h1 && hits[e].query < frame_end) ++e;
                for (const plan::WindowRun& run : merge(h, e)) nearest.push_back(kept[run.nearest].at);
                h = e;
            }
            return nearest;
        };
    for_each_chunk(a.pos[1], [&](const Chunk& c) {
        s.dev.search_translated_windows(c.seq, c.rec_offsets, window, step, [&](uint64_t n) { return s.threshold.of(n); }, s.with_counts, win_offsets, lens,
                                        thresholds, hits, verify ? &verified : nullptr);
        size_t h = 0;
        for (size_t r = 0; r < c.names.size(); ++r) {
            const uint64_t L = c.rec_offsets[r + 1] - c.rec_offsets[r];
            bool searched = false, any_kmer = false;
            for (uint64_t j = win_offsets[6 * r]; j < win_offsets[6 * r + 6]; ++j) {
                searched = searched || thresholds[j] > 0;
                any_kmer = any_kmer || lens[j] > 0;
                n_searched += thresholds[j] > 0;
            }
            if (!any_kmer)
                std::cerr << "[tetrex search] " << c.names[r] << ": no frame with " << k << "-mers enough for a threshold above 0, skipped" << std::endl;
            else if (!searched)
                std::cerr << "[tetrex search] " << c.names[r] << ": no window with a threshold above 0, not searched" << std::endl;
            for (uint32_t f = 0; f < 6; ++f) {
                const uint64_t w0 = win_offsets[6 * r + f], w1 = win_offsets[6 * r + f + 1];
                mine.clear();
                const size_t h0 = h;
                for (; h < hits.size() && hits[h].query < w1; ++h) mine.push_back(hits[h]);
                if (mine.empty()) continue;
                const txq::fw::Frame layout = txq::fw::frame_plan(txq::tr::frame_len(L, f % 3), (uint32_t)k, window, step);
                for (size_t i = 0; i < mine.size(); ++i) n_hit += i == 0 || mine[i].query != mine[i - 1].query;
                const auto begin_row = [&](uint32_t bin, uint32_t first, uint32_t last) {
                    const txq::fw::Window wf = txq::fw::window_at(layout, first - w0), wl = txq::fw::window_at(layout, last - w0);
                    const txq::fw::Span at = txq::fw::residues_on_record(L, f, wf.a, wl.a + wl.len);
                    row.assign(c.names[r]).append("\t").append(image.bin_paths[bin]).append("\t").append(kFrames[f]);
                    row.append("\t").append(std::to_string(at.begin)).append("\t").append(std::to_string(at.end));
                };
                if (verify) {
                    for (const plan::WindowRun& run : merge(h0, h)) {
                        const Confirmed &first = kept[run.first], &last = kept[run.last], &best = kept[run.best], &nearest = kept[run.nearest];
                        begin_row(first.bin, first.query, last.query);
                        s.append_count(row, best.count, lens[best.query]);
                        s.append_verified(row, hit_of(nearest), false);
                        if (s.align_windows) {
                            const txq::fw::Window wn = txq::fw::window_at(layout, nearest.query - w0);
                            const txq::fw::Span on = txq::fw::residues_on_record(L, f, wn.a, wn.a + wn.len);
                            s.append_window_alignment(row, hit_of(nearest), on.begin, on.end);
                        }
                        *s.out << row << '\n';
                        ++n_rows;
                    }
                    continue;
                }
                std::stable_sort(mine.begin(), mine.end(), [](const Hit& x, const Hit& y) { return x.bin < y.bin; });
                plan::for_each_run(mine, [&](const Hit& first, const Hit& last, const Hit& best) {
                    begin_row(first.bin, first.query, last.query);
                    s.append_count(row, best.count, lens[best.query]);
                    *s.out << row << '\n';
                    ++n_rows;
                });
            }
        }
    });
    s.out->flush();
    if (s.verbose) std::cerr << "Windows: " << n_searched << " searched, " << n_hit << " hit, " << n_rows << " rows" << std::endl;
    return s.finish();
}

// tetrex search: each record of the query file is a query; its values are the index's k-mers of the record (n of them) and a
// bin is reported when at least t of them are in it (txq_count).  -e E: t = max(n - k E, 0) — a record within E edits of a
// substring of a bin shares at least n - k E k-mer positions with it (q-gram lemma), and a Bloom filter drops none of them,
// so that bin is always reported.  --threshold F (0 < F <= 1): t = ceil(F n).  Rows: name \t bin path [\t count/n].
// -e E --verify: the reported bins are candidates; each is confirmed by the edit distance of the record to the
// bin's records (BinVerifier) and only the bins within E edits are written, with distance \t target \t end [\t strand] appended.
// --align (with --verify or --verify-frames) appends \t start \t cigar to each of those rows; on strand - the cigar is
// that of the reverse-complemented record against the target, in the target's coordinates.
int search_plain(const Args& a, const IndexImage& image, unsigned long long errors, double fraction, double t_start) {
    Search s(a, image, errors, fraction, t_start);
    const KmerEncoder enc = s.dev.encoder();
    const uint64_t bins = s.dev.bins(), W = s.dev.result_words();
    // queries go to the device in batches: at most 2^24 values, and at most 256 MiB of counts
    const size_t max_values = (size_t)1 << 24, max_queries = std::max<size_t>(1, ((size_t)256 << 20) / (W * 64 * 4));
    std::vector<std::string> names;
    std::vector<uint64_t> values, offsets{0}, n_of;
    std::vector<uint32_t> thresholds, counts;
    std::vector<uint64_t> hits;
    std::string row;
    const bool dna = enc.molecule() == Molecule::DNA;
    s.make_verifier(a.has("verify"), dna);
    const bool verify = s.verifier != nullptr;
    std::vector<std::string> seqs;  // --verify: the batch's records themselves
    std::vector<BinVerifier::Candidate> candidates;
    std::vector<VerifiedHit> confirmed;
    std::vector<std::vector<VerifiedHit>> targets;
    auto flush = [&]() {
        if (names.empty()) return;
        s.dev.count(values, offsets, thresholds, hits, s.with_counts ? &counts : nullptr);
        const auto write = [&](size_t q, size_t u, const VerifiedHit* h) {
            row.assign(names[q]).append("\t").append(image.bin_paths[u]);
            if (s.with_counts) s.append_count(row, counts[q * W * 64 + u], n_of[q]);
            if (h) s.append_verified(row, *h, dna);
            *s.out << row << '\n';
        };
        if (verify) {
            candidates.clear();
            for (size_t q = 0; q < names.size(); ++q)
                for (uint64_t u : set_bins(hits.data() + q * W, bins)) candidates.push_back({(uint32_t)q, (uint32_t)u});
            s.verifier->verify(seqs, candidates, confirmed, s.all_targets ? &targets : nullptr);
            for (size_t c = 0; c < candidates.size(); ++c) {
                const size_t q = candidates[c].query, u = candidates[c].bin;
                if (s.all_targets) {
                    for (const VerifiedHit& h : targets[c]) write(q, u, &h);
                    continue;
                }
                if (confirmed[c].distance == 0xFFFFFFFFu) continue;
                write(q, u, &confirmed[c]);
            }
            seqs.clear();
        } else {
            for (size_t q = 0; q < names.size(); ++q)
                for (uint64_t u : set_bins(hits.data() + q * W, bins)) write(q, u, nullptr);
        }
        names.clear();
        values.clear();
        offsets.assign(1, 0);
        n_of.clear();
        thresholds.clear();
    };
    std::vector<uint64_t> v;
    for_each_record(a.pos[1], [&](const FastaRecord& r) {
        v.clear();
        enc.record_values(r.seq, false, v);
        const uint64_t n = v.size();
        if (n == 0) {
            std::cerr << "[tetrex search] " << r.name << ": no k-mer of length " << enc.k() << ", skipped" << std::endl;
            return;
        }
        const uint64_t t = s.threshold.of(n);
        if (t == 0) std::cerr << "[tetrex search] " << r.name << ": threshold 0, every bin is reported" << std::endl;
        if (values.size() + n > max_values || names.size() >= max_queries) flush();
        names.push_back(r.name);
        if (verify) seqs.push_back(r.seq);
        values.insert(values.end(), v.begin(), v.end());
        offsets.push_back(values.size());
        n_of.push_back(n);
        thresholds.push_back((uint32_t)std::min<uint64_t>(t, 0xFFFFFFFFull));
    });
    flush();
    return s.finish();
}

}  // namespace

int cmd_search(int argc, char** argv) {
    const std::vector<OptSpec> spec = {{'e', "errors", true}, {'\0', "threshold", true}, {'\0', "counts", false}, {'o', "output", true},
                                       {'v', "verbose", false}, {'D', "device", true}, {'\0', "translate", false}, {'\0', "verify", false},
                                       {'\0', "verify-frames", false}, {'\0', "verify-windows", false}, {'\0', "verify-frame-windows", false}, {'\0', "align", false}, {'\0', "align-windows", false}, {'\0', "all-targets", false}, {'\0', "window-targets", false},
                                       {'\0', "window", true}, {'\0', "step", true}, {'\0', "frame-window", true}, {'\0', "frame-step", true}};
    Args a;
    unsigned long long errors = 0, window = 0, step = 0, frame_window = 0, frame_step = 0;
    double fraction = 0;
    try {
        a = parse(argc, argv, 2, spec);
        if (a.pos.size() != 2) throw std::runtime_error("expected <index> <queries.fa>");
        if (a.has("align-windows") && !a.has("verify-windows") && !a.has("verify-frame-windows"))
            throw std::runtime_error("--align-windows gives start and cigar of confirmed window runs: it needs --window W -e E --verify-windows, or --translate --frame-window W -e E --verify-frame-windows");
        // (--align is the whole-record flag; next to the window modes its refusal names the flag that is meant)
        // (likewise --all-targets: every target of confirmed window runs is --window-targets)
        if (a.has("window-targets") && !a.has("verify-windows") && !a.has("verify-frame-windows"))
            throw std::runtime_error("--window-targets gives a row for every target of confirmed window runs: it needs --window W -e E --verify-windows, or --translate --frame-window W -e E --verify-frame-windows");
        const auto hint = [](const char* o) {
            return std::string(o) == "align"         ? " (the alignment of confirmed window runs is --align-windows)"
                   : std::string(o) == "all-targets" ? " (every target of confirmed window runs is --window-targets)"
                                                     : "";
        };
        if (a.has("step") && !a.has("window")) throw std::runtime_error("--step is the distance between the windows of --window W: it needs --window");
        if (a.has("frame-step") && !a.has("frame-window"))
            throw std::runtime_error("--frame-step is the distance between the windows of --frame-window W: it needs --frame-window");
        if (a.has("frame-window")) {
            if (!a.has("translate")) throw std::runtime_error("--frame-window cuts the translated frames of --translate into windows: it needs --translate");
            if (a.has("window")) throw std::runtime_error("--frame-window cannot be combined with --window: one counts residues of a translated frame, the other letters of the record");
            if (a.has("step")) throw std::runtime_error("--frame-window cannot be combined with --step: the distance between frame windows is --frame-step");
            for (const char* o : {"verify-windows", "verify-frames", "all-targets", "align", "verify"})
                if (a.has(o))
                    throw std::runtime_error(std::string("--frame-window cannot be combined with --") + o +
                                             ": frame windows are not verified by it (they are confirmed with --verify-frame-windows, which gives distance, target and end)" + hint(o));
            if (!a.has("errors") && !a.has("threshold")) throw std::runtime_error("--frame-window needs -e E or --threshold F");
            frame_window = parse_count(a.get("frame-window", ""), "--frame-window must be a number of residues >= k", 1, 0x7FFFFFFFull);
            frame_step = std::max<unsigned long long>(1, frame_window / 2);
            if (a.has("frame-step"))
                frame_step = parse_count(a.get("frame-step", ""), "--frame-step must be a number of residues in 1 .. --frame-window", 1, frame_window);
        }
        if (a.has("verify-frame-windows")) {
            if (!a.has("translate")) throw std::runtime_error("--verify-frame-windows confirms the windows of --translate --frame-window W: it needs --translate");
            for (const char* o : {"window", "step", "verify-windows", "verify-frames", "all-targets", "align", "verify"})
                if (a.has(o)) throw std::runtime_error(std::string("--verify-frame-windows cannot be combined with --") + o + ": it confirms the windows of --frame-window, with distance, target and end" + hint(o));
            if (!a.has("frame-window")) throw std::runtime_error("--verify-frame-windows confirms the windows of --frame-window W: it needs --frame-window");
            if (a.has("threshold")) throw std::runtime_error("--verify-frame-windows confirms the windows of -e E: it cannot be combined with --threshold");
            if (!a.has("errors")) throw std::runtime_error("--verify-frame-windows needs -e E: the number of residue edits a confirmed window may be away");
        }
        if (a.has("verify-windows")) {
            if (a.has("translate")) throw std::runtime_error("--verify-windows cannot be combined with --translate: it confirms the windows of --window, which --translate does not cut");
            if (!a.has("window")) throw std::runtime_error("--verify-windows confirms the windows of --window W: it needs --window");
            if (a.has("threshold")) throw std::runtime_error("--verify-windows confirms the windows of -e E: it cannot be combined with --threshold");
            if (!a.has("errors")) throw std::runtime_error("--verify-windows needs -e E: the number of edits a confirmed window may be away");
            for (const char* o : {"verify-frames", "all-targets", "align", "verify"})
                if (a.has(o)) throw std::runtime_error(std::string("--verify-windows cannot be combined with --") + o + ": a confirmed window gets its distance, target and end" + hint(o));
        }
        if (a.has("window")) {
            if (a.has("translate")) throw std::runtime_error("--window cannot be combined with --translate: translated frames lose their positions where stops are taken out (translated records: --frame-window)");
            if (a.has("verify-frames")) throw std::runtime_error("--window cannot be combined with --verify-frames: it confirms translated frames, which --window does not search");
            for (const char* o : {"all-targets", "align", "verify"})
                if (a.has(o)) throw std::runtime_error(std::string("--window cannot be combined with --") + o + ": windows are confirmed with --verify-windows" + hint(o));
            if (!a.has("errors") && !a.has("threshold")) throw std::runtime_error("--window needs -e E or --threshold F");
            window = parse_count(a.get("window", ""), "--window must be a number of letters >= k", 1, 0x7FFFFFFFull);
            step = std::max<unsigned long long>(1, window / 2);
            if (a.has("step")) step = parse_count(a.get("step", ""), "--step must be a number of letters in 1 .. --window", 1, window);
        }
        if (a.has("verify-frames")) {
            if (a.has("verify")) throw std::runtime_error("--verify-frames cannot be combined with --verify: one confirms translated frames, the other plain records");
            if (!a.has("translate")) throw std::runtime_error("--verify-frames confirms the rows of --translate: it needs --translate");
            if (a.has("threshold")) throw std::runtime_error("--verify-frames confirms the bins of -e E: it cannot be combined with --threshold");
            if (!a.has("errors")) throw std::runtime_error("--verify-frames needs -e E: the number of residue edits a confirmed frame may be away");
        }
        if (a.has("align") && !a.has("verify") && !a.has("verify-frames"))
            throw std::runtime_error("--align gives the alignment of confirmed rows: it needs --verify, or --translate --verify-frames");
        if (a.has("all-targets") && !a.has("verify") && !a.has("verify-frames"))
            throw std::runtime_error("--all-targets lists every target of confirmed rows: it needs -e E --verify, or --translate -e E --verify-frames");
        if (a.has("verify") && a.has("threshold")) throw std::runtime_error("--verify confirms the bins of -e E: it cannot be combined with --threshold");
        if (a.has("verify") && a.has("translate")) throw std::runtime_error("--verify cannot be combined with --translate (translated rows are confirmed with --verify-frames)");
        if (a.has("verify") && !a.has("errors")) throw std::runtime_error("--verify needs -e E: the number of edits a confirmed bin may be away");
        if (a.has("errors") && a.has("threshold")) throw std::runtime_error("-e and --threshold exclude each other");
        if (a.has("errors")) errors = parse_count(a.get("errors", ""), "-e must be a number of errors >= 0", 0, ~0ull);
        if (a.has("threshold")) {
            const std::string f = a.get("threshold", "");
            char* end = nullptr;
            fraction = std::strtod(f.c_str(), &end);
            if (f.empty() || *end || !(fraction > 0.0 && fraction <= 1.0)) throw std::runtime_error("--threshold must be a fraction in (0, 1]");
        }
    } catch (const std::exception& e) {
        std::cerr << "[Search Parser Error] " << e.what() << "\n";
        return 1;
    }
    const double t_start = now();
    IndexImage image;
    try {
        image = read_index_file(a.pos[0]);
    } catch (const std::exception& e) {
        std::cerr << "Filepath to (H)IBF Index not valid" << std::endl;
        std::cerr << e.what() << '\n';
        return 1;
    }
    // --window W / --frame-window W against the index's k: W must hold a k-mer, and with -e E a full window (w = W - k + 1 values,
    // t = max(w - k E, 0)) must keep a threshold above 0, or no full window at all would be searched
    const auto window_fits = [&](const char* option, const char* unit, unsigned long long w) {
        const unsigned long long k = image.k;
        if (w < k) {
            std::cerr << "[Search Parser Error] " << option << " must be a number of " << unit << " >= k: the index has k = " << k << "\n";
            return false;
        }
        if (a.has("errors") && (errors > 0xFFFFFFFFull || w - k + 1 <= k * errors)) {
            std::cerr << "[Search Parser Error] " << option << " " << w << " with -e " << errors << " leaves every window a threshold of 0 (k = " << k
                      << "): the smallest workable " << option << " is " << (k * errors + k) << "\n";
            return false;
        }
        return true;
    };
    if (a.has("translate")) {
        if (image.molecule == "na" || image.k < 1 || image.k > 12) {
            std::cerr << "[tetrex search] --translate needs a peptide index with k in 1..12: " << a.pos[0] << " is a "
                      << (image.molecule == "na" ? "nucleotide index" : "peptide index with k = " + std::to_string(image.k)) << std::endl;
            return 1;
        }
        if (!a.has("frame-window")) return search_translated(a, image, errors, fraction);
        if (!window_fits("--frame-window", "residues", frame_window)) return 1;
        return search_translated_windowed(a, image, errors, fraction, (uint32_t)frame_window, (uint32_t)frame_step);
    }
    if (a.has("window")) {
        if (!window_fits("--window", "letters", window)) return 1;
        return search_windowed(a, image, errors, fraction, window, step);
    }
    return search_plain(a, image, errors, fraction, t_start);
}

}  // namespace tetrex
