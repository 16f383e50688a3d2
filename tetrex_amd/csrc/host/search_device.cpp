// The device batchers of `tetrex search`: DeviceIndex::search_translated, search_windows and search_translated_windows
// (device_index.hpp, where their contracts are), and what the three share — the limits of a batch, the hit lister, the record
// batches and their upload.  How windows and records are cut into batches is search_plan.hpp's.
#include "device_buffer.hpp"
#include "device_index.hpp"
#include "search_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

namespace tetrex {

namespace {

// a batch: at most 2^24 values, and at most 256 MiB of hit words / counts
constexpr uint64_t kMaxBatchValues = (uint64_t)1 << 24;
constexpr size_t kMaxBatchHitBytes = (size_t)256 << 20;
size_t max_batch_rows(size_t W, bool with_counts) { return kMaxBatchHitBytes / (W * (with_counts ? 64 * 4 : 8)); }
// ... and, for windows, at most TETREX_SEARCH_BATCH_WINDOWS of them where that is set
size_t max_batch_windows(size_t W, bool with_counts) {
    size_t most = std::max<size_t>(1, max_batch_rows(W, with_counts));
    if (const char* e = std::getenv("TETREX_SEARCH_BATCH_WINDOWS"); e && *e) most = std::min<size_t>(most, std::max<long long>(1, std::atoll(e)));
    return most;
}

// what the device gets for a threshold: 0 becomes 0xFFFFFFFF (no count reaches it: a query that is not searched has no hits)
uint32_t device_threshold(uint64_t t) { return t ? (uint32_t)std::min<uint64_t>(t, 0xFFFFFFFEull) : 0xFFFFFFFFu; }

// The list of the set bits of a hit matrix (txq_hit_list_device), one list buffer for all batches of a call.
struct HitLister {
    DeviceBuffer d_list, d_total{8};
    size_t list_cap = (size_t)1 << 20;
    std::vector<uint32_t> list;  // the last matrix's (row, bin, count) triples as the device gave them
    HitLister() { d_list.reserve(list_cap * 12); }
    // n rows of W words at d_hit (d_cnt: their counts, or null): appends (query0 + row, bin0 + bin, count) to hits, in
    // (row, bin) order, and returns how many
    uint64_t run(const DeviceBuffer& d_hit, const DeviceBuffer* d_cnt, size_t n, size_t W, uint32_t query0, uint32_t bin0,
                 std::vector<DeviceIndex::TranslatedHit>& hits) {
        uint64_t total = 0;
        for (;;) {
            d_list.reserve(list_cap * 12);
            txq_check(txq_hit_list_device((const uint64_t*)d_hit.p, d_cnt ? (const uint32_t*)d_cnt->p : nullptr, n, W, (uint32_t*)d_list.p, list_cap,
                                          (uint64_t*)d_total.p, nullptr), "txq_hit_list_device");
            txq_check(txq_memcpy_d2h(&total, d_total.p, 8), "d2h");
            if (total <= list_cap) break;
            list_cap = total;  // (the list did not fit: once more with room for all of it)
        }
        list.resize(3 * total);
        if (total) txq_check(txq_memcpy_d2h(list.data(), d_list.p, total * 12), "d2h");
        for (uint64_t i = 0; i < total; ++i) hits.push_back(DeviceIndex::TranslatedHit{query0 + list[3 * i], bin0 + list[3 * i + 1], list[3 * i + 2]});
        return total;
    }
};

// the record batches of the two translating searches: at most 2^24 values by txq_translate_bound, a larger record alone
plan::Cuts cut_translate_batches(const std::vector<uint64_t>& rec_offsets, unsigned k, size_t max_records) {
    return plan::cut_records(rec_offsets, [&](size_t r) {
        const uint64_t b = txq_translate_bound(rec_offsets.data() + r, 1, k);
        if (b == UINT64_MAX) txq_check(TXQ_ERR_ARG, "txq_translate_bound");
        return b;
    }, kMaxBatchValues, max_records);
}

// the records [r0, r1) to the device: their bytes, and their offsets rebased to the first of them (left in `rebased`)
void upload_records(std::string_view seq, const std::vector<uint64_t>& rec_offsets, size_t r0, size_t r1, DeviceBuffer& d_seq, DeviceBuffer& d_rec,
                    std::vector<uint64_t>& rebased) {
    const uint64_t first = rec_offsets[r0], bytes = rec_offsets[r1] - first;
    rebased.assign(rec_offsets.begin() + r0, rec_offsets.begin() + r1 + 1);
    for (uint64_t& o : rebased) o -= first;
    if (bytes) txq_check(txq_memcpy_h2d(d_seq.p, seq.data() + first, bytes), "h2d");
    txq_check(txq_memcpy_h2d(d_rec.p, rebased.data(), rebased.size() * 8), "h2d");
}

}  // namespace

void DeviceIndex::search_translated(std::string_view seq, const std::vector<uint64_t>& rec_offsets,
                                    const std::function<uint64_t(uint64_t)>& threshold_of, bool with_counts, std::vector<uint64_t>& n_of,
                                    std::vector<uint64_t>& thresholds, std::vector<TranslatedHit>& hits, BinVerifier* verifier,
                                    std::vector<VerifiedHit>* confirmed, std::vector<std::vector<VerifiedHit>>* all_targets) {
    if (!ix_) throw std::runtime_error("index not uploaded");
    if (verifier && !confirmed) throw std::runtime_error("search_translated: a verifier needs somewhere to put its answers");
    if (confirmed) confirmed->clear();
    if (all_targets) all_targets->clear();
    std::vector<std::vector<VerifiedHit>> batch_targets;
    if (shards_.size() > 1) throw std::runtime_error("search_translated: one shard only");
    if (enc_.molecule() != Molecule::Peptide) throw std::runtime_error("search_translated: a peptide index is needed");
    if (rec_offsets.empty() || rec_offsets.back() > seq.size()) throw std::runtime_error("search_translated: record offsets run past the bytes");
    const unsigned k = enc_.k();
    const size_t R = rec_offsets.size() - 1, W = info_.shard_words;
    n_of.assign(6 * R, 0);
    thresholds.assign(6 * R, 0);
    hits.clear();
    if (R == 0 || W == 0) return;
    // the record batches, at most 256 MiB of hit words / counts each (six queries a record).  The buffers are sized for the
    // largest batch before the first one runs, so that no device memory of the call is freed or allocated between its
    // launches ("Host").
    const plan::Cuts cuts = cut_translate_batches(rec_offsets, k, std::max<size_t>(6, max_batch_rows(W, with_counts)) / 6);
    const size_t most_queries = 6 * cuts.most_items;
    DeviceBuffer d_codes(256), d_seq(cuts.most_bytes + 16), d_rec((cuts.most_items + 1) * 8), d_val(cuts.most_values * 8 + 8),
        d_off((most_queries + 1) * 8), d_thr(most_queries * 4), d_hit(most_queries * W * 8), d_cnt;
    if (with_counts) d_cnt.reserve(most_queries * W * 64 * 4);
    txq_check(txq_memcpy_h2d(d_codes.p, enc_.aa_table().data(), 256), "h2d");
    HitLister lister;
    std::vector<uint64_t> rebased, off;
    std::vector<uint32_t> thr;
    const uint32_t bin0 = (uint32_t)(info_.shard_word0 * 64);
    // --verify-frames
    const char* frames_env = std::getenv("TETREX_VERIFY_FRAMES");
    const bool frames_on_host = frames_env && std::string(frames_env) == "host";
    DeviceBuffer d_frames, d_foff;
    std::vector<BinVerifier::Candidate> candidates;
    std::vector<uint64_t> lengths;
    std::vector<std::string> frame_strings;
    std::vector<VerifiedHit> batch_confirmed;
    for (size_t c = 0; c + 1 < cuts.cut.size(); ++c) {
        const size_t r0 = cuts.cut[c], r1 = cuts.cut[c + 1], nr = r1 - r0, nq = 6 * nr;
        const uint64_t first = rec_offsets[r0];
        upload_records(seq, rec_offsets, r0, r1, d_seq, d_rec, rebased);
        txq_check(txq_translate_device((const uint8_t*)d_seq.p, (const uint64_t*)d_rec.p, nr, k, (const uint8_t*)d_codes.p, (uint64_t*)d_val.p,
                                       (uint64_t*)d_off.p, nullptr), "txq_translate_device");
        off.resize(nq + 1);
        txq_check(txq_memcpy_d2h(off.data(), d_off.p, off.size() * 8), "d2h");
        thr.resize(nq);
        bool any = false;
        for (size_t q = 0; q < nq; ++q) {
            const uint64_t n = off[q + 1] - off[q], t = n ? threshold_of(n) : 0;
            n_of[6 * r0 + q] = n;
            thresholds[6 * r0 + q] = t;
            thr[q] = device_threshold(t);
            any = any || t;
        }
        if (!any) continue;
        txq_check(txq_memcpy_h2d(d_thr.p, thr.data(), nq * 4), "h2d");
        txq_check(txq_count_device(ix_, (const uint64_t*)d_val.p, (const uint64_t*)d_off.p, nq, (const uint32_t*)d_thr.p, (uint64_t*)d_hit.p,
                                   with_counts ? (uint32_t*)d_cnt.p : nullptr, nullptr), "txq_count_device");
        const uint64_t total = lister.run(d_hit, with_counts ? &d_cnt : nullptr, nq, W, (uint32_t)(6 * r0), bin0, hits);
        if (!verifier || total == 0) continue;
        // --verify-frames: the batch's hits are candidates, pattern index = query index within the batch
        const std::vector<uint32_t>& list = lister.list;
        candidates.resize(total);
        for (uint64_t i = 0; i < total; ++i) candidates[i] = BinVerifier::Candidate{list[3 * i], bin0 + list[3 * i + 1]};
        const auto frame_letters = [&](uint32_t q) {
            return translate_frame(seq.substr(first + rebased[q / 6], rebased[q / 6 + 1] - rebased[q / 6]), q % 6);
        };
        if (frames_on_host) {
            frame_strings.assign(nq, std::string());
            for (const BinVerifier::Candidate& x : candidates)
                if (frame_strings[x.query].empty()) frame_strings[x.query] = frame_letters(x.query);
            verifier->verify(frame_strings, candidates, batch_confirmed, all_targets ? &batch_targets : nullptr);
        } else {
            const uint64_t frames_bytes = txq_translate_frames_bound(rebased.data(), nr);
            if (frames_bytes == UINT64_MAX) txq_check(TXQ_ERR_ARG, "txq_translate_frames_bound");
            d_frames.reserve(frames_bytes + 16);  // (the slack BinVerifier gives its own pattern buffer)
            d_foff.reserve((nq + 1) * 8);
            txq_check(txq_translate_frames_device((const uint8_t*)d_seq.p, (const uint64_t*)d_rec.p, nr, (uint8_t*)d_frames.p, frames_bytes,
                                                  (uint64_t*)d_foff.p, nullptr), "txq_translate_frames_device");
            lengths.resize(total);
            for (uint64_t i = 0; i < total; ++i) {
                const uint32_t q = candidates[i].query;
                const uint64_t L = rebased[q / 6 + 1] - rebased[q / 6], o = q % 3;
                lengths[i] = L >= o ? (L - o) / 3 : 0;
            }
            verifier->verify(BinVerifier::DevicePatterns{(const uint8_t*)d_frames.p, (const uint64_t*)d_foff.p, nq, frames_bytes}, candidates, lengths,
                             frame_letters, batch_confirmed, all_targets ? &batch_targets : nullptr);
        }
        confirmed->insert(confirmed->end(), batch_confirmed.begin(), batch_confirmed.end());
        if (all_targets) all_targets->insert(all_targets->end(), std::make_move_iterator(batch_targets.begin()), std::make_move_iterator(batch_targets.end()));
    }
}

void DeviceIndex::search_windows(const std::vector<uint64_t>& values, const std::vector<uint64_t>& begins, const std::vector<uint32_t>& lens,
                                 const std::vector<uint32_t>& thresholds, bool with_counts, std::vector<TranslatedHit>& hits) {
    if (!ix_) throw std::runtime_error("index not uploaded");
    if (shards_.size() > 1) throw std::runtime_error("search_windows: one shard only");
    const size_t N = begins.size(), W = info_.shard_words;
    if (lens.size() != N || thresholds.size() != N) throw std::runtime_error("search_windows: begins, lens and thresholds disagree");
    hits.clear();
    for (size_t j = 0; j < N; ++j) {
        if (begins[j] > values.size() || lens[j] > values.size() - begins[j]) throw std::runtime_error("search_windows: a window runs past the values");
        if (j && (begins[j] < begins[j - 1] || begins[j] + lens[j] < begins[j - 1] + lens[j - 1])) throw std::runtime_error("search_windows: the windows do not slide");
    }
    if (N == 0 || W == 0) return;
    const bool trace = std::getenv("TETREX_TRACE") != nullptr;
    // the batches: windows [cut[i], cut[i + 1]), values [begin of the first, end of the last) (a window longer than the bound
    // on values: a batch of its own).  The buffers are sized for the largest batch before the first one runs, so that no
    // device memory is freed or allocated between the launches of a call.
    const plan::Cuts cuts = plan::cut_windows(begins, lens, kMaxBatchValues, max_batch_windows(W, with_counts));
    const size_t most_windows = cuts.most_items;
    DeviceBuffer d_val(cuts.most_values * 8 + 8), d_beg(most_windows * 8), d_len(most_windows * 4), d_thr(most_windows * 4), d_hit(most_windows * W * 8), d_cnt;
    if (with_counts) d_cnt.reserve(most_windows * W * 64 * 4);
    HitLister lister;
    std::vector<uint64_t> beg;
    std::vector<uint32_t> thr;
    const uint32_t bin0 = (uint32_t)(info_.shard_word0 * 64);
    for (size_t c = 0; c + 1 < cuts.cut.size(); ++c) {
        const size_t first = cuts.cut[c], j1 = cuts.cut[c + 1], n = j1 - first;
        const uint64_t v0 = begins[first], v1 = begins[j1 - 1] + lens[j1 - 1];
        bool any = false;
        for (size_t j = first; j < j1; ++j) any = any || thresholds[j] > 0;
        if (!any) continue;
        beg.assign(begins.begin() + first, begins.begin() + j1);
        for (uint64_t& b : beg) b -= v0;
        thr.resize(n);
        for (size_t j = 0; j < n; ++j) thr[j] = device_threshold(thresholds[first + j]);
        if (v1 > v0) txq_check(txq_memcpy_h2d(d_val.p, values.data() + v0, (v1 - v0) * 8), "h2d");
        txq_check(txq_memcpy_h2d(d_beg.p, beg.data(), n * 8), "h2d");
        txq_check(txq_memcpy_h2d(d_len.p, lens.data() + first, n * 4), "h2d");
        txq_check(txq_memcpy_h2d(d_thr.p, thr.data(), n * 4), "h2d");
        txq_check(txq_count_windows_device(ix_, (const uint64_t*)d_val.p, (const uint64_t*)d_beg.p, (const uint32_t*)d_len.p, n, (const uint32_t*)d_thr.p,
                                           (uint64_t*)d_hit.p, with_counts ? (uint32_t*)d_cnt.p : nullptr, nullptr), "txq_count_windows_device");
        const uint64_t total = lister.run(d_hit, with_counts ? &d_cnt : nullptr, n, W, (uint32_t)first, bin0, hits);
        if (trace)
            std::fprintf(stderr, "[tetrex search] window batch: windows %zu..%zu, values %llu..%llu, %llu hits\n", first, j1, (unsigned long long)v0,
                         (unsigned long long)v1, (unsigned long long)total);
    }
}

void DeviceIndex::search_translated_windows(std::string_view seq, const std::vector<uint64_t>& rec_offsets, uint32_t window, uint32_t step,
                                            const std::function<uint64_t(uint64_t)>& threshold_of, bool with_counts,
                                            std::vector<uint64_t>& win_offsets, std::vector<uint32_t>& lens, std::vector<uint32_t>& thresholds,
                                            std::vector<TranslatedHit>& hits, VerifiedWindows* verified) {
    if (!ix_) throw std::runtime_error("index not uploaded");
    if (shards_.size() > 1) throw std::runtime_error("search_translated_windows: one shard only");
    if (enc_.molecule() != Molecule::Peptide) throw std::runtime_error("search_translated_windows: a peptide index is needed");
    if (rec_offsets.empty() || rec_offsets.back() > seq.size()) throw std::runtime_error("search_translated_windows: record offsets run past the bytes");
    const unsigned k = enc_.k();
    if (window < k || step < 1 || step > window) throw std::runtime_error("search_translated_windows: the window must hold a k-mer and the step lie in 1 .. window");
    const size_t R = rec_offsets.size() - 1, W = info_.shard_words;
    // the window layout is closed-form in the record lengths (txq_frame_windows_plan.hpp): the device writes the same offsets
    win_offsets.assign(6 * R + 1, 0);
    for (size_t r = 0; r < R; ++r) {
        if (rec_offsets[r + 1] < rec_offsets[r]) throw std::runtime_error("search_translated_windows: record offsets descend");
        for (uint32_t f = 0; f < 6; ++f)
            win_offsets[6 * r + f + 1] = win_offsets[6 * r + f] + txq::fw::window_count(txq::tr::frame_len(rec_offsets[r + 1] - rec_offsets[r], f % 3), k, window, step);
    }
    const uint64_t N = win_offsets.back();
    if (N > 0xFFFFFFFEull) throw std::runtime_error("search_translated_windows: more than 2^32 - 2 windows in one call");
    lens.assign(N, 0);
    thresholds.assign(N, 0);
    hits.clear();
    if (verified) {
        if (!verified->verifier) throw std::runtime_error("search_translated_windows: verified windows need a verifier");
        verified->stops.assign(N, 0);
        verified->confirmed.clear();
        verified->targets.clear();
    }
    if (R == 0 || W == 0 || N == 0) return;
    // --verify-frame-windows: the threshold follows from a window's stops (fw::stop_threshold) unless the A/B variable asks for §18's
    const char* thr_env = std::getenv("TETREX_FRAME_WINDOW_THRESHOLD");
    const bool stop_rule = verified && !(thr_env && std::string(thr_env) == "plain");
    const bool trace = std::getenv("TETREX_TRACE") != nullptr;
    // the record batches [cut[i], cut[i + 1]): at most 2^24 values by their bound, a larger record alone.  The buffers are sized
    // for the largest batch before the first one runs, so that no device memory of the call is freed or allocated between
    // its launches ("Host").
    const plan::Cuts cuts = cut_translate_batches(rec_offsets, k, 0);
    const std::vector<size_t>& cut = cuts.cut;
    uint64_t most_windows = 0;
    for (size_t c = 0; c + 1 < cut.size(); ++c) most_windows = std::max(most_windows, win_offsets[6 * cut[c + 1]] - win_offsets[6 * cut[c]]);
    const size_t most_records = cuts.most_items, sub_windows = (size_t)std::min<uint64_t>(most_windows, max_batch_windows(W, with_counts));
    DeviceBuffer d_codes(256), d_seq(cuts.most_bytes + 16), d_rec((most_records + 1) * 8), d_val(cuts.most_values * 8 + 8),
        d_off((6 * most_records + 1) * 8), d_woff((6 * most_records + 1) * 8), d_beg(most_windows * 8 + 8), d_len(most_windows * 4 + 8),
        d_thr(most_windows * 4 + 8), d_hit(sub_windows * W * 8), d_cnt;
    if (with_counts) d_cnt.reserve(sub_windows * W * 64 * 4);
    // --verify-frame-windows: the frames as letters (six frames of L bytes are below 2 L residues; 16 bytes of slack as
    // BinVerifier gives its own pattern buffer) and, per window, where its letters lie and its stops
    DeviceBuffer d_frames, d_foff, d_lbeg, d_llen, d_stops;
    if (verified) {
        d_frames.reserve(2 * cuts.most_bytes + 16);
        d_foff.reserve((6 * most_records + 1) * 8);
        d_lbeg.reserve(most_windows * 8 + 8);
        d_llen.reserve(most_windows * 4 + 8);
        d_stops.reserve(most_windows * 4 + 8);
    }
    txq_check(txq_memcpy_h2d(d_codes.p, enc_.aa_table().data(), 256), "h2d");
    HitLister lister;
    std::vector<uint64_t> rebased;
    std::vector<uint32_t> thr, lengths;
    std::vector<BinVerifier::Candidate> candidates;
    std::vector<VerifiedHit> batch_confirmed;
    std::vector<std::vector<VerifiedHit>> batch_targets;
    const uint32_t bin0 = (uint32_t)(info_.shard_word0 * 64);
    for (size_t c = 0; c + 1 < cut.size(); ++c) {
        const size_t r0 = cut[c], r1 = cut[c + 1], nr = r1 - r0;
        const uint64_t w0 = win_offsets[6 * r0], nw = win_offsets[6 * r1] - w0;
        if (nw == 0) continue;
        upload_records(seq, rec_offsets, r0, r1, d_seq, d_rec, rebased);
        txq_check(txq_translate_windows_device((const uint8_t*)d_seq.p, (const uint64_t*)d_rec.p, nr, k, (const uint8_t*)d_codes.p, window, step,
                                               (uint64_t*)d_val.p, (uint64_t*)d_off.p, (uint64_t*)d_woff.p, (uint64_t*)d_beg.p, (uint32_t*)d_len.p, nullptr),
                  "txq_translate_windows_device");
        uint64_t frames_bytes = 0;
        if (verified) {  // the frames of the same bytes, then every window's letters, stops and threshold: nothing comes back in between
            frames_bytes = txq_translate_frames_bound(rebased.data(), nr);
            if (frames_bytes == UINT64_MAX || frames_bytes > 2 * cuts.most_bytes) txq_check(TXQ_ERR_ARG, "txq_translate_frames_bound");
            txq_check(txq_translate_frames_device((const uint8_t*)d_seq.p, (const uint64_t*)d_rec.p, nr, (uint8_t*)d_frames.p, frames_bytes,
                                                  (uint64_t*)d_foff.p, nullptr), "txq_translate_frames_device");
            txq_check(txq_frame_window_letters_device((const uint64_t*)d_rec.p, nr, k, window, step, (const uint8_t*)d_frames.p, frames_bytes,
                                                      (const uint64_t*)d_foff.p, (const uint64_t*)d_woff.p, (const uint32_t*)d_len.p, nw, verified->edits,
                                                      (uint64_t*)d_lbeg.p, (uint32_t*)d_llen.p, (uint32_t*)d_stops.p, (uint32_t*)d_thr.p, nullptr),
                      "txq_frame_window_letters_device");
        }
        txq_check(txq_memcpy_d2h(lens.data() + w0, d_len.p, nw * 4), "d2h");
        if (verified) txq_check(txq_memcpy_d2h(verified->stops.data() + w0, d_stops.p, nw * 4), "d2h");
        thr.resize(nw);
        bool any = false;
        for (uint64_t j = 0; j < nw; ++j) {
            const uint64_t w = lens[w0 + j];
            // (with the stop rule this is what the device wrote into d_thr: the same function of the same two numbers)
            thr[j] = stop_rule ? txq::fw::stop_threshold((uint32_t)w, verified->stops[w0 + j], k, verified->edits) : device_threshold(w ? threshold_of(w) : 0);
            if (thr[j] != 0xFFFFFFFFu) thresholds[w0 + j] = thr[j], any = true;
        }
        if (!any) continue;
        if (!stop_rule) txq_check(txq_memcpy_h2d(d_thr.p, thr.data(), nw * 4), "h2d");
        const size_t h0 = hits.size();
        // sub-ranges of the batch's windows: the begins are absolute in the batch's values, so nothing is sent again
        for (uint64_t j0 = 0; j0 < nw; j0 += sub_windows) {
            const size_t n = (size_t)std::min<uint64_t>(sub_windows, nw - j0);
            bool some = false;
            for (size_t j = 0; j < n && !some; ++j) some = thr[j0 + j] != 0xFFFFFFFFu;
            if (!some) continue;
            txq_check(txq_count_windows_device(ix_, (const uint64_t*)d_val.p, (const uint64_t*)d_beg.p + j0, (const uint32_t*)d_len.p + j0, n,
                                               (const uint32_t*)d_thr.p + j0, (uint64_t*)d_hit.p, with_counts ? (uint32_t*)d_cnt.p : nullptr, nullptr),
                      "txq_count_windows_device");
            const uint64_t total = lister.run(d_hit, with_counts ? &d_cnt : nullptr, n, W, (uint32_t)(w0 + j0), bin0, hits);
            if (trace)
                std::fprintf(stderr, "[tetrex search] frame window batch: records %zu..%zu, windows %llu..%llu, %llu hits\n", r0, r1,
                             (unsigned long long)(w0 + j0), (unsigned long long)(w0 + j0 + n), (unsigned long long)total);
        }
        if (!verified) continue;
        // --verify-frame-windows: the batch's hits are candidates, window index = the window's index within the batch
        verified->confirmed.resize(hits.size());
        if (verified->all_targets) verified->targets.resize(hits.size());
        if (hits.size() == h0) continue;
        candidates.clear();
        lengths.clear();
        const auto frame_of = [&](uint64_t j) { return (size_t)(std::upper_bound(win_offsets.begin(), win_offsets.end(), j) - win_offsets.begin()) - 1; };
        const auto residues_of = [&](uint64_t j, size_t q) {  // window j of the call, in frame q
            const uint64_t L = rec_offsets[q / 6 + 1] - rec_offsets[q / 6];
            return txq::fw::window_at(txq::fw::frame_plan(txq::tr::frame_len(L, (uint32_t)(q % 3)), k, window, step), j - win_offsets[q]);
        };
        for (size_t h = h0; h < hits.size(); ++h) {
            candidates.push_back({(uint32_t)(hits[h].query - w0), hits[h].bin});
            lengths.push_back((uint32_t)residues_of(hits[h].query, frame_of(hits[h].query)).len);
        }
        size_t held = ~(size_t)0;  // the frame translated last: the host routes ask for windows in ascending order
        std::string held_letters;
        const auto window_letters = [&](uint32_t j) {
            const size_t q = frame_of(w0 + j);
            if (q != held) {
                held_letters = translate_frame(seq.substr(rec_offsets[q / 6], rec_offsets[q / 6 + 1] - rec_offsets[q / 6]), (unsigned)(q % 6));
                held = q;
            }
            const txq::fw::Window at = residues_of(w0 + j, q);
            return held_letters.substr(at.a, at.len);
        };
        verified->verifier->verify_windows(BinVerifier::DeviceWindows{(const uint8_t*)d_frames.p, frames_bytes, (const uint64_t*)d_lbeg.p,
                                                                      (const uint32_t*)d_llen.p, (size_t)nw},
                                           candidates, lengths, window_letters, batch_confirmed, verified->all_targets ? &batch_targets : nullptr);
        std::move(batch_confirmed.begin(), batch_confirmed.end(), verified->confirmed.begin() + (long)h0);
        if (verified->all_targets) std::move(batch_targets.begin(), batch_targets.end(), verified->targets.begin() + (long)h0);
        if (verified->all_targets && verified->select_rows) {  // --window-targets --align-windows: the selected rows
            std::vector<BinVerifier::Selected> selection;
            for (const auto& [h, t] : verified->select_rows(h0, hits.size())) {
                if (h < h0 || h >= hits.size() || t >= verified->targets[h].size()) throw std::runtime_error("search_translated_windows: a selected row is not of the batch");
                selection.push_back({h - h0, &verified->targets[h][t]});
            }
            verified->verifier->align_windows(candidates, selection);
        } else if (verified->select) {  // --align-windows: the selected hits, while the batch's frames are still on the device
            std::vector<BinVerifier::Selected> selection;
            for (const size_t h : verified->select(h0, hits.size())) {
                if (h < h0 || h >= hits.size()) throw std::runtime_error("search_translated_windows: a selected hit is not of the batch");
                selection.push_back({h - h0, &verified->confirmed[h]});
            }
            verified->verifier->align_windows(candidates, selection);
        }
    }
}

}  // namespace tetrex
