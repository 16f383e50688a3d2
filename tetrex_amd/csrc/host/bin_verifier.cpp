#include "bin_verifier.hpp"
#include "device_buffer.hpp"
#include "edit_distance.hpp"
#include "fasta.hpp"

#include <algorithm>
#include <cstdlib>
#include <numeric>
#include <stdexcept>
#include <tuple>

namespace tetrex {

ResidentBins::ResidentBins(const std::vector<std::string>& bin_paths, std::string who)
    : paths_(bin_paths), who_(std::move(who)), bins_(bin_paths.size()) {
    const char* mb = std::getenv("TETREX_VERIFY_TEXT_MB");
    const double mib = mb && *mb ? std::atof(mb) : 4096.0;  // (a fraction is allowed: tests bound the cache to one bin)
    limit_bytes_ = (uint64_t)std::max(1.0, std::min(mib, 1e9) * 1048576.0);
}

ResidentBins::~ResidentBins() {
    for (Bin& b : bins_) drop(b);
}

void ResidentBins::drop(Bin& b) {
    if (b.d_text) txq_free(b.d_text);  // (waits for the kernels that read it)
    if (b.d_rec) txq_free(b.d_rec);
    b.d_text = b.d_rec = nullptr;
    held_bytes_ -= b.device_bytes;
    b.device_bytes = 0;
}

void ResidentBins::read(uint32_t bin, std::string& text, std::vector<uint64_t>& rec, std::vector<std::string>& names) const {
    text.clear();
    rec.assign(1, 0);
    names.clear();
    try {
        for_each_record(paths_[bin], [&](const FastaRecord& r) {
            names.push_back(r.name);
            text.append(r.seq);
            rec.push_back(text.size());
        });
    } catch (const std::exception& e) {
        throw std::runtime_error(who_ + ": cannot read bin file " + paths_[bin] + ": " + e.what());
    }
}

void ResidentBins::read_keeping_names(uint32_t bin, std::string& text, std::vector<uint64_t>& rec) {
    std::vector<std::string> names;
    read(bin, text, rec, names);
    if (bins_[bin].names.empty()) bins_[bin].names = std::move(names);
}

ResidentBins::Bin& ResidentBins::resident(uint32_t bin) {
    Bin& b = bins_[bin];
    if (b.d_rec) { b.last_use = ++clock_; return b; }
    std::string text;
    std::vector<uint64_t> rec;
    std::vector<std::string> names;
    read(bin, text, rec, names);
    return resident(bin, text, rec, names);
}

ResidentBins::Bin& ResidentBins::resident(uint32_t bin, const std::string& text, std::vector<uint64_t>& rec, std::vector<std::string>& names) {
    Bin& b = bins_[bin];
    b.last_use = ++clock_;
    if (b.d_rec) return b;
    // (a bin that left the device and comes back keeps the names it has: they are the same, and confirmed rows point into them)
    if (b.names.empty()) b.names = std::move(names);
    const uint64_t n = rec.size() - 1;
    rec.push_back(0);  // behind the record offsets: the one group's offsets {0, n}
    rec.push_back(n);
    const uint64_t bytes = bytes_on_device(text.size(), n);
    while (held_bytes_ && held_bytes_ + bytes > limit_bytes_) {  // the bin used longest ago leaves
        Bin* oldest = nullptr;
        for (Bin& o : bins_)
            if (o.d_rec && &o != &b && (!oldest || o.last_use < oldest->last_use)) oldest = &o;
        if (!oldest) break;
        drop(*oldest);
    }
    txq_check(txq_malloc(&b.d_text, text.size() + 16), "txq_malloc");
    txq_check(txq_malloc(&b.d_rec, rec.size() * 8), "txq_malloc");
    b.device_bytes = bytes;
    held_bytes_ += bytes;
    if (!text.empty()) txq_check(txq_memcpy_h2d(b.d_text, text.data(), text.size()), "h2d");
    txq_check(txq_memcpy_h2d(b.d_rec, rec.data(), rec.size() * 8), "h2d");
    b.n_records = n;
    b.text_bytes = text.size();
    return b;
}

// ---- tetrex search --verify --------------------------------------------------------------------------------------------

BinVerifier::BinVerifier(const std::vector<std::string>& bin_paths, bool dna, uint32_t errors)
    : bins_(bin_paths, "tetrex search --verify"), dna_(dna), errors_(errors) {
    std::fill(codes_, codes_ + 256, (uint8_t)255);
    if (dna) {
        const char* acgt = "ACGT";
        for (uint8_t c = 0; c < 4; ++c) codes_[(uint8_t)acgt[c]] = codes_[(uint8_t)(acgt[c] | 0x20)] = c;
        codes_[(uint8_t)'U'] = codes_[(uint8_t)'u'] = 3;
    } else {
        for (uint8_t c = 0; c < 26; ++c) codes_[(uint8_t)('A' + c)] = codes_[(uint8_t)('a' + c)] = c;
    }
    txq_check(txq_malloc(&d_codes_, 256), "txq_malloc");
    txq_check(txq_memcpy_h2d(d_codes_, codes_, 256), "h2d");
}

BinVerifier::~BinVerifier() {
    if (d_codes_) txq_free(d_codes_);
}

size_t BinVerifier::device_max() {
    const char* long_env = std::getenv("TETREX_VERIFY_LONG");
    return long_env && long_env[0] == '0' && !long_env[1] ? TXQ_EDIT_MAX_PATTERN : TXQ_EDIT_LONG_MAX_PATTERN;
}

namespace {
uint64_t target_slot_budget();  // (defined with run_targets below)
// TETREX_VERIFY_TARGETS=host: run_targets answers every pair on the host, so every window is written out for it
bool window_targets_on_host() {
    const char* e = std::getenv("TETREX_VERIFY_TARGETS");
    return e && std::string(e) == "host";
}
std::string reverse_complement(const std::string& s) {
    std::string out(s.rbegin(), s.rend());
    for (char& c : out) switch (c & 0xDF) {
        case 'A': c = 'T'; break;
        case 'C': c = 'G'; break;
        case 'G': c = 'C'; break;
        case 'T': case 'U': c = 'A'; break;
        default: c = 'N'; break;  // (no class: matches nothing, as the byte it stands for)
    }
    return out;
}
}  // namespace

void BinVerifier::verify(const std::vector<std::string>& queries, const std::vector<Candidate>& candidates, std::vector<Hit>& hits,
                         std::vector<std::vector<Hit>>* rows) {
    hits.assign(candidates.size(), Hit{});
    if (rows) rows->assign(candidates.size(), {});
    if (candidates.empty()) return;
    const size_t strands = dna_ ? 2 : 1;
    // the patterns: every record that is a candidate somewhere, and on a nucleotide index its reverse complement behind it
    constexpr uint32_t kNoPattern = 0xFFFFFFFFu;
    std::vector<uint32_t> pattern_of(queries.size(), kNoPattern), of_candidate(candidates.size(), kNoPattern);
    std::vector<uint64_t> pat_off{0}, lengths(candidates.size());
    std::string pat;
    const size_t longest = device_max();
    for (size_t i = 0; i < candidates.size(); ++i) {
        const uint32_t q = candidates[i].query;
        const std::string& s = queries.at(q);
        lengths[i] = s.size();
        if (s.empty() || s.size() > longest) continue;  // (the host route: letters() below)
        if (pattern_of[q] == kNoPattern) {
            pattern_of[q] = (uint32_t)(pat_off.size() - 1);
            pat.append(s);
            pat_off.push_back(pat.size());
            if (dna_) {
                pat.append(reverse_complement(s));
                pat_off.push_back(pat.size());
            }
        }
        of_candidate[i] = pattern_of[q];
    }
    DeviceBuffer d_pat(pat.size() + 16), d_po(pat_off.size() * 8);
    if (!pat.empty()) {
        txq_check(txq_memcpy_h2d(d_pat.p, pat.data(), pat.size()), "h2d");
        txq_check(txq_memcpy_h2d(d_po.p, pat_off.data(), pat_off.size() * 8), "h2d");
    }
    run(DevicePatterns{(const uint8_t*)d_pat.p, (const uint64_t*)d_po.p, pat_off.size() - 1, pat.size()}, strands, candidates, of_candidate, lengths,
        [&](size_t i, size_t strand) { return strand ? reverse_complement(queries[candidates[i].query]) : queries[candidates[i].query]; }, hits, rows);
}

void BinVerifier::verify(const DevicePatterns& patterns, const std::vector<Candidate>& candidates, const std::vector<uint64_t>& lengths,
                         const std::function<std::string(uint32_t)>& letters, std::vector<Hit>& hits, std::vector<std::vector<Hit>>* rows) {
    hits.assign(candidates.size(), Hit{});
    if (rows) rows->assign(candidates.size(), {});
    if (candidates.empty()) return;
    std::vector<uint32_t> of_candidate(candidates.size());
    for (size_t i = 0; i < candidates.size(); ++i) of_candidate[i] = candidates[i].query;
    run(patterns, 1, candidates, of_candidate, lengths, [&](size_t i, size_t) { return letters(candidates[i].query); }, hits, rows);
}

namespace {
// each(bin, a, b) for every maximal run [a, b) of positions in [begin, end) with the same bin_at(position)
template <class BinAt, class Each>
void for_each_bin_run(size_t begin, size_t end, BinAt&& bin_at, Each&& each) {
    for (size_t a = begin; a < end;) {
        size_t b = a;
        const uint32_t bin = bin_at(a);
        while (b < end && bin_at(b) == bin) ++b;
        each(bin, a, b);
        a = b;
    }
}
}  // namespace

BinVerifier::Routes BinVerifier::split_routes(const std::vector<Candidate>& candidates, const std::vector<uint64_t>& lengths, bool all_on_host) const {
    Routes r;
    r.order.resize(candidates.size());
    std::iota(r.order.begin(), r.order.end(), (size_t)0);
    std::stable_sort(r.order.begin(), r.order.end(), [&](size_t x, size_t y) { return candidates[x].bin < candidates[y].bin; });
    // (TETREX_VERIFY_LONG=0: what the long-pattern kernels would answer goes to the host, for A/B runs)
    const size_t longest = device_max();
    std::vector<size_t> on_long;
    for (size_t i : r.order) {
        if (all_on_host || lengths[i] == 0 || lengths[i] > longest) r.on_host.push_back(i);
        else (lengths[i] > TXQ_EDIT_MAX_PATTERN ? on_long : r.on_device).push_back(i);
    }
    r.n_short = r.on_device.size();
    r.on_device.insert(r.on_device.end(), on_long.begin(), on_long.end());
    return r;
}

BinVerifier::AlignRoute BinVerifier::align_route() const {
    const char* align_env = std::getenv("TETREX_VERIFY_ALIGN");
    const uint32_t device_errors = std::min<uint32_t>(errors_, TXQ_EDIT_ALIGN_MAX_DISTANCE);
    return {align_ && !(align_env && std::string(align_env) == "host"), device_errors, TXQ_EDIT_ALIGN_STRIDE(device_errors)};
}

void BinVerifier::align_on_host(uint32_t bin, const PendingAlign* pairs, size_t n, const std::string& text, const std::vector<uint64_t>& rec,
                                const Letters& letters) {
    bool failed = false;
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic)
#endif
    for (size_t k = 0; k < n; ++k) {
        const PendingAlign& p = pairs[k];
        const std::string pattern = letters(p.candidate, p.strand);
        EditAlignment a;
        if (p.r + 1 >= rec.size() ||
            !edit_align((const uint8_t*)pattern.data(), pattern.size(), (const uint8_t*)text.data() + rec[p.r], (size_t)(rec[p.r + 1] - rec[p.r]), p.d, p.j, codes_, a)) {
#ifdef _OPENMP
#pragma omp atomic write
#endif
            failed = true;
            continue;
        }
        p.into->start = a.start;
        p.into->runs = std::move(a.runs);
    }
    if (failed) throw std::runtime_error("tetrex search --align: a confirmed pair has no alignment (bin " + std::to_string(bin) + ")");
    n_align_host_ += n;
}

void BinVerifier::align_rest(std::vector<PendingAlign>& pending, const std::vector<Candidate>& candidates, const Letters& letters) {
    std::stable_sort(pending.begin(), pending.end(), [&](const PendingAlign& x, const PendingAlign& y) { return candidates[x.candidate].bin < candidates[y.candidate].bin; });
    for_each_bin_run(0, pending.size(), [&](size_t k) { return candidates[pending[k].candidate].bin; }, [&](uint32_t bin, size_t a, size_t b) {
        std::string text;
        std::vector<uint64_t> rec;
        bins_.read_keeping_names(bin, text, rec);
        align_on_host(bin, pending.data() + a, b - a, text, rec, letters);
    });
}

void BinVerifier::run(const DevicePatterns& patterns, size_t strands, const std::vector<Candidate>& candidates, const std::vector<uint32_t>& pattern_of,
                      const std::vector<uint64_t>& lengths, const Letters& letters, std::vector<Hit>& hits, std::vector<std::vector<Hit>>* rows) {
    if (rows) return run_targets(patterns, strands, candidates, pattern_of, lengths, letters, *rows);
    n_candidates_ += candidates.size();
    const Routes routes = split_routes(candidates, lengths, false);
    const std::vector<size_t>&on_device = routes.on_device, &on_host = routes.on_host;
    const size_t n_short = routes.n_short;
    n_device_ += n_short, n_device_long_ += on_device.size() - n_short, n_host_ += on_host.size();
    // take the better strand of `strands` results (distance, record, end); + wins on equal distance.  Returns that strand, or
    // `strands` where neither is within the cap.
    const auto settle = [&](size_t i, const uint32_t* res, const std::vector<std::string>& names) {
        Hit& h = hits[i];
        size_t kept = strands;
        for (size_t s = 0; s < strands; ++s)
            if (res[3 * s] != kEditNone && (h.distance == kEditNone || res[3 * s] < h.distance)) {
                h.distance = res[3 * s];
                h.target = &names.at(res[3 * s + 1]);
                h.end = res[3 * s + 2];
                h.strand = s ? '-' : '+';
                kept = s;
            }
        if (h.distance != kEditNone) ++n_confirmed_;
        return kept;
    };
    // --align: the alignment of the strand that settle kept.  What the device declines waits in `pending` for the host twin.
    const AlignRoute align = align_route();
    const size_t stride = align.stride;
    std::vector<PendingAlign> pending;
    if (!on_device.empty()) {
        std::vector<uint32_t> pairs;
        pairs.reserve(on_device.size() * strands * 3);
        for (size_t i : on_device)
            for (size_t s = 0; s < strands; ++s) pairs.insert(pairs.end(), {pattern_of[i] + (uint32_t)s, 0u, errors_});
        // (the alignments lie behind the triples: one buffer, one copy back)
        const size_t n_pairs = pairs.size() / 3, align_words = align.on_device ? n_pairs * stride : 0;
        DeviceBuffer d_pairs(pairs.size() * 4), d_out((pairs.size() + align_words) * 4);
        uint32_t* const d_align = (uint32_t*)d_out.p + pairs.size();
        static_assert(TXQ_EDIT_LONG_WORKSPACE(7) == TXQ_EDIT_WORKSPACE(7), "one workspace, cut the same way for either call");
        DeviceBuffer d_work(TXQ_EDIT_WORKSPACE(pairs.size() / 3) + 8 * on_device.size());  // (every call its own part: they are all in flight at once)
        size_t n_calls = 0;
        txq_check(txq_memcpy_h2d(d_pairs.p, pairs.data(), pairs.size() * 4), "h2d");
        for (int is_long = 0; is_long < 2; ++is_long)  // one call per bin and kernel: the bin's records are one group
            for_each_bin_run(is_long ? n_short : 0, is_long ? on_device.size() : n_short, [&](size_t k) { return candidates[on_device[k]].bin; }, [&](uint32_t bin, size_t a, size_t b) {
                ResidentBins::Bin& e = bins_.resident(bin);
                const uint64_t* d_rec = (const uint64_t*)e.d_rec;
                txq_check((is_long ? txq_edit_search_long_device : txq_edit_search_device)(patterns.d_letters, patterns.d_offsets, patterns.n_patterns, patterns.bytes, (const uint8_t*)e.d_text, d_rec,
                                                 e.n_records, e.text_bytes, d_rec + e.n_records + 1, 1, (const uint32_t*)d_pairs.p + 3 * strands * a,
                                                 (b - a) * strands, (const uint8_t*)d_codes_, (uint32_t*)d_out.p + 3 * strands * a,
                                                 (unsigned char*)d_work.p + 16 * strands * a + 8 * n_calls++, nullptr),
                          is_long ? "txq_edit_search_long_device" : "txq_edit_search_device");
                if (align.on_device)  // behind the search call on its stream: the triples are read where it left them
                    txq_check(txq_edit_align_device(patterns.d_letters, patterns.d_offsets, patterns.n_patterns, patterns.bytes, (const uint8_t*)e.d_text, d_rec,
                                                    e.n_records, e.text_bytes, d_rec + e.n_records + 1, 1, (const uint32_t*)d_pairs.p + 3 * strands * a,
                                                    (b - a) * strands, (const uint32_t*)d_out.p + 3 * strands * a, (const uint8_t*)d_codes_, align.device_errors,
                                                    d_align + stride * strands * a, nullptr, nullptr),
                              "txq_edit_align_device");
            });
        std::vector<uint32_t> out(pairs.size() + align_words);
        txq_check(txq_memcpy_d2h(out.data(), d_out.p, out.size() * 4), "d2h");  // (waits for the kernels)
        for (size_t k = 0; k < on_device.size(); ++k) {
            const uint32_t* res = out.data() + 3 * strands * k;
            const size_t i = on_device[k], kept = settle(i, res, bins_.at(candidates[i].bin).names);
            if (!align_ || kept == strands) continue;
            const uint32_t* words = out.data() + pairs.size() + stride * (strands * k + kept);
            if (align.on_device && words[0] < kEditNotAligned) {
                hits[i].start = words[0];
                hits[i].runs.assign(words + 2, words + 2 + words[1]);
                ++n_align_device_;
            } else pending.push_back({i, kept, res[3 * kept], res[3 * kept + 1], res[3 * kept + 2], &hits[i]});
        }
    }
    // records too long for the device: the bin is read once more, the pairs of a bin run side by side
    for_each_bin_run(0, on_host.size(), [&](size_t k) { return candidates[on_host[k]].bin; }, [&](uint32_t bin, size_t a, size_t b) {
        std::string text;
        std::vector<uint64_t> rec;
        bins_.read_keeping_names(bin, text, rec);
        std::vector<uint32_t> out(3 * strands * (b - a), kEditNone);
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic)
#endif
        for (size_t k = a; k < b; ++k) {
            if (lengths[on_host[k]] == 0) continue;
            for (size_t st = 0; st < strands; ++st) {
                const std::string p = letters(on_host[k], st);
                EditPattern ep((const uint8_t*)p.data(), p.size(), codes_);
                const EditResult r = edit_search_group(ep, (const uint8_t*)text.data(), rec.data(), 0, rec.size() - 1, errors_);
                uint32_t* o = out.data() + 3 * (strands * (k - a) + st);
                o[0] = r.distance, o[1] = r.record, o[2] = r.end;
            }
        }
        std::vector<PendingAlign> confirmed;
        for (size_t k = a; k < b; ++k) {
            const uint32_t* res = out.data() + 3 * strands * (k - a);
            const size_t kept = settle(on_host[k], res, bins_.at(bin).names);
            if (!align_ || kept == strands) continue;
            confirmed.push_back({on_host[k], kept, res[3 * kept], res[3 * kept + 1], res[3 * kept + 2], &hits[on_host[k]]});
        }
        align_on_host(bin, confirmed.data(), confirmed.size(), text, rec, letters);
    });
    align_rest(pending, candidates, letters);
}

// ---- tetrex search --window --verify-windows ---------------------------------------------------------------------------

void BinVerifier::verify_windows(const std::vector<std::string>& queries, const std::vector<Window>& windows, const std::vector<Candidate>& candidates,
                                 std::vector<Hit>& hits, std::vector<std::vector<Hit>>* rows) {
    hits.assign(candidates.size(), Hit{});
    if (rows) rows->assign(candidates.size(), {});
    const size_t strands = dna_ ? 2 : 1;
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    kept_.on_device = DeviceWindows{};
    kept_.strands = strands;
    kept_.entry_of.assign(candidates.size(), kNone);
    kept_.letters_of = [&queries, &windows, &candidates](size_t i, size_t strand) {
        const Window& w = windows[candidates[i].query];
        const std::string s = queries[w.record].substr(w.begin, w.len);
        return strand ? reverse_complement(s) : s;
    };
    if (candidates.empty()) return;
    const char* route_env = std::getenv("TETREX_VERIFY_WINDOWS");
    const bool all_written = (route_env && std::string(route_env) == "written") || (rows && window_targets_on_host());
    // by route: what the window kernel takes, and what is written out (longer windows; everything for an A/B run)
    std::vector<size_t> on_kernel, written;
    for (size_t i = 0; i < candidates.size(); ++i) {
        const Window& w = windows.at(candidates[i].query);
        if (w.begin + w.len > queries.at(w.record).size()) throw std::runtime_error("tetrex search --verify-windows: a window leaves its record");
        (all_written || w.len == 0 || w.len > TXQ_EDIT_MAX_PATTERN ? written : on_kernel).push_back(i);
    }
    const auto window_string = [&](uint32_t q) { return queries[windows[q].record].substr(windows[q].begin, windows[q].len); };
    if (rows) written_window_targets(written, windows.size(), candidates, window_string, *rows);
    else if (!written.empty()) {  // each distinct window becomes a string of its own: verify() and its routes, unchanged
        std::vector<uint32_t> string_of(windows.size(), kNone);
        std::vector<std::string> strings;
        std::vector<Candidate> as_records;
        for (size_t i : written) {
            const uint32_t q = candidates[i].query;
            if (string_of[q] == kNone) {
                string_of[q] = (uint32_t)strings.size();
                strings.push_back(queries[windows[q].record].substr(windows[q].begin, windows[q].len));
            }
            as_records.push_back({string_of[q], candidates[i].bin});
        }
        std::vector<Hit> answers;
        verify(strings, as_records, answers);
        for (size_t k = 0; k < written.size(); ++k) hits[written[k]] = std::move(answers[k]);
    }
    if (on_kernel.empty()) return;
    if (!rows) n_candidates_ += on_kernel.size(), n_windows_ += on_kernel.size();  // (with rows: run_window_targets counts what it answers)
    // by bin, and by window within the bin: the windows of a record that hit a bin are consecutive pairs, which walk together
    std::stable_sort(on_kernel.begin(), on_kernel.end(), [&](size_t x, size_t y) {
        return std::tie(candidates[x].bin, candidates[x].query) < std::tie(candidates[y].bin, candidates[y].query);
    });
    // the letters: every record with a candidate once, on a nucleotide index its reverse complement behind it; the windows
    // that are candidates as (begin, length) into them, `strands` entries each
    std::vector<uint64_t> base_of(queries.size(), ~0ull), win_begin;
    std::vector<uint32_t> entry_of(windows.size(), kNone), win_len;
    std::string letters;
    for (size_t i : on_kernel) {
        const uint32_t q = candidates[i].query;
        if (entry_of[q] != kNone) continue;
        const Window& w = windows[q];
        const std::string& s = queries[w.record];
        if (base_of[w.record] == ~0ull) {
            base_of[w.record] = letters.size();
            letters.append(s);
            if (dna_) letters.append(reverse_complement(s));
        }
        entry_of[q] = (uint32_t)win_begin.size();
        win_begin.push_back(base_of[w.record] + w.begin);
        win_len.push_back(w.len);
        if (dna_) {
            win_begin.push_back(base_of[w.record] + s.size() + (s.size() - w.begin - w.len));
            win_len.push_back(w.len);
        }
    }
    // (with keep_windows the buffers stay until the next call: align_windows reads the selected windows where they are)
    DeviceBuffer own_letters, own_begin, own_len;
    DeviceBuffer &d_letters = keep_windows_ ? kept_.letters : own_letters, &d_begin = keep_windows_ ? kept_.begin : own_begin,
                 &d_len = keep_windows_ ? kept_.len : own_len;
    d_letters.reserve(letters.size() + 16), d_begin.reserve(win_begin.size() * 8), d_len.reserve(win_len.size() * 4);
    txq_check(txq_memcpy_h2d(d_letters.p, letters.data(), letters.size()), "h2d");
    txq_check(txq_memcpy_h2d(d_begin.p, win_begin.data(), win_begin.size() * 8), "h2d");
    txq_check(txq_memcpy_h2d(d_len.p, win_len.data(), win_len.size() * 4), "h2d");
    kept_.on_device = DeviceWindows{(const uint8_t*)d_letters.p, letters.size(), (const uint64_t*)d_begin.p, (const uint32_t*)d_len.p, win_begin.size()};
    for (size_t i : on_kernel) kept_.entry_of[i] = entry_of[candidates[i].query];
    if (rows) return run_window_targets(kept_.on_device, strands, on_kernel, [&](size_t i) { return entry_of[candidates[i].query]; }, candidates, windows.size(), window_string, *rows);
    run_windows(kept_.on_device, strands, on_kernel, [&](size_t i) { return entry_of[candidates[i].query]; }, candidates, hits);
}

void BinVerifier::run_windows(const DeviceWindows& w, size_t strands, const std::vector<size_t>& on_kernel, const std::function<uint32_t(size_t)>& entry_of,
                              const std::vector<Candidate>& candidates, std::vector<Hit>& hits) {
    std::vector<uint32_t> pairs;
    pairs.reserve(on_kernel.size() * strands * 3);
    for (size_t i : on_kernel)
        for (size_t s = 0; s < strands; ++s) pairs.insert(pairs.end(), {entry_of(i) + (uint32_t)s, 0u, errors_});
    const size_t n_pairs = pairs.size() / 3;
    DeviceBuffer d_pairs(pairs.size() * 4), d_out(pairs.size() * 4);
    DeviceBuffer d_work(TXQ_EDIT_WINDOWS_WORKSPACE(n_pairs) + 8 * on_kernel.size());  // (every call its own part: they are all in flight at once)
    txq_check(txq_memcpy_h2d(d_pairs.p, pairs.data(), pairs.size() * 4), "h2d");
    size_t n_calls = 0;
    for_each_bin_run(0, on_kernel.size(), [&](size_t k) { return candidates[on_kernel[k]].bin; }, [&](uint32_t bin, size_t a, size_t b) {
        ResidentBins::Bin& e = bins_.resident(bin);
        const uint64_t* d_rec = (const uint64_t*)e.d_rec;
        txq_check(txq_edit_windows_device(w.d_letters, w.bytes, w.d_begin, w.d_len, w.n_windows, (const uint8_t*)e.d_text, d_rec, e.n_records, e.text_bytes,
                                          d_rec + e.n_records + 1, 1, (const uint32_t*)d_pairs.p + 3 * strands * a, (b - a) * strands, (const uint8_t*)d_codes_,
                                          (uint32_t*)d_out.p + 3 * strands * a, (unsigned char*)d_work.p + 16 * strands * a + 8 * n_calls++, nullptr),
                  "txq_edit_windows_device");
    });
    std::vector<uint32_t> out(pairs.size());
    txq_check(txq_memcpy_d2h(out.data(), d_out.p, out.size() * 4), "d2h");  // (waits for the kernels)
    for (size_t k = 0; k < on_kernel.size(); ++k) {  // the better strand; + wins on equal distance
        const uint32_t* res = out.data() + 3 * strands * k;
        const size_t i = on_kernel[k];
        Hit& h = hits[i];
        const std::vector<std::string>& names = bins_.at(candidates[i].bin).names;
        for (size_t s = 0; s < strands; ++s) {
            if (res[3 * s] == kEditNone && res[3 * s + 1] == 0xFFFFFFFEu) throw std::runtime_error("tetrex search --verify-windows / --verify-frame-windows: the device refused a pair of bin " + std::to_string(candidates[i].bin));
            if (res[3 * s] != kEditNone && (h.distance == kEditNone || res[3 * s] < h.distance)) {
                h.distance = res[3 * s];
                h.target = &names.at(res[3 * s + 1]);
                h.end = res[3 * s + 2];
                h.strand = s ? '-' : '+';
            }
        }
        if (h.distance != kEditNone) ++n_confirmed_;
    }
}

// ---- tetrex search --translate --frame-window --verify-frame-windows ------------------------------------------------------

void BinVerifier::verify_windows(const DeviceWindows& windows, const std::vector<Candidate>& candidates, const std::vector<uint32_t>& lengths,
                                 const std::function<std::string(uint32_t)>& letters, std::vector<Hit>& hits, std::vector<std::vector<Hit>>* rows) {
    hits.assign(candidates.size(), Hit{});
    if (rows) rows->assign(candidates.size(), {});
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    kept_.on_device = windows;
    kept_.strands = 1;
    kept_.entry_of.assign(candidates.size(), kNone);
    kept_.letters_of = [&candidates, letters](size_t i, size_t) { return letters(candidates[i].query); };
    if (candidates.empty()) return;
    if (lengths.size() != candidates.size()) throw std::runtime_error("tetrex search --verify-frame-windows: candidates and lengths disagree");
    if (dna_) throw std::runtime_error("tetrex search --verify-frame-windows: translated windows have one strand, the verifier two");
    const char* route_env = std::getenv("TETREX_VERIFY_FRAME_WINDOWS");
    const bool all_written = (route_env && std::string(route_env) == "written") || (rows && window_targets_on_host());
    std::vector<size_t> on_kernel, written;
    for (size_t i = 0; i < candidates.size(); ++i) {
        if (candidates[i].query >= windows.n_windows) throw std::runtime_error("tetrex search --verify-frame-windows: a candidate names no window");
        (all_written || lengths[i] == 0 || lengths[i] > TXQ_EDIT_MAX_PATTERN ? written : on_kernel).push_back(i);
    }
    if (rows) written_window_targets(written, windows.n_windows, candidates, letters, *rows);
    else if (!written.empty()) {  // each distinct window becomes a string of its own, in window order: verify() and its routes, unchanged
        std::vector<size_t> by_window(written);
        std::stable_sort(by_window.begin(), by_window.end(), [&](size_t x, size_t y) { return candidates[x].query < candidates[y].query; });
        std::vector<uint32_t> string_of(windows.n_windows, kNone);
        std::vector<std::string> strings;
        for (size_t i : by_window) {
            const uint32_t q = candidates[i].query;
            if (string_of[q] != kNone) continue;
            string_of[q] = (uint32_t)strings.size();
            strings.push_back(letters(q));
        }
        std::vector<Candidate> as_records;
        for (size_t i : written) as_records.push_back({string_of[candidates[i].query], candidates[i].bin});
        std::vector<Hit> answers;
        verify(strings, as_records, answers);
        for (size_t k = 0; k < written.size(); ++k) hits[written[k]] = std::move(answers[k]);
    }
    if (on_kernel.empty()) return;
    if (!rows) n_candidates_ += on_kernel.size(), n_windows_ += on_kernel.size();  // (with rows: run_window_targets counts what it answers)
    // by bin, and by window within the bin: the windows of a frame that hit a bin are consecutive pairs, which walk together
    std::stable_sort(on_kernel.begin(), on_kernel.end(), [&](size_t x, size_t y) {
        return std::tie(candidates[x].bin, candidates[x].query) < std::tie(candidates[y].bin, candidates[y].query);
    });
    for (size_t i : on_kernel) kept_.entry_of[i] = candidates[i].query;
    if (rows) return run_window_targets(windows, 1, on_kernel, [&](size_t i) { return candidates[i].query; }, candidates, windows.n_windows, letters, *rows);
    run_windows(windows, 1, on_kernel, [&](size_t i) { return candidates[i].query; }, candidates, hits);
}

// ---- tetrex search --verify-windows / --verify-frame-windows --align-windows ------------------------------------------------

void BinVerifier::align_windows(const std::vector<Candidate>& candidates, const std::vector<Selected>& selection) {
    if (selection.empty()) return;
    if (!keep_windows_) throw std::runtime_error("tetrex search --align-windows: verify_windows was not asked to keep its windows");
    if (kept_.entry_of.size() != candidates.size()) throw std::runtime_error("tetrex search --align-windows: the candidates are not those of the last verify_windows call");
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    const char* align_env = std::getenv("TETREX_VERIFY_ALIGN");
    const bool on_device = !(align_env && std::string(align_env) == "host");
    const uint32_t device_errors = std::min<uint32_t>(errors_, TXQ_EDIT_ALIGN_MAX_DISTANCE);
    const size_t stride = TXQ_EDIT_ALIGN_STRIDE(device_errors);
    // a selected window as the pair the device aligns: its entry on the kept strand, and the triple (d, r, j) of its hit
    struct Sent {
        PendingAlign pair;
        uint32_t bin, entry;
    };
    std::vector<Sent> sent;
    std::vector<PendingAlign> pending;
    for (const Selected& x : selection) {
        if (x.candidate >= candidates.size() || !x.hit || x.hit->distance == kEditNone || !x.hit->target)
            throw std::runtime_error("tetrex search --align-windows: a selected window is not a confirmed candidate");
        const uint32_t bin = candidates[x.candidate].bin, entry = kept_.entry_of[x.candidate];
        const std::vector<std::string>& names = bins_.at(bin).names;
        const size_t r = (size_t)(x.hit->target - names.data()), strand = x.hit->strand == '-' ? 1 : 0;
        if (r >= names.size() || strand >= kept_.strands) throw std::runtime_error("tetrex search --align-windows: a hit that its bin did not give");
        const PendingAlign pair{x.candidate, strand, x.hit->distance, (uint32_t)r, x.hit->end, x.hit};
        if (on_device && entry != kNone && pair.d <= device_errors) sent.push_back({pair, bin, entry + (uint32_t)strand});
        else pending.push_back(pair);
    }
    std::stable_sort(sent.begin(), sent.end(), [](const Sent& x, const Sent& y) { return x.bin < y.bin; });
    // one round, sent[a, b) — whole bins, all resident: their views, the pairs and the triples go up, ONE call, one copy back
    const auto run_round = [&](size_t a, size_t b) {
        if (a == b) return;
        std::vector<txq_text_view> views;
        std::vector<uint32_t> pairs, triples;
        bool all_resident = true;
        for (size_t k = a; k < b; ++k) {
            if (k == a || sent[k].bin != sent[k - 1].bin) {
                all_resident = all_resident && bins_.is_resident(sent[k].bin);
                const ResidentBins::Bin& e = bins_.at(sent[k].bin);
                views.push_back({(const uint8_t*)e.d_text, (const uint64_t*)e.d_rec, e.n_records, e.text_bytes});
            }
            pairs.insert(pairs.end(), {sent[k].entry, (uint32_t)(views.size() - 1), errors_});
            triples.insert(triples.end(), {sent[k].pair.d, sent[k].pair.r, sent[k].pair.j});
        }
        if (!all_resident) {  // a bin left while a later one of the round came: the host answers the round
            for (size_t k = a; k < b; ++k) pending.push_back(sent[k].pair);
            return;
        }
        const size_t n = b - a;
        DeviceBuffer d_views(views.size() * sizeof(txq_text_view)), d_pairs(pairs.size() * 4), d_triples(triples.size() * 4), d_align(n * stride * 4);
        txq_check(txq_memcpy_h2d(d_views.p, views.data(), views.size() * sizeof(txq_text_view)), "h2d");
        txq_check(txq_memcpy_h2d(d_pairs.p, pairs.data(), pairs.size() * 4), "h2d");
        txq_check(txq_memcpy_h2d(d_triples.p, triples.data(), triples.size() * 4), "h2d");
        const DeviceWindows& w = kept_.on_device;
        txq_check(txq_edit_align_windows_device(w.d_letters, w.bytes, w.d_begin, w.d_len, w.n_windows, (const txq_text_view*)d_views.p, views.size(),
                                                (const uint32_t*)d_pairs.p, n, (const uint32_t*)d_triples.p, (const uint8_t*)d_codes_, device_errors,
                                                (uint32_t*)d_align.p, nullptr, nullptr),
                  "txq_edit_align_windows_device");
        ++n_align_windows_calls_;
        std::vector<uint32_t> words(n * stride);
        txq_check(txq_memcpy_d2h(words.data(), d_align.p, words.size() * 4), "d2h");  // (waits for the kernel)
        for (size_t k = 0; k < n; ++k) {
            const uint32_t* o = words.data() + stride * k;
            const PendingAlign& p = sent[a + k].pair;
            if (o[0] == kEditNone) throw std::runtime_error("tetrex search --align-windows: the device refused a pair of bin " + std::to_string(sent[a + k].bin));
            if (o[0] < kEditNotAligned) {
                p.into->start = o[0];
                p.into->runs.assign(o + 2, o + 2 + o[1]);
                ++n_align_device_;
            } else pending.push_back(p);
        }
    };
    // the rounds: bins in order while they fit the cache together.  A bin's bytes are known before it is uploaded (a bin that is
    // not resident is read first), so a round ends BEFORE the bin that would push one of its own out.
    size_t round_begin = 0;
    uint64_t round_bytes = 0;
    for_each_bin_run(0, sent.size(), [&](size_t k) { return sent[k].bin; }, [&](uint32_t bin, size_t a, size_t) {
        std::string text;
        std::vector<uint64_t> rec;
        std::vector<std::string> names;
        const bool there = bins_.is_resident(bin);
        if (!there) bins_.read(bin, text, rec, names);
        const uint64_t bytes = there ? bins_.at(bin).device_bytes : ResidentBins::bytes_on_device(text.size(), rec.size() - 1);
        if (a > round_begin && round_bytes + bytes > bins_.limit_bytes()) {
            run_round(round_begin, a);
            round_begin = a, round_bytes = 0;
        }
        if (there) bins_.resident(bin);
        else bins_.resident(bin, text, rec, names);
        round_bytes += bytes;
    });
    run_round(round_begin, sent.size());
    if (pending.empty()) return;
    // the host route: the windows as strings, made one after the other (the way to a frame window's letters keeps state), then
    // the pairs of a bin side by side
    std::stable_sort(pending.begin(), pending.end(), [](const PendingAlign& x, const PendingAlign& y) { return x.candidate < y.candidate; });
    std::vector<std::string> strings;
    std::vector<size_t> string_of(candidates.size() * kept_.strands, ~(size_t)0);
    for (const PendingAlign& p : pending) {
        size_t& at = string_of[p.candidate * kept_.strands + p.strand];
        if (at != ~(size_t)0) continue;
        at = strings.size();
        strings.push_back(kept_.letters_of(p.candidate, p.strand));
    }
    align_rest(pending, candidates, [&](size_t i, size_t strand) { return strings[string_of[i * kept_.strands + strand]]; });
}

// ---- tetrex search --verify-windows / --verify-frame-windows --window-targets -----------------------------------------------

void BinVerifier::written_window_targets(const std::vector<size_t>& which, size_t n_windows, const std::vector<Candidate>& candidates,
                                         const std::function<std::string(uint32_t)>& window_string, std::vector<std::vector<Hit>>& rows) {
    if (which.empty()) return;
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    // each distinct window becomes a string of its own, in window order (the way to a frame window's letters keeps state)
    std::vector<size_t> by_window(which);
    std::stable_sort(by_window.begin(), by_window.end(), [&](size_t x, size_t y) { return candidates[x].query < candidates[y].query; });
    std::vector<uint32_t> string_of(n_windows, kNone);
    std::vector<std::string> strings;
    for (size_t i : by_window) {
        const uint32_t q = candidates[i].query;
        if (string_of[q] != kNone) continue;
        string_of[q] = (uint32_t)strings.size();
        strings.push_back(window_string(q));
    }
    std::vector<Candidate> as_records;
    for (size_t i : which) as_records.push_back({string_of[candidates[i].query], candidates[i].bin});
    std::vector<Hit> none;
    std::vector<std::vector<Hit>> answers;
    verify(strings, as_records, none, &answers);
    for (size_t k = 0; k < which.size(); ++k) rows[which[k]] = std::move(answers[k]);
    n_wt_host_ += which.size();
}

void BinVerifier::run_window_targets(const DeviceWindows& w, size_t strands, const std::vector<size_t>& on_kernel, const std::function<uint32_t(size_t)>& entry_of,
                                     const std::vector<Candidate>& candidates, size_t n_windows, const std::function<std::string(uint32_t)>& window_string,
                                     std::vector<std::vector<Hit>>& rows) {
    const uint64_t budget = target_slot_budget();
    // what the rounds find: (record, strand, distance, end) of every hit of a candidate; settled below
    struct Found { uint32_t r, strand, d, j; };
    std::vector<std::vector<Found>> found(candidates.size());
    std::vector<size_t> answered, fallback;
    const auto bin_at = [&](size_t k) { return candidates[on_kernel[k]].bin; };
    // one round, on_kernel[a, b) — its bins all resident: their views and the pairs go up, ONE call, one wait, the rows written come back
    const auto run_round = [&](size_t a, size_t b) {
        if (a == b) return;
        std::vector<txq_text_view> views;
        std::vector<uint32_t> pairs;
        bool all_resident = true;
        uint64_t n_slots = 0;
        for (size_t k = a; k < b; ++k) {
            if (k == a || bin_at(k) != bin_at(k - 1)) {
                all_resident = all_resident && bins_.is_resident(bin_at(k));
                const ResidentBins::Bin& e = bins_.at(bin_at(k));
                views.push_back({(const uint8_t*)e.d_text, (const uint64_t*)e.d_rec, e.n_records, e.text_bytes});
            }
            for (size_t s = 0; s < strands; ++s) pairs.insert(pairs.end(), {entry_of(on_kernel[k]) + (uint32_t)s, (uint32_t)(views.size() - 1), errors_});
            n_slots += strands * views.back().n_records;
        }
        if (!all_resident) {  // a bin left while a later one of the round came: verify()'s routes answer the round
            fallback.insert(fallback.end(), on_kernel.begin() + (long)a, on_kernel.begin() + (long)b);
            return;
        }
        const size_t n_pairs = (b - a) * strands;
        DeviceBuffer d_views(views.size() * sizeof(txq_text_view)), d_pairs(pairs.size() * 4 + 4), d_hits(n_slots * 16 + 16), d_total(8), d_status(n_pairs * 4 + 4),
            d_work(TXQ_EDIT_WINDOW_TARGETS_WORKSPACE(n_pairs, n_slots) + 8);
        txq_check(txq_memcpy_h2d(d_views.p, views.data(), views.size() * sizeof(txq_text_view)), "h2d");
        txq_check(txq_memcpy_h2d(d_pairs.p, pairs.data(), pairs.size() * 4), "h2d");
        txq_check(txq_edit_window_targets_device(w.d_letters, w.bytes, w.d_begin, w.d_len, w.n_windows, (const txq_text_view*)d_views.p, views.size(),
                                                 (const uint32_t*)d_pairs.p, n_pairs, (const uint8_t*)d_codes_, (uint32_t*)d_hits.p, n_slots, (uint64_t*)d_total.p,
                                                 (uint32_t*)d_status.p, n_slots, d_work.p, nullptr),
                  "txq_edit_window_targets_device");
        ++n_wt_calls_;
        uint64_t total = 0;
        std::vector<uint32_t> status(n_pairs);
        txq_check(txq_memcpy_d2h(&total, d_total.p, 8), "d2h");  // (waits for the kernels)
        txq_check(txq_memcpy_d2h(status.data(), d_status.p, n_pairs * 4), "d2h");
        for (size_t p = 0; p < n_pairs; ++p)
            if (status[p] != 0) throw std::runtime_error("tetrex search --window-targets: the device refused a pair of bin " + std::to_string(bin_at(a + p / strands)));
        if (total > n_slots) throw std::runtime_error("tetrex search --window-targets: more hits than slots");
        std::vector<uint32_t> hits(4 * total);
        if (total) txq_check(txq_memcpy_d2h(hits.data(), d_hits.p, total * 16), "d2h");
        for (uint64_t h = 0; h < total; ++h) {
            const uint32_t* row = hits.data() + 4 * h;
            found[on_kernel[a + row[0] / strands]].push_back({row[2], (uint32_t)(row[0] % strands), row[1], row[3]});
        }
        answered.insert(answered.end(), on_kernel.begin() + (long)a, on_kernel.begin() + (long)b);
    };
    // the rounds: candidates in order while their bins fit the cache together and their slots the bound.  A bin's bytes and
    // records are known before it is uploaded (a bin that is not resident is read first), so a round ends BEFORE the bin that
    // would push one of its own out, and a bin of more records than a call's slots is never uploaded.
    size_t round_begin = 0;
    uint64_t round_bytes = 0, round_slots = 0;
    for_each_bin_run(0, on_kernel.size(), bin_at, [&](uint32_t bin, size_t a, size_t b) {
        std::string text;
        std::vector<uint64_t> rec;
        std::vector<std::string> names;
        const bool there = bins_.is_resident(bin);
        if (!there) bins_.read(bin, text, rec, names);
        const uint64_t n_records = there ? bins_.at(bin).n_records : rec.size() - 1;
        const uint64_t bytes = there ? bins_.at(bin).device_bytes : ResidentBins::bytes_on_device(text.size(), n_records);
        if (n_records > budget) {  // a single pair above the bound: run_targets sends it to the host
            run_round(round_begin, a);
            fallback.insert(fallback.end(), on_kernel.begin() + (long)a, on_kernel.begin() + (long)b);
            round_begin = b, round_bytes = round_slots = 0;
            return;
        }
        if (a > round_begin && round_bytes + bytes > bins_.limit_bytes()) {
            run_round(round_begin, a);
            round_begin = a, round_bytes = round_slots = 0;
        }
        if (there) bins_.resident(bin);
        else bins_.resident(bin, text, rec, names);
        round_bytes += bytes;
        for (size_t k = a; k < b; ++k) {  // (the pairs of one candidate stay in one round)
            if (k > round_begin && round_slots + strands * n_records > 8 * budget) {
                run_round(round_begin, k);
                round_begin = k, round_bytes = bytes, round_slots = 0;
            }
            round_slots += strands * n_records;
        }
    });
    run_round(round_begin, on_kernel.size());
    // settle: a target's row is its better strand, + on equal distance; rows in the order of the bin's file
    n_candidates_ += answered.size();
    n_wt_device_ += answered.size();
    for (size_t i : answered) {
        std::vector<Found>& f = found[i];
        std::sort(f.begin(), f.end(), [](const Found& x, const Found& y) { return std::tie(x.r, x.d, x.strand) < std::tie(y.r, y.d, y.strand); });
        const std::vector<std::string>& names = bins_.at(candidates[i].bin).names;
        for (size_t k = 0; k < f.size(); ++k) {
            if (k && f[k].r == f[k - 1].r) continue;
            Hit h;
            h.distance = f[k].d, h.end = f[k].j, h.strand = f[k].strand ? '-' : '+', h.target = &names.at(f[k].r);
            rows[i].push_back(std::move(h));
        }
        if (!rows[i].empty()) ++n_confirmed_;
        n_targets_ += rows[i].size();
    }
    written_window_targets(fallback, n_windows, candidates, window_string, rows);
}

// ---- tetrex search --verify --all-targets ------------------------------------------------------------------------------

namespace {
// slots of one txq_edit_targets*_device call (TETREX_VERIFY_TARGET_SLOTS, default 2^20: 8 MiB of keys and 16 MiB of rows)
uint64_t target_slot_budget() {
    const char* e = std::getenv("TETREX_VERIFY_TARGET_SLOTS");
    const long long v = e && *e ? std::atoll(e) : 1ll << 20;
    return (uint64_t)std::max<long long>(1, std::min<long long>(v, 1ll << 32));
}
}  // namespace

void BinVerifier::run_targets(const DevicePatterns& patterns, size_t strands, const std::vector<Candidate>& candidates, const std::vector<uint32_t>& pattern_of,
                              const std::vector<uint64_t>& lengths, const Letters& letters, std::vector<std::vector<Hit>>& rows) {
    rows.assign(candidates.size(), {});
    n_candidates_ += candidates.size();
    const char* route_env = std::getenv("TETREX_VERIFY_TARGETS");
    Routes routes = split_routes(candidates, lengths, route_env && std::string(route_env) == "host");
    const std::vector<size_t>& on_device = routes.on_device;
    std::vector<size_t>& on_host = routes.on_host;
    const uint64_t budget = target_slot_budget();
    // what the routes find: (record, strand, distance, end) of every hit of a candidate; settled below
    struct Found { uint32_t r, strand, d, j; };
    std::vector<std::vector<Found>> found(candidates.size());

    // the device: one call per bin, kernel and at most `budget` slots, queued in rounds with one copy back each
    struct Call { uint32_t bin; bool is_long; size_t first, n_pairs; uint64_t n_records; size_t row0, work0; };
    const auto run_round = [&](const std::vector<Call>& calls, const std::vector<uint32_t>& pairs, const std::vector<size_t>& owner, size_t n_rows, size_t work_bytes) {
        const size_t n_pairs = pairs.size() / 3;
        DeviceBuffer d_pairs(pairs.size() * 4 + 4), d_hits(n_rows * 16 + 16), d_total(calls.size() * 8), d_status(n_pairs * 4 + 4), d_work(work_bytes + 8);
        txq_check(txq_memcpy_h2d(d_pairs.p, pairs.data(), pairs.size() * 4), "h2d");
        for (size_t c = 0; c < calls.size(); ++c) {
            const Call& k = calls[c];
            ResidentBins::Bin& e = bins_.resident(k.bin);
            const uint64_t* d_rec = (const uint64_t*)e.d_rec;
            const size_t n_slots = k.n_pairs * k.n_records;
            txq_check((k.is_long ? txq_edit_targets_long_device : txq_edit_targets_device)(
                          patterns.d_letters, patterns.d_offsets, patterns.n_patterns, patterns.bytes, (const uint8_t*)e.d_text, d_rec, e.n_records, e.text_bytes,
                          d_rec + e.n_records + 1, 1, (const uint32_t*)d_pairs.p + 3 * k.first, k.n_pairs, (const uint8_t*)d_codes_,
                          (uint32_t*)d_hits.p + 4 * k.row0, n_slots, (uint64_t*)d_total.p + c, (uint32_t*)d_status.p + k.first, n_slots,
                          (unsigned char*)d_work.p + k.work0, nullptr),
                      k.is_long ? "txq_edit_targets_long_device" : "txq_edit_targets_device");
        }
        std::vector<uint32_t> hits, status(n_pairs + 1);
        std::vector<uint64_t> totals(calls.size());
        txq_check(txq_memcpy_d2h(totals.data(), d_total.p, totals.size() * 8), "d2h");  // (waits for the kernels)
        txq_check(txq_memcpy_d2h(status.data(), d_status.p, n_pairs * 4), "d2h");
        for (size_t p = 0; p < n_pairs; ++p)
            if (status[p] != 0) throw std::runtime_error("tetrex search --all-targets: the device refused a pair of bin " + std::to_string(candidates[owner[p / strands]].bin));
        // The rows: a call's area is as large as its slots, what was written is usually far less.  One copy of the round's whole
        // area where that is at most kOneCopyBytes; above it, only the rows that were written, call by call.
        constexpr size_t kOneCopyBytes = (size_t)4 << 20;
        const bool one_copy = n_rows * 16 <= kOneCopyBytes;
        if (one_copy && n_rows) {
            hits.resize(4 * n_rows);
            txq_check(txq_memcpy_d2h(hits.data(), d_hits.p, n_rows * 16), "d2h");
        }
        for (size_t c = 0; c < calls.size(); ++c) {
            const Call& k = calls[c];
            if (totals[c] > k.n_pairs * k.n_records) throw std::runtime_error("tetrex search --all-targets: more hits than slots");
            if (totals[c] == 0) continue;
            if (!one_copy) {
                hits.resize(4 * totals[c]);
                txq_check(txq_memcpy_d2h(hits.data(), (const uint32_t*)d_hits.p + 4 * k.row0, totals[c] * 16), "d2h");
            }
            for (uint64_t h = 0; h < totals[c]; ++h) {
                const uint32_t* row = hits.data() + 4 * ((one_copy ? k.row0 : 0) + h);
                const size_t pair = k.first + row[0];
                found[owner[pair / strands]].push_back({row[2], (uint32_t)(pair % strands), row[1], row[3]});
            }
        }
    };
    {
        std::vector<Call> calls;
        std::vector<uint32_t> pairs;
        std::vector<size_t> owner;  // the candidate of every `strands` pairs of the round
        size_t n_rows = 0, work_bytes = 0;
        const auto flush_round = [&]() {
            if (!calls.empty()) run_round(calls, pairs, owner, n_rows, work_bytes);
            calls.clear(), pairs.clear(), owner.clear();
            n_rows = work_bytes = 0;
        };
        for (int is_long = 0; is_long < 2; ++is_long)
            for_each_bin_run(is_long ? routes.n_short : 0, is_long ? on_device.size() : routes.n_short, [&](size_t k) { return candidates[on_device[k]].bin; }, [&](uint32_t bin, size_t a, size_t b) {
                // the bin's record count decides its route, so a bin that is not on the device is read first and uploaded only if it stays
                uint64_t n_records;
                if (bins_.is_resident(bin)) n_records = bins_.at(bin).n_records;
                else {
                    std::string text;
                    std::vector<uint64_t> rec;
                    std::vector<std::string> names;
                    bins_.read(bin, text, rec, names);
                    n_records = rec.size() - 1;
                    if (n_records <= budget) bins_.resident(bin, text, rec, names);
                }
                if (n_records > budget) {  // a single pair above the bound: the host
                    on_host.insert(on_host.end(), on_device.begin() + (long)a, on_device.begin() + (long)b);
                    return;
                }
                (is_long ? n_device_long_ : n_device_) += b - a;
                const size_t first = pairs.size() / 3;
                for (size_t k = a; k < b; ++k) {
                    owner.push_back(on_device[k]);
                    for (size_t s = 0; s < strands; ++s) pairs.insert(pairs.end(), {pattern_of[on_device[k]] + (uint32_t)s, 0u, errors_});
                }
                const size_t n_pairs = (b - a) * strands, per_call = (size_t)std::max<uint64_t>(1, n_records ? budget / n_records : n_pairs);
                for (size_t p = 0; p < n_pairs; p += per_call) {
                    const size_t np = std::min(per_call, n_pairs - p), n_slots = np * n_records;
                    calls.push_back({bin, is_long != 0, first + p, np, n_records, n_rows, work_bytes});
                    n_rows += n_slots;
                    work_bytes += TXQ_EDIT_TARGETS_WORKSPACE(np, n_slots);
                }
                // (pairs of one candidate stay in one round: a round ends between bins)
                if (n_rows >= 8 * budget) flush_round();
            });
        flush_round();
    }
    // the host: what is too long or empty, bins of more records than a call's slots, and with TETREX_VERIFY_TARGETS=host everything
    std::stable_sort(on_host.begin(), on_host.end(), [&](size_t x, size_t y) { return candidates[x].bin < candidates[y].bin; });
    n_host_ += on_host.size();
    for_each_bin_run(0, on_host.size(), [&](size_t k) { return candidates[on_host[k]].bin; }, [&](uint32_t bin, size_t a, size_t b) {
        std::string text;
        std::vector<uint64_t> rec;
        bins_.read_keeping_names(bin, text, rec);
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic)
#endif
        for (size_t k = a; k < b; ++k) {
            if (lengths[on_host[k]] == 0) continue;
            std::vector<uint32_t> quads;
            for (size_t st = 0; st < strands; ++st) {
                const std::string p = letters(on_host[k], st);
                EditPattern ep((const uint8_t*)p.data(), p.size(), codes_);
                quads.clear();
                edit_targets_group(ep, (const uint8_t*)text.data(), rec.data(), 0, rec.size() - 1, errors_, 0, quads);
                for (size_t h = 0; h < quads.size(); h += 4) found[on_host[k]].push_back({quads[h + 2], (uint32_t)st, quads[h + 1], quads[h + 3]});
            }
        }
    });
    // settle: a target's row is its better strand, + on equal distance; rows in the order of the bin's file
    struct ToAlign { size_t candidate, row; uint32_t strand, d, r, j; };
    std::vector<ToAlign> to_align;
    for (size_t i : routes.order) {
        std::vector<Found>& f = found[i];
        std::sort(f.begin(), f.end(), [](const Found& x, const Found& y) { return std::tie(x.r, x.d, x.strand) < std::tie(y.r, y.d, y.strand); });
        const std::vector<std::string>& names = bins_.at(candidates[i].bin).names;
        for (size_t k = 0; k < f.size(); ++k) {
            if (k && f[k].r == f[k - 1].r) continue;
            Hit h;
            h.distance = f[k].d, h.end = f[k].j, h.strand = f[k].strand ? '-' : '+', h.target = &names.at(f[k].r);
            if (align_) to_align.push_back({i, rows[i].size(), f[k].strand, f[k].d, f[k].r, f[k].j});
            rows[i].push_back(std::move(h));
        }
        if (!rows[i].empty()) ++n_confirmed_;
        n_targets_ += rows[i].size();
    }
    if (to_align.empty()) return;
    // --align: the rows that were kept, bin by bin (to_align is in bin order).  One txq_edit_align_device call per bin on pair and
    // triple arrays built here, after the copy back; what the device declines or cannot reach, on the host.
    const AlignRoute align = align_route();
    const size_t stride = align.stride;
    const auto on_host_later = [&](const ToAlign& x) { return PendingAlign{x.candidate, x.strand, x.d, x.r, x.j, &rows[x.candidate][x.row]}; };
    std::vector<PendingAlign> pending;
    std::vector<size_t> sent;
    for (size_t t = 0; t < to_align.size(); ++t) {
        const size_t i = to_align[t].candidate;
        const bool reachable = align.on_device && pattern_of[i] != 0xFFFFFFFFu && lengths[i] >= 1 && lengths[i] <= TXQ_EDIT_LONG_MAX_PATTERN &&
                               to_align[t].d <= align.device_errors;
        if (reachable) sent.push_back(t);
        else pending.push_back(on_host_later(to_align[t]));
    }
    if (!sent.empty()) {
        std::vector<uint32_t> pairs, triples;
        for (size_t t : sent) {
            const ToAlign& x = to_align[t];
            pairs.insert(pairs.end(), {pattern_of[x.candidate] + x.strand, 0u, errors_});
            triples.insert(triples.end(), {x.d, x.r, x.j});
        }
        DeviceBuffer d_pairs(pairs.size() * 4), d_triples(triples.size() * 4), d_align(sent.size() * stride * 4);
        txq_check(txq_memcpy_h2d(d_pairs.p, pairs.data(), pairs.size() * 4), "h2d");
        txq_check(txq_memcpy_h2d(d_triples.p, triples.data(), triples.size() * 4), "h2d");
        for_each_bin_run(0, sent.size(), [&](size_t k) { return candidates[to_align[sent[k]].candidate].bin; }, [&](uint32_t bin, size_t a, size_t b) {
            ResidentBins::Bin& e = bins_.resident(bin);
            const uint64_t* d_rec = (const uint64_t*)e.d_rec;
            txq_check(txq_edit_align_device(patterns.d_letters, patterns.d_offsets, patterns.n_patterns, patterns.bytes, (const uint8_t*)e.d_text, d_rec,
                                            e.n_records, e.text_bytes, d_rec + e.n_records + 1, 1, (const uint32_t*)d_pairs.p + 3 * a, b - a,
                                            (const uint32_t*)d_triples.p + 3 * a, (const uint8_t*)d_codes_, align.device_errors, (uint32_t*)d_align.p + stride * a,
                                            nullptr, nullptr),
                      "txq_edit_align_device");
        });
        std::vector<uint32_t> words(sent.size() * stride);
        txq_check(txq_memcpy_d2h(words.data(), d_align.p, words.size() * 4), "d2h");  // (waits for the kernels)
        for (size_t k = 0; k < sent.size(); ++k) {
            const uint32_t* w = words.data() + stride * k;
            const ToAlign& x = to_align[sent[k]];
            if (w[0] < kEditNotAligned) {
                rows[x.candidate][x.row].start = w[0];
                rows[x.candidate][x.row].runs.assign(w + 2, w + 2 + w[1]);
                ++n_align_device_;
            } else pending.push_back(on_host_later(x));
        }
    }
    align_rest(pending, candidates, letters);
}

}  // namespace tetrex
