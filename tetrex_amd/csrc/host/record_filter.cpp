#include "record_filter.hpp"
#include "device_buffer.hpp"
#include "matcher.hpp"
#include "regex_front.hpp"
#include "../../../include/txq_regex.h"

#include <algorithm>
#include <chrono>
#include <stdexcept>

namespace tetrex {

RecordFilter::RecordFilter(const std::vector<std::string>& bin_paths, const KmerEncoder& enc, int threads)
    : bins_(bin_paths, "tetrex query --gpu-verify"), enc_(enc), threads_(std::max(1, threads)) {}

void RecordFilter::run(const std::vector<const uint64_t*>& masks, uint64_t bins, const std::vector<std::string>& regexes, RecordSelection& out) {
    const bool dna = enc_.molecule() == Molecule::DNA;
    const bool reduced = !dna && enc_.alphabet() != Alphabet::Base;
    const size_t strands = dna ? 2 : 1, nq = regexes.size();
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_begin = now();
    // what verification does to a bin's text before the matcher sees it, folded into the automata's class tables
    uint8_t fwd_map[256], rev_map[256];
    for (unsigned b = 0; b < 256; ++b) {
        fwd_map[b] = reduced ? (uint8_t)enc_.reduce((unsigned char)b) : (uint8_t)b;
        rev_map[b] = (uint8_t)complement_base((char)b);
    }
    std::vector<std::vector<uint8_t>> blobs(nq * strands);
    std::vector<uint8_t> exported(nq, 0);
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic) num_threads(threads_)
#endif
    for (size_t q = 0; q < nq; ++q) {
        if (!masks[q]) continue;
        try {
            std::string pattern = regexes[q];
            if (reduced) pattern = reduce_query_alphabet(pattern, enc_.reduce_table());
            const Matcher m("(" + pattern + ")", dna ? Matcher::Semantics::LeftmostFirst : Matcher::Semantics::LeftmostLongest);
            exported[q] = m.export_dfa(false, fwd_map, blobs[q * strands]) && (!dna || m.export_dfa(true, rev_map, blobs[q * strands + 1]));
        } catch (const std::exception&) {
            exported[q] = 0;  // (a pattern the matcher refuses: verification says so, as without the flag)
        }
    }
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    std::vector<uint32_t> automaton_of(nq, kNone);
    std::vector<uint8_t> arena;
    std::vector<uint64_t> arena_off{0};
    for (size_t q = 0; q < nq; ++q) {
        if (!masks[q]) continue;
        if (!exported[q]) { ++stats_.automata_host; continue; }
        automaton_of[q] = (uint32_t)(arena_off.size() - 1);
        for (size_t s = 0; s < strands; ++s) {
            const std::vector<uint8_t>& b = blobs[q * strands + s];
            ++(b.size() <= 65536 ? stats_.automata_lds : stats_.automata_l2);
            arena.insert(arena.end(), b.begin(), b.end());  // (a blob's size is a multiple of 16)
            arena_off.push_back(arena.size());
        }
    }
    blobs.clear();
    stats_.export_seconds += now() - t_begin;
    // bin -> the motifs that selected it (ascending), as verify_batch walks them
    std::vector<std::vector<uint32_t>> wanted(bins);
    for (size_t q = 0; q < nq; ++q) {
        if (!masks[q]) continue;
        for (uint64_t w = 0; w * 64 < bins; ++w)
            for (uint64_t x = masks[q][w]; x; x &= x - 1) {
                const uint64_t b = w * 64 + (uint64_t)__builtin_ctzll(x);
                if (b >= bins || b >= bins_.size()) continue;
                if (automaton_of[q] == kNone) ++stats_.pairs_host;
                else wanted[b].push_back((uint32_t)q);
            }
    }
    std::vector<uint32_t> todo;
    for (uint64_t b = 0; b < bins; ++b)
        if (!wanted[b].empty()) todo.push_back((uint32_t)b);
    if (todo.empty()) return;
    const size_t n_automata = arena_off.size() - 1;
    DeviceBuffer d_arena(arena.size() + 16), d_arena_off(arena_off.size() * 8);
    txq_check(txq_memcpy_h2d(d_arena.p, arena.data(), arena.size()), "h2d");
    txq_check(txq_memcpy_h2d(d_arena_off.p, arena_off.data(), arena_off.size() * 8), "h2d");

    constexpr size_t kBlockBins = 256;  // bins read side by side, filtered, and copied back in one piece
    for (size_t b0 = 0; b0 < todo.size(); b0 += kBlockBins) {
        const size_t nb = std::min(kBlockBins, todo.size() - b0);
        const double t0 = now();
        std::vector<std::string> texts(nb);
        std::vector<std::vector<uint64_t>> recs(nb);
        std::vector<std::vector<std::string>> names(nb);
        std::string error;
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic) num_threads(threads_)
#endif
        for (size_t i = 0; i < nb; ++i) {
            if (bins_.is_resident(todo[b0 + i])) continue;
            try {
                bins_.read(todo[b0 + i], texts[i], recs[i], names[i]);
            } catch (const std::exception& e) {
#ifdef _OPENMP
#pragma omp critical
#endif
                error = e.what();
            }
        }
        if (!error.empty()) throw std::runtime_error(error);
        // the block's pairs, bin after bin: (automaton, group 0) per motif and strand; a bin's bitmaps are a region of their own
        std::vector<uint32_t> pairs;
        std::vector<uint64_t> out_off, pair0(nb + 1, 0), word0(nb + 1, 0), n_records(nb);
        for (size_t i = 0; i < nb; ++i) {
            const uint32_t bin = todo[b0 + i];
            n_records[i] = bins_.is_resident(bin) ? bins_.at(bin).n_records : recs[i].size() - 1;
            const uint64_t words = (n_records[i] + 31) / 32;
            uint64_t at = 0;
            for (uint32_t q : wanted[bin])
                for (size_t s = 0; s < strands; ++s) {
                    pairs.push_back(automaton_of[q] + (uint32_t)s);
                    pairs.push_back(0);
                    out_off.push_back(at);
                    at += words;
                }
            pair0[i + 1] = out_off.size();
            word0[i + 1] = word0[i] + at;
        }
        const size_t n_pairs = out_off.size(), n_words = word0[nb];
        DeviceBuffer d_pairs(n_pairs * 8 + 8), d_out_off(n_pairs * 8 + 8), d_out(n_words * 4 + 4), d_status(n_pairs * 4 + 4),
            d_work(TXQ_REGEX_WORKSPACE(n_pairs) + 8 * nb);  // (every call its own part: they are all in flight at once)
        txq_check(txq_memcpy_h2d(d_pairs.p, pairs.data(), n_pairs * 8), "h2d");
        txq_check(txq_memcpy_h2d(d_out_off.p, out_off.data(), n_pairs * 8), "h2d");
        double t_upload = now() - t0, t_filter = 0;
        for (size_t i = 0; i < nb; ++i) {  // one call per bin: its records are one group
            const double ta = now();
            if (recs[i].empty() && !bins_.is_resident(todo[b0 + i])) bins_.read(todo[b0 + i], texts[i], recs[i], names[i]);  // (it left for a bin of this block)
            ResidentBins::Bin& e = bins_.resident(todo[b0 + i], texts[i], recs[i], names[i]);
            std::string().swap(texts[i]);
            const double tb = now();
            const uint64_t* d_rec = (const uint64_t*)e.d_rec;
            const size_t p0 = pair0[i], np = pair0[i + 1] - p0;
            txq_check(txq_regex_filter_device((const uint8_t*)d_arena.p, (const uint64_t*)d_arena_off.p, n_automata, arena.size(), (const uint8_t*)e.d_text,
                                              d_rec, e.n_records, e.text_bytes, d_rec + e.n_records + 1, 1, (const uint32_t*)d_pairs.p + 2 * p0, np,
                                              (const uint64_t*)d_out_off.p + p0, (uint32_t*)d_out.p + word0[i], word0[i + 1] - word0[i],
                                              (uint32_t*)d_status.p + p0, (unsigned char*)d_work.p + 8 * p0 + 8 * i, nullptr),
                      "txq_regex_filter_device");
            t_upload += tb - ta;
            t_filter += now() - tb;
        }
        const double t1 = now();
        txq_check(txq_synchronize(), "txq_synchronize");
        const double t2 = now();
        std::vector<uint32_t> words(n_words + 1), status(n_pairs + 1);
        txq_check(txq_memcpy_d2h(words.data(), d_out.p, n_words * 4), "d2h");
        txq_check(txq_memcpy_d2h(status.data(), d_status.p, n_pairs * 4), "d2h");
        for (size_t i = 0; i < nb; ++i) {
            const uint32_t bin = todo[b0 + i];
            size_t p = pair0[i];
            for (uint32_t q : wanted[bin]) {
                bool answered = true;
                for (size_t s = 0; s < strands; ++s) answered = answered && status[p + s] == 0;
                if (!answered) { ++stats_.pairs_host; p += strands; continue; }
                RecordSelection::Lists& lists = out.pairs[RecordSelection::key(q, bin)];
                for (size_t s = 0; s < strands; ++s, ++p) {
                    const uint32_t* bits = words.data() + word0[i] + out_off[p];
                    for (uint64_t r = 0; r < n_records[i]; ++r)
                        if ((bits[r >> 5] >> (r & 31)) & 1) lists.strand[s].push_back((uint32_t)r);
                    stats_.records_flagged += lists.strand[s].size();
                    stats_.records_total += n_records[i];
                }
                ++stats_.pairs_device;
            }
        }
        stats_.upload_seconds += t_upload;
        stats_.filter_seconds += t_filter + (t2 - t1);
        stats_.copy_seconds += now() - t2;
    }
}

}  // namespace tetrex
