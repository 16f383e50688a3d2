#include "index_build.hpp"
#include "device_buffer.hpp"
#include "device_index.hpp"
#include "fasta.hpp"
#include "kgraph.hpp"
#include "layout.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>

namespace tetrex {

namespace {

void ensure_device(int device) { DeviceIndex::warm_up(std::vector<int>{device}); }

// Build one flat IBF on the device from per-bin value lists and copy its words back.
IbfImage build_flat(const std::vector<const std::vector<uint64_t>*>& per_bin, uint64_t rows, unsigned h) {
    IbfImage img;
    img.shape(per_bin.size(), rows, h);
    txq_index* ix = nullptr;
    txq_check(txq_index_create_ibf(img.bins, rows, h, 0, 1, &ix), "txq_index_create_ibf");
    try {
        std::vector<uint64_t> vals;
        std::vector<uint32_t> bins;
        auto flush = [&]() {
            if (vals.empty()) return;
            DeviceBuffer dv(vals.size() * 8), db(bins.size() * 4);
            txq_check(txq_memcpy_h2d(dv.p, vals.data(), vals.size() * 8), "h2d");
            txq_check(txq_memcpy_h2d(db.p, bins.data(), bins.size() * 4), "h2d");
            txq_check(txq_emplace_device(ix, (const uint64_t*)dv.p, (const uint32_t*)db.p, vals.size(), nullptr), "txq_emplace_device");
            txq_check(txq_synchronize(), "txq_synchronize");
            vals.clear();
            bins.clear();
        };
        for (size_t b = 0; b < per_bin.size(); ++b) {
            for (uint64_t v : *per_bin[b]) { vals.push_back(v); bins.push_back((uint32_t)b); }
            if (vals.size() >= (1u << 24)) flush();
        }
        flush();
        txq_check(txq_index_download_words(ix, img.words.data(), img.words.size()), "txq_index_download_words");
    } catch (...) {
        txq_index_free(ix);
        throw;
    }
    txq_index_free(ix);
    return img;
}

// The size-aware tree (`--layout sized`, host/layout.hpp) built on the device: the k-mer values of all bins go up as one CSR
// array (streamed in chunks of at most kBuildChunk values when the library is larger), are sketched, the union table
// is estimated for the layout DP, and one pass inserts every value into each IBF on its user bin's path.
constexpr uint64_t kBuildChunk = uint64_t(1) << 27;  // values per chunk (1 GiB)

HibfImage build_sized_hibf(const std::vector<std::vector<uint64_t>>& values, const BuildOptions& opt) {
    using clock = std::chrono::steady_clock;
    const bool trace = std::getenv("TETREX_TRACE") != nullptr;
    auto ms = [](clock::time_point a, clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const uint64_t B = values.size();
    std::vector<uint64_t> offsets(B + 1, 0);
    for (uint64_t b = 0; b < B; ++b) offsets[b + 1] = offsets[b] + values[b].size();
    const uint64_t total = offsets[B];
    const uint64_t chunk = std::max<uint64_t>(1, std::min(total, kBuildChunk));
    const uint64_t n_chunks = std::max<uint64_t>(1, (total + chunk - 1) / chunk);
    DeviceBuffer d_vals(chunk * 8), d_offs((B + 1) * 8);
    std::vector<uint64_t> chunk_offs(B + 1);
    // chunk c = values [c * chunk, ...) of the concatenation; every bin's slice of it is copied from the bin's own vector
    auto upload_chunk = [&](uint64_t c) -> uint64_t {
        const uint64_t g0 = c * chunk, g1 = std::min(total, g0 + chunk);
        for (uint64_t b = 0; b <= B; ++b) chunk_offs[b] = std::min(std::max(offsets[b], g0), g1) - g0;
        for (uint64_t b = 0; b < B; ++b) {
            const uint64_t lo = chunk_offs[b], hi = chunk_offs[b + 1];
            if (hi > lo)
                txq_check(txq_memcpy_h2d((uint64_t*)d_vals.p + lo, values[b].data() + (g0 + lo - offsets[b]), (hi - lo) * 8), "h2d values");
        }
        txq_check(txq_memcpy_h2d(d_offs.p, chunk_offs.data(), (B + 1) * 8), "h2d offsets");
        return g1 - g0;
    };
    const auto t0 = clock::now();
    // sketches
    DeviceBuffer d_regs(B * TXQ_HLL_REGISTERS);
    {
        const std::vector<uint8_t> zero(B * TXQ_HLL_REGISTERS, 0);
        txq_check(txq_memcpy_h2d(d_regs.p, zero.data(), zero.size()), "h2d registers");
    }
    uint64_t resident = UINT64_MAX;  // the chunk now on the device
    for (uint64_t c = 0; c < n_chunks; ++c) {
        const uint64_t n = upload_chunk(c);
        resident = c;
        txq_check(txq_sketch_device((const uint64_t*)d_vals.p, n, (const uint64_t*)d_offs.p, B, (uint8_t*)d_regs.p, nullptr), "txq_sketch_device");
    }
    txq_check(txq_synchronize(), "sketch");
    const auto t1 = clock::now();
    // each bin's estimate (identity order, window 1), the layout order, the union table
    LayoutParams lp;
    lp.tmax = opt.tmax ? opt.tmax : default_tmax(B);
    lp.fpr = opt.fpr;
    lp.hash_count = opt.hash_count;
    const uint64_t W = union_window(B, lp.tmax);
    std::vector<double> counts(B), unions(B * W);
    std::vector<uint64_t> final_order;
    uint64_t n_intervals = 0, longest_interval = 0;
    double rearrange_ms = 0;
    {
        std::vector<uint32_t> order(B);
        for (uint64_t b = 0; b < B; ++b) order[b] = (uint32_t)b;
        DeviceBuffer d_order(B * 4), d_est(B * W * 8);
        txq_check(txq_memcpy_h2d(d_order.p, order.data(), B * 4), "h2d order");
        txq_check(txq_union_estimates_device((const uint8_t*)d_regs.p, (const uint32_t*)d_order.p, B, 1, (double*)d_est.p, nullptr), "txq_union_estimates_device");
        txq_check(txq_memcpy_d2h(counts.data(), d_est.p, B * 8), "d2h estimates");
        final_order = layout_order(counts.data(), B);
        if (opt.rearrange_ratio != 0) {
            // inside each interval of the sorted order: the pairwise unions from the device, the chain on the host
            const auto r0 = clock::now();
            const std::vector<uint64_t> sorted = final_order;
            const std::vector<uint64_t> starts = rearrange_intervals(counts.data(), sorted.data(), B, opt.rearrange_ratio);
            n_intervals = starts.size();
            for (uint64_t i = 0; i < n_intervals; ++i)
                longest_interval = std::max(longest_interval, (i + 1 < n_intervals ? starts[i + 1] : B) - starts[i]);
            if (longest_interval >= 3) {
                DeviceBuffer d_ids(longest_interval * 4), d_pairs(longest_interval * longest_interval * 8);
                std::vector<uint32_t> ids;
                std::vector<double> pairs, c;
                for (uint64_t i = 0; i < n_intervals; ++i) {
                    const uint64_t s = starts[i], n = (i + 1 < n_intervals ? starts[i + 1] : B) - s;
                    if (n < 3) continue;
                    ids.resize(n);
                    c.resize(n);
                    pairs.resize(n * n);
                    for (uint64_t j = 0; j < n; ++j) { ids[j] = (uint32_t)sorted[s + j]; c[j] = counts[sorted[s + j]]; }
                    txq_check(txq_memcpy_h2d(d_ids.p, ids.data(), n * 4), "h2d interval");
                    txq_check(txq_pair_unions_device((const uint8_t*)d_regs.p, (const uint32_t*)d_ids.p, n, (double*)d_pairs.p, nullptr), "txq_pair_unions_device");
                    txq_check(txq_memcpy_d2h(pairs.data(), d_pairs.p, n * n * 8), "d2h pair unions");
                    const std::vector<uint64_t> chain = rearrange_chain(c.data(), pairs.data(), n);
                    for (uint64_t j = 0; j < n; ++j) final_order[s + j] = sorted[s + chain[j]];
                }
            }
            rearrange_ms = ms(r0, clock::now());
        }
        for (uint64_t s = 0; s < B; ++s) order[s] = (uint32_t)final_order[s];
        txq_check(txq_memcpy_h2d(d_order.p, order.data(), B * 4), "h2d order");
        txq_check(txq_union_estimates_device((const uint8_t*)d_regs.p, (const uint32_t*)d_order.p, B, W, (double*)d_est.p, nullptr), "txq_union_estimates_device");
        txq_check(txq_memcpy_d2h(unions.data(), d_est.p, B * W * 8), "d2h unions");
    }
    const auto t2 = clock::now();
    const HibfLayout layout = hibf_layout_ordered(counts.data(), B, final_order.data(), unions.data(), W, lp);
    const auto paths = layout_paths(layout, B);
    const auto t3 = clock::now();
    // the tree on the device
    HibfImage h;
    h.user_bins = B;
    const uint64_t n_ibf = layout.ibfs.size();
    h.ibfs.resize(n_ibf);
    std::vector<std::unique_ptr<DeviceBuffer>> d_words;
    std::vector<txq_ibf_desc> descs(n_ibf);
    for (uint64_t i = 0; i < n_ibf; ++i) {
        const LayoutIbf& f = layout.ibfs[i];
        IbfImage& img = h.ibfs[i];
        img.shape(f.tb_to_user_bin.size(), f.bin_size, opt.hash_count);
        h.next_ibf_id.push_back(f.next_ibf_id);
        h.tb_to_user_bin.push_back(f.tb_to_user_bin);
        d_words.push_back(std::make_unique<DeviceBuffer>(img.words.size() * 8));
        txq_check(txq_memcpy_h2d(d_words.back()->p, img.words.data(), img.words.size() * 8), "h2d zero words");
        descs[i] = txq_ibf_desc{img.bins, img.tech_bins, img.bin_size, img.hash_shift, img.bin_words, img.hash_funs, (const uint64_t*)d_words.back()->p};
    }
    std::vector<uint64_t> path_offsets(B + 1, 0), path;
    for (uint64_t b = 0; b < B; ++b) {
        for (const PathStep& st : paths[b]) { path.push_back(st.ibf); path.push_back(st.tb); path.push_back(st.parts); }
        path_offsets[b + 1] = path.size() / 3;
    }
    DeviceBuffer d_descs(n_ibf * sizeof(txq_ibf_desc)), d_poff((B + 1) * 8), d_path(path.size() * 8);
    txq_check(txq_memcpy_h2d(d_descs.p, descs.data(), n_ibf * sizeof(txq_ibf_desc)), "h2d descriptors");
    txq_check(txq_memcpy_h2d(d_poff.p, path_offsets.data(), (B + 1) * 8), "h2d path offsets");
    txq_check(txq_memcpy_h2d(d_path.p, path.data(), path.size() * 8), "h2d paths");
    for (uint64_t c = 0; c < n_chunks; ++c) {
        // the last chunk the sketch pass uploaded is still resident (values and offsets)
        const uint64_t n = resident == c ? std::min(total - c * chunk, chunk) : upload_chunk(c);
        resident = c;
        txq_check(txq_tree_insert_device((const uint64_t*)d_vals.p, n, (const uint64_t*)d_offs.p, B, (const uint64_t*)d_poff.p,
                                         (const uint64_t*)d_path.p, (const txq_ibf_desc*)d_descs.p, n_ibf, nullptr), "txq_tree_insert_device");
    }
    txq_check(txq_synchronize(), "tree insert");
    const auto t4 = clock::now();
    for (uint64_t i = 0; i < n_ibf; ++i)
        txq_check(txq_memcpy_d2h(h.ibfs[i].words.data(), d_words[i]->p, h.ibfs[i].words.size() * 8), "d2h words");
    const auto t5 = clock::now();
    if (trace) {
        uint64_t bits = 0;
        for (const IbfImage& f : h.ibfs) bits += f.tech_bins * f.bin_size;
        std::fprintf(stderr, "[tetrex] sized layout: %llu user bins, %llu IBFs, %llu bits, t_max %llu, window %llu, %llu values in %llu chunk(s)\n",
                     (unsigned long long)B, (unsigned long long)n_ibf, (unsigned long long)bits, (unsigned long long)lp.tmax,
                     (unsigned long long)W, (unsigned long long)total, (unsigned long long)n_chunks);
        if (opt.rearrange_ratio != 0) {
            std::fprintf(stderr, "[tetrex] sized layout: rearranged in %llu interval(s), the longest of %llu bins (ratio %g)\n",
                         (unsigned long long)n_intervals, (unsigned long long)longest_interval, opt.rearrange_ratio);
            std::fprintf(stderr, "[tetrex] build ms: upload+sketch %.3f union %.3f rearrange %.3f layout %.3f insert %.3f download %.3f\n",
                         ms(t0, t1), ms(t1, t2) - rearrange_ms, rearrange_ms, ms(t2, t3), ms(t3, t4), ms(t4, t5));
        } else
            std::fprintf(stderr, "[tetrex] build ms: upload+sketch %.3f union %.3f layout %.3f insert %.3f download %.3f\n", ms(t0, t1),
                         ms(t1, t2), ms(t2, t3), ms(t3, t4), ms(t4, t5));
    }
    return h;
}

}  // namespace

IndexImage build_index(const std::vector<std::string>& bin_files, const BuildOptions& opt, size_t* n_sequences) {
    if (bin_files.empty()) throw std::runtime_error("no input libraries");
    if (!opt.dna && opt.k > 12) throw std::runtime_error("Max kmer size for amino acids is 12");
    if (opt.dna && opt.k > 32) throw std::runtime_error("Max kmer size for nucleic acids is 32");
    ensure_device(opt.device);
    if (opt.layout == BuildOptions::kSized && !opt.hibf) throw std::runtime_error("a sized layout is an HIBF layout (not with -i)");
    if (opt.layout == BuildOptions::kSized && (opt.tmax % 64 != 0)) throw std::runtime_error("t_max must be a positive multiple of 64");
    if (opt.rearrange_ratio != 0 && opt.layout != BuildOptions::kSized) throw std::runtime_error("rearrangement is an option of the sized layout");
    if (opt.rearrange_ratio != 0 && !(opt.rearrange_ratio > 0 && opt.rearrange_ratio <= 1))
        throw std::runtime_error("the rearrangement ratio must lie in (0, 1]");
    const auto t_encode = std::chrono::steady_clock::now();
    const KmerEncoder enc(opt.dna ? Molecule::DNA : Molecule::Peptide, opt.k, (Alphabet)opt.reduction);
    std::vector<std::vector<uint64_t>> values(bin_files.size());
    size_t seqs = 0;
    for (size_t b = 0; b < bin_files.size(); ++b)
        for_each_record(bin_files[b], [&](const FastaRecord& r) {
            if (r.seq.size() < opt.k) return;  // "RECORD TOO SHORT"
            ++seqs;
            enc.record_values(r.seq, opt.dna_wraparound, values[b]);
        });
    if (n_sequences) *n_sequences = seqs;
    if (std::getenv("TETREX_TRACE"))
        std::fprintf(stderr, "[tetrex] build ms: encode %.3f\n",
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_encode).count());

    IndexImage img;
    img.k = (uint8_t)opt.k;
    img.molecule = opt.dna ? "na" : "aa";
    img.reduction = (uint8_t)opt.reduction;
    img.hash_count = (uint8_t)opt.hash_count;
    img.fpr = opt.fpr;
    img.bin_paths = bin_files;
    auto largest = [](const std::vector<const std::vector<uint64_t>*>& v) {
        size_t m = 0;
        for (auto* p : v) m = std::max(m, p->size());
        return m;
    };
    if (!opt.hibf) {
        // IBFIndex::init_ibf: size every bin like the largest one, occurrences not deduplicated
        std::vector<const std::vector<uint64_t>*> per_bin;
        for (auto& v : values) per_bin.push_back(&v);
        const uint64_t rows = std::max<uint64_t>(1, compute_bitcount(largest(per_bin), opt.fpr));
        img.ibf = build_flat(per_bin, rows, opt.hash_count);
        img.format = "ibf";
        return img;
    }
    // HIBF with this project's own two-level layout (the reference delegates the layout to
    // seqan::hibf's sketch-based algorithm, which is index construction, not query): user bins are
    // dealt in order over at most t_max = 64*ceil(sqrt(B)/64) merged technical bins of the root, each
    // pointing at a child IBF with one technical bin per user bin.  B <= t_max: a single level.
    // A child holds a multiple of 64 user bins, so its rows are whole words of the result mask, and all children
    // have the rows of the largest user bin (as the flat IBF sizes its bins): the device keeps such a tree's children
    // side by side and probes them like one flat IBF (csrc/txq_hibf.hip: regular trees, uniform children).
    img.is_hibf = true;
    if (opt.layout == BuildOptions::kSized) {
        img.hibf = build_sized_hibf(values, opt);
        img.format = "hibf";
        return img;
    }
    HibfImage& h = img.hibf;
    const uint64_t B = bin_files.size();
    h.user_bins = B;
    const uint64_t tmax = 64 * (((uint64_t)std::ceil(std::sqrt((double)B)) + 63) / 64);
    if (B <= tmax) {
        std::vector<const std::vector<uint64_t>*> per_bin;
        for (auto& v : values) per_bin.push_back(&v);
        h.ibfs.push_back(build_flat(per_bin, std::max<uint64_t>(1, compute_bitcount(largest(per_bin), opt.fpr)), opt.hash_count));
        h.next_ibf_id.emplace_back(B, 0);
        h.tb_to_user_bin.emplace_back();
        for (uint64_t b = 0; b < B; ++b) h.tb_to_user_bin.back().push_back(b);
    } else {
        const uint64_t per_child = 64 * (((B + tmax - 1) / tmax + 63) / 64), n_child = (B + per_child - 1) / per_child;
        std::vector<const std::vector<uint64_t>*> all_bins;
        for (auto& v : values) all_bins.push_back(&v);
        const uint64_t child_rows = std::max<uint64_t>(1, compute_bitcount(largest(all_bins), opt.fpr));
        std::vector<std::vector<uint64_t>> merged(n_child);
        h.ibfs.resize(1 + n_child);
        h.next_ibf_id.resize(1 + n_child);
        h.tb_to_user_bin.resize(1 + n_child);
        for (uint64_t c = 0; c < n_child; ++c) {
            const uint64_t lo = c * per_child, hi = std::min(B, lo + per_child);
            std::vector<const std::vector<uint64_t>*> per_bin;
            for (uint64_t b = lo; b < hi; ++b) {
                per_bin.push_back(&values[b]);
                merged[c].insert(merged[c].end(), values[b].begin(), values[b].end());
                h.tb_to_user_bin[1 + c].push_back(b);
            }
            h.next_ibf_id[1 + c].assign(hi - lo, 0);
            h.ibfs[1 + c] = build_flat(per_bin, child_rows, opt.hash_count);
            h.next_ibf_id[0].push_back(1 + c);
            h.tb_to_user_bin[0].push_back(UINT64_MAX);
        }
        std::vector<const std::vector<uint64_t>*> per_bin;
        for (auto& v : merged) per_bin.push_back(&v);
        h.ibfs[0] = build_flat(per_bin, std::max<uint64_t>(1, compute_bitcount(largest(per_bin), opt.fpr)), opt.hash_count);
    }
    img.format = "hibf";
    return img;
}

DgramImage build_dgram_index(const std::vector<std::string>& bin_files, uint64_t min_gap, uint64_t max_gap, unsigned hash_count,
                             float fpr, int device) {
    if (bin_files.empty()) throw std::runtime_error("no input libraries");
    if (min_gap > max_gap) throw std::runtime_error("lower gap bound above the upper bound");
    ensure_device(device);
    std::vector<std::vector<uint64_t>> values(bin_files.size());
    for (size_t b = 0; b < bin_files.size(); ++b)
        for_each_record(bin_files[b], [&](const FastaRecord& r) { dgram_record_values(r.seq, min_gap, max_gap, values[b]); });
    std::vector<const std::vector<uint64_t>*> per_bin;
    size_t most = 0;
    for (auto& v : values) { per_bin.push_back(&v); most = std::max(most, v.size()); }
    DgramImage d;
    d.min_gap = min_gap;
    d.max_gap = max_gap;
    d.hash_count = (uint8_t)hash_count;
    d.fpr = fpr;
    d.bin_paths = bin_files;
    d.ibf = build_flat(per_bin, std::max<uint64_t>(1, compute_bitcount(most, fpr)), hash_count);
    d.format = "dgram";
    return d;
}

}  // namespace tetrex
