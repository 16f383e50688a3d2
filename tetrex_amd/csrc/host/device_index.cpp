#include "device_index.hpp"
#include "edit_distance.hpp"
#include "fasta.hpp"
#include "kgraph.hpp"
#include "matcher.hpp"
#include "regex_front.hpp"
#include "../../../include/txq_regex.h"
#include "../txq_frame_windows_plan.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <future>
#include <memory>
#include <numeric>
#include <tuple>
#include <stdexcept>

namespace tetrex {

void txq_check(int rc, const char* what) {
    if (rc != TXQ_OK) throw std::runtime_error(std::string(what) + ": " + txq_last_error());
}

static void ensure_devices(const std::vector<int>& devices) {
    static std::vector<int> bound;
    if (bound == devices) return;
    txq_check(txq_init((int)devices.size(), devices.data()), "txq_init");
    bound = devices;
}
static void ensure_device(int device) { ensure_devices(std::vector<int>{device}); }

void DeviceIndex::warm_up(const std::vector<int>& devices) { ensure_devices(devices); }

static txq_ibf_desc describe(const IbfImage& f) {
    return txq_ibf_desc{f.bins, f.tech_bins, f.bin_size, f.hash_shift, f.bin_words, f.hash_funs, f.word_data()};  // possibly a view into the mapped index file
}

DeviceIndex::~DeviceIndex() {
    for (txq_index* a : aux_shards_) txq_index_free(a);
    for (txq_index* s : shards_) txq_index_free(s);
}

void DeviceIndex::attach_dgram(const DgramImage& dgram) {
    if (!ix_) throw std::runtime_error("index not uploaded");
    if (dgram.ibf.bins != info_.user_bins) throw std::runtime_error("the d-gram index was built over a different number of bins");
    for (txq_index* a : aux_shards_) txq_index_free(a);
    aux_shards_.clear();
    aux_ = nullptr;
    txq_ibf_desc d = describe(dgram.ibf);
    txq_index_desc desc{1, &d, nullptr, nullptr, dgram.ibf.bins};
    for (size_t r = 0; r < shards_.size(); ++r) {  // same shard, same device as the main index's shard
        txq_index* a = nullptr;
        txq_check(txq_index_upload(&desc, shards_.size() > 1 ? (int)r : shard_rank_, n_shards_, &a), "txq_index_upload(d-gram)");
        aux_shards_.push_back(a);
    }
    aux_ = aux_shards_[0];
    dgram_min_ = dgram.min_gap;
    dgram_max_ = dgram.max_gap;
}

txq_index* DeviceIndex::upload_one(const IndexImage& image, int shard_rank, int n_shards) {
    txq_index* ix = nullptr;
    if (!image.is_hibf) {
        txq_ibf_desc d = describe(image.ibf);
        txq_index_desc desc{1, &d, nullptr, nullptr, image.ibf.bins};
        txq_check(txq_index_upload(&desc, shard_rank, n_shards, &ix), "txq_index_upload");
    } else {
        const HibfImage& h = image.hibf;
        std::vector<txq_ibf_desc> ds;
        std::vector<const uint64_t*> nx, tb;
        for (size_t i = 0; i < h.ibfs.size(); ++i) {
            ds.push_back(describe(h.ibfs[i]));
            nx.push_back(h.next_ibf_id[i].data());
            tb.push_back(h.tb_to_user_bin[i].data());
        }
        txq_index_desc desc{ds.size(), ds.data(), nx.data(), tb.data(), h.user_bins};
        // (a general tree is sharded by sub-trees — full-width masks, ORed —, a regular two-level one by mask columns: the library decides)
        txq_check(txq_index_upload_subtrees(&desc, shard_rank, n_shards, &ix), "txq_index_upload_subtrees");
    }
    return ix;
}

void DeviceIndex::upload(const IndexImage& image, int device, int shard_rank, int n_shards) {
    ensure_device(device);
    for (txq_index* a : aux_shards_) txq_index_free(a);
    for (txq_index* s : shards_) txq_index_free(s);
    aux_shards_.clear();
    shards_.clear();
    aux_ = ix_ = nullptr;
    shard_rank_ = shard_rank;
    n_shards_ = n_shards;
    enc_ = KmerEncoder(image.molecule == "na" ? Molecule::DNA : Molecule::Peptide, image.k, (Alphabet)image.reduction);
    // the library deals shards over its devices by rank; with one device every rank lands on it
    ix_ = upload_one(image, shard_rank, n_shards);
    shards_.push_back(ix_);
    txq_check(txq_index_get_info(ix_, &info_), "txq_index_get_info");
}

void DeviceIndex::upload_sharded(const IndexImage& image, const std::vector<int>& devices, int n_shards) {
    if (devices.empty() || n_shards < 1) throw std::runtime_error("upload_sharded needs at least one device and one shard");
    ensure_devices(devices);
    for (txq_index* a : aux_shards_) txq_index_free(a);
    for (txq_index* s : shards_) txq_index_free(s);
    aux_shards_.clear();
    shards_.clear();
    aux_ = ix_ = nullptr;
    shard_rank_ = 0;
    n_shards_ = n_shards;
    enc_ = KmerEncoder(image.molecule == "na" ? Molecule::DNA : Molecule::Peptide, image.k, (Alphabet)image.reduction);
    for (int r = 0; r < n_shards; ++r) shards_.push_back(upload_one(image, r, n_shards));
    ix_ = shards_[0];
    txq_check(txq_index_get_info(ix_, &info_), "txq_index_get_info");
}

TxqStageExecutor::TxqStageExecutor(txq_index* ix, size_t n_programs, txq_index* aux) {
    txq_check(txq_session_begin(ix, n_programs, &session_), "txq_session_begin");
    if (aux) {
        const int rc = txq_session_set_aux_index(session_, aux);
        if (rc != TXQ_OK) {
            txq_session_end(session_, nullptr);
            session_ = nullptr;
            txq_check(rc, "txq_session_set_aux_index");
        }
    }
}
TxqStageExecutor::~TxqStageExecutor() {
    if (session_) txq_session_end(session_, nullptr);
}
void TxqStageExecutor::stage(const uint8_t* blob, size_t blob_bytes, const std::vector<uint32_t>& qp, const std::vector<uint32_t>& qs,
                             std::vector<uint8_t>& alive) {
    alive.assign(qp.size(), 1);
    txq_check(txq_session_stage(session_, blob, blob_bytes, qp.data(), qs.data(), qp.size(), alive.data()), "txq_session_stage");
}
void TxqStageExecutor::finish(uint64_t* masks) {
    txq_session* s = session_;
    session_ = nullptr;
    txq_check(txq_session_end(s, masks), "txq_session_end");
}

ShardedStageExecutor::ShardedStageExecutor(const std::vector<txq_index*>& shards, size_t n_programs, const std::vector<txq_index*>& aux)
    : n_programs_(n_programs) {
    if (shards.empty()) throw std::runtime_error("no shards");
    if (!aux.empty() && aux.size() != shards.size()) throw std::runtime_error("the d-gram index must be sharded like the main index");
    try {
        for (size_t r = 0; r < shards.size(); ++r) {
            txq_index_info info{};
            txq_check(txq_index_get_info(shards[r], &info), "txq_index_get_info");
            info_.push_back(info);
            txq_session* s = nullptr;
            txq_check(txq_session_begin(shards[r], n_programs, &s), "txq_session_begin");
            sessions_.push_back(s);
            if (!aux.empty()) txq_check(txq_session_set_aux_index(s, aux[r]), "txq_session_set_aux_index");
        }
    } catch (...) {
        for (txq_session* s : sessions_) txq_session_end(s, nullptr);
        throw;
    }
}
ShardedStageExecutor::~ShardedStageExecutor() {
    for (txq_session* s : sessions_)
        if (s) txq_session_end(s, nullptr);
}
void ShardedStageExecutor::stage(const uint8_t* blob, size_t blob_bytes, const std::vector<uint32_t>& qp, const std::vector<uint32_t>& qs,
                                 std::vector<uint8_t>& alive) {
    const size_t R = sessions_.size(), nq = qp.size();
    std::vector<std::vector<uint8_t>> answers(R, std::vector<uint8_t>(nq, 0));
    std::vector<std::string> errors(R);
    auto run = [&](size_t r) {  // txq_last_error() is per thread: fetch it on the thread that made the call
        if (txq_session_stage(sessions_[r], blob, blob_bytes, qp.data(), qs.data(), nq, answers[r].data()) != TXQ_OK)
            errors[r] = std::string("txq_session_stage (shard ") + std::to_string(r) + "): " + txq_last_error();
    };
    std::vector<std::future<void>> others;
    for (size_t r = 1; r < R; ++r) others.push_back(std::async(std::launch::async, run, r));
    run(0);
    for (auto& f : others) f.get();
    for (const std::string& e : errors)
        if (!e.empty()) throw std::runtime_error(e);
    // an answer is 0 (no bit) or 1 + floor(log2(bits set in the shard's columns)): the shards' counts add up
    alive.assign(nq, 0);
    for (size_t i = 0; i < nq; ++i) {
        uint64_t bits = 0;
        for (size_t r = 0; r < R; ++r) {
            const uint8_t b = answers[r][i];
            bits += b == 0 ? 0 : b == 1 ? 1 : (3ULL << (b - 2));  // the middle of [2^(b-1), 2^b)
        }
        alive[i] = bits ? (uint8_t)(64 - __builtin_clzll(bits)) : 0;
    }
}
std::vector<uint64_t> ShardedStageExecutor::finish() {
    const size_t R = sessions_.size();
    std::vector<std::vector<uint64_t>> part(R);
    std::vector<uint64_t> word0(R), words(R);
    std::vector<const uint64_t*> ptr(R);
    std::string error;
    for (size_t r = 0; r < R; ++r) {
        part[r].resize(n_programs_ * info_[r].shard_words + 1);
        txq_session* s = sessions_[r];
        sessions_[r] = nullptr;
        if (txq_session_end(s, part[r].data()) != TXQ_OK && error.empty()) error = std::string("txq_session_end: ") + txq_last_error();
        word0[r] = info_[r].shard_word0;
        words[r] = info_[r].shard_words;
        ptr[r] = part[r].data();
    }
    if (!error.empty()) throw std::runtime_error(error);
    if (info_[0].join_or) {  // sub-tree shards of a general HIBF: full-width masks, ORed (a split bin may straddle shards)
        const uint64_t mw = info_[0].mask_words;
        std::vector<uint64_t> full(n_programs_ * mw, 0);
        for (size_t r = 0; r < R; ++r) {
            if (!info_[r].join_or || info_[r].shard_words != mw) throw std::runtime_error("shards of different kinds in one join");
            for (size_t i = 0; i < n_programs_ * mw; ++i) full[i] |= part[r][i];
        }
        return full;
    }
    return join_shard_masks(n_programs_, info_[0].mask_words, word0, words, ptr);
}

std::vector<uint64_t> run_queries_sharded(const std::vector<txq_index*>& shards, const KmerEncoder& enc, const std::vector<std::string>& regexes,
                                          std::vector<int>* status, std::vector<std::string>* messages, StagedStats* stats,
                                          const StagedOptions* options, const std::vector<txq_index*>& aux) {
    if (shards.empty()) throw std::runtime_error("no shards");
    txq_index_info info{};
    txq_check(txq_index_get_info(shards[0], &info), "txq_index_get_info");
    if (status) status->assign(regexes.size(), 0);
    if (messages) messages->assign(regexes.size(), std::string());
    if (regexes.empty()) return std::vector<uint64_t>();
    ShardedStageExecutor exec(shards, regexes.size(), aux);
    StagedOptions opt = options ? *options : StagedOptions{};
    opt.dense.enabled = true;
    opt.dense.tracked_ok = true;
    opt.dense.slot_bytes = 0;
    for (txq_index* s : shards) {  // dense steps only where every shard can run them; budgets by the widest shard
        txq_index_info i{};
        txq_check(txq_index_get_info(s, &i), "txq_index_get_info");
        if (i.shard_words) opt.dense.enabled = opt.dense.enabled && txq_index_supports_dense(s) != 0;
        if (i.shard_words) opt.dense.tracked_ok = opt.dense.tracked_ok && txq_index_supports_dense(s) == 2;
        opt.dense.slot_bytes = std::max<uint64_t>(opt.dense.slot_bytes, i.shard_words * 8);
    }
    uint64_t tag = 0;
    (void)txq_index_get_tag(shards[0], &tag);
    if (opt.dense_evidence == DenseOptions::kUnknown) opt.dense_evidence = (int)(tag & 3);  // what earlier runs learned about the index
    const StagedStats st = run_staged(enc, info.user_bins, regexes, exec, opt, status, messages);
    if (st.dense_evidence != DenseOptions::kUnknown) (void)txq_index_set_tag(shards[0], (tag & ~(uint64_t)3) | (uint64_t)st.dense_evidence);
    if (stats) *stats = st;
    return exec.finish();
}

std::vector<uint64_t> run_queries(txq_index* ix, const KmerEncoder& enc, const std::vector<std::string>& regexes,
                                  std::vector<int>* status, std::vector<std::string>* messages, StagedStats* stats,
                                  const StagedOptions* options, txq_index* aux, uint64_t* into) {
    txq_index_info info{};
    txq_check(txq_index_get_info(ix, &info), "txq_index_get_info");
    // into: the caller's own n x shard_words words (a binding's array): the masks go there and nothing is returned — 10 000 masks
    // of 8192 bins are 10 MB that would otherwise be zeroed, filled and copied once more
    std::vector<uint64_t> masks(into ? 0 : regexes.size() * info.shard_words);
    if (status) status->assign(regexes.size(), 0);
    if (messages) messages->assign(regexes.size(), std::string());
    if (regexes.empty()) return masks;
    const bool trace = std::getenv("TETREX_TRACE") != nullptr;
    const auto t_begin = std::chrono::steady_clock::now();
    TxqStageExecutor exec(ix, regexes.size(), aux);
    if (trace)
        std::fprintf(stderr, "[tetrex] session begin %.2f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
    StagedOptions opt = options ? *options : StagedOptions{};
    // saturated state lists run as dense DP steps on the device where the index allows it (TETREX_DENSE=0 switches them off)
    opt.dense.enabled = txq_index_supports_dense(ix) != 0;
    opt.dense.tracked_ok = txq_index_supports_dense(ix) == 2;  // fused steps: the session keeps live lists (tracked programs)
    opt.dense.slot_bytes = info.shard_words * 8;
    opt.feedback_bins = std::min<uint64_t>(info.user_bins, info.shard_words * 64);
    {   // dense blocks may take three quarters of what the device has left (and of what the index kept from earlier sessions),
        // not a constant that ignores a 64 GB index next to them
        uint64_t free_b = 0, kept_b = 0;
        if (txq_index_memory(ix, &free_b, &kept_b) == TXQ_OK) opt.dense_pool_bytes = std::min<uint64_t>(opt.dense_pool_bytes, (free_b + kept_b) / 4 * 3);
    }
    uint64_t tag = 0;
    (void)txq_index_get_tag(ix, &tag);
    if (opt.dense_evidence == DenseOptions::kUnknown) opt.dense_evidence = (int)(tag & 3);  // what earlier runs learned about the index
    const auto t0 = std::chrono::steady_clock::now();
    const StagedStats st = run_staged(enc, info.user_bins, regexes, exec, opt, status, messages);
    if (st.dense_evidence != DenseOptions::kUnknown) (void)txq_index_set_tag(ix, (tag & ~(uint64_t)3) | (uint64_t)st.dense_evidence);
    if (stats) *stats = st;
    const auto t1 = std::chrono::steady_clock::now();
    exec.finish(into ? into : masks.data());  // waits for the device: a stage without feedback questions returns as soon as it is launched
    if (trace)
        std::fprintf(stderr, "[tetrex] run_staged %.2f ms, finish (device drain + result copy) %.2f ms\n",
                     std::chrono::duration<double, std::milli>(t1 - t0).count(),
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
    return masks;
}

void DeviceIndex::count(const std::vector<uint64_t>& values, const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& thresholds,
                        std::vector<uint64_t>& hits, std::vector<uint32_t>* counts) {
    if (!ix_) throw std::runtime_error("index not uploaded");
    if (shards_.size() > 1) throw std::runtime_error("count: one shard only");
    if (offsets.empty() || thresholds.size() + 1 != offsets.size()) throw std::runtime_error("count: offsets and thresholds disagree");
    const size_t n = thresholds.size(), W = info_.shard_words;
    hits.assign(n * W, 0);
    if (counts) counts->assign(n * W * 64, 0);
    txq_check(txq_count(ix_, values.data(), offsets.data(), n, thresholds.data(), hits.data(), counts ? counts->data() : nullptr), "txq_count");
}

std::vector<uint64_t> DeviceIndex::query_masks(const std::vector<std::string>& regexes, std::vector<int>* status,
                                               std::vector<std::string>* messages, StagedStats* stats, const StagedOptions* options) {
    if (!ix_) throw std::runtime_error("index not uploaded");
    StagedOptions opt = options ? *options : StagedOptions{};
    if (aux_) {
        opt.gaps.dgram_loaded = true;
        opt.gaps.min_gap = dgram_min_;
        opt.gaps.max_gap = dgram_max_;
    }
    if (shards_.size() > 1) return run_queries_sharded(shards_, enc_, regexes, status, messages, stats, &opt, aux_shards_);
    return run_queries(ix_, enc_, regexes, status, messages, stats, &opt, aux_);
}

std::vector<uint64_t> set_bins(const uint64_t* mask, uint64_t bins) {
    std::vector<uint64_t> out;
    if (bins == 1) { out.push_back(0); return out; }  // a 1-bin library is always scanned
    const uint64_t words = (bins + 63) / 64;
    for (uint64_t w = 0; w < words; ++w)
        for (uint64_t v = mask[w]; v; v &= v - 1) out.push_back(w * 64 + (unsigned)__builtin_ctzll(v));
    return out;
}

namespace {

struct DevBuf {
    void* p = nullptr;
    explicit DevBuf(size_t bytes) { txq_check(txq_malloc(&p, bytes), "txq_malloc"); }
    ~DevBuf() { txq_free(p); }
};

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
            DevBuf dv(vals.size() * 8), db(bins.size() * 4);
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
    DevBuf d_vals(chunk * 8), d_offs((B + 1) * 8);
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
    DevBuf d_regs(B * TXQ_HLL_REGISTERS);
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
        DevBuf d_order(B * 4), d_est(B * W * 8);
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
                DevBuf d_ids(longest_interval * 4), d_pairs(longest_interval * longest_interval * 8);
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
    std::vector<std::unique_ptr<DevBuf>> d_words;
    std::vector<txq_ibf_desc> descs(n_ibf);
    for (uint64_t i = 0; i < n_ibf; ++i) {
        const LayoutIbf& f = layout.ibfs[i];
        IbfImage& img = h.ibfs[i];
        img.shape(f.tb_to_user_bin.size(), f.bin_size, opt.hash_count);
        h.next_ibf_id.push_back(f.next_ibf_id);
        h.tb_to_user_bin.push_back(f.tb_to_user_bin);
        d_words.push_back(std::make_unique<DevBuf>(img.words.size() * 8));
        txq_check(txq_memcpy_h2d(d_words.back()->p, img.words.data(), img.words.size() * 8), "h2d zero words");
        descs[i] = txq_ibf_desc{img.bins, img.tech_bins, img.bin_size, img.hash_shift, img.bin_words, img.hash_funs, (const uint64_t*)d_words.back()->p};
    }
    std::vector<uint64_t> path_offsets(B + 1, 0), path;
    for (uint64_t b = 0; b < B; ++b) {
        for (const PathStep& st : paths[b]) { path.push_back(st.ibf); path.push_back(st.tb); path.push_back(st.parts); }
        path_offsets[b + 1] = path.size() / 3;
    }
    DevBuf d_descs(n_ibf * sizeof(txq_ibf_desc)), d_poff((B + 1) * 8), d_path(path.size() * 8);
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

namespace {
// a device buffer that only grows (one per kind for all batches of a call)
struct GrowBuf {
    void* p = nullptr;
    size_t cap = 0;
    void* reserve(size_t bytes) {
        if (bytes > cap || !p) {
            if (p) txq_free(p);
            p = nullptr;
            cap = 0;
            txq_check(txq_malloc(&p, std::max<size_t>(bytes, 256)), "txq_malloc");
            cap = std::max<size_t>(bytes, 256);
        }
        return p;
    }
    ~GrowBuf() { if (p) txq_free(p); }
};
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
    // a batch: at most 2^24 values (by their bound), and at most 256 MiB of hit words / counts
    const uint64_t max_values = (uint64_t)1 << 24;
    const size_t max_queries = std::max<size_t>(6, ((size_t)256 << 20) / (W * (with_counts ? 64 * 4 : 8)));
    GrowBuf d_codes, d_seq, d_rec, d_val, d_off, d_thr, d_hit, d_cnt, d_list, d_total;
    txq_check(txq_memcpy_h2d(d_codes.reserve(256), enc_.aa_table().data(), 256), "h2d");
    d_total.reserve(8);
    size_t list_cap = (size_t)1 << 20;
    std::vector<uint64_t> rebased, off;
    std::vector<uint32_t> thr, list;
    // --verify-frames
    const char* frames_env = std::getenv("TETREX_VERIFY_FRAMES");
    const bool frames_on_host = frames_env && std::string(frames_env) == "host";
    GrowBuf d_frames, d_foff;
    std::vector<BinVerifier::Candidate> candidates;
    std::vector<uint64_t> lengths;
    std::vector<std::string> frame_strings;
    std::vector<VerifiedHit> batch_confirmed;
    for (size_t r0 = 0; r0 < R;) {
        size_t r1 = r0;
        uint64_t bound = 0;
        while (r1 < R) {
            const uint64_t b = txq_translate_bound(rec_offsets.data() + r1, 1, k);
            if (b == UINT64_MAX) txq_check(TXQ_ERR_ARG, "txq_translate_bound");
            if (r1 > r0 && (bound + b > max_values || 6 * (r1 - r0 + 1) > max_queries)) break;
            bound += b;
            ++r1;
        }
        const size_t nr = r1 - r0, nq = 6 * nr;
        const uint64_t first = rec_offsets[r0], bytes = rec_offsets[r1] - first;
        rebased.assign(rec_offsets.begin() + r0, rec_offsets.begin() + r1 + 1);
        for (uint64_t& o : rebased) o -= first;
        if (bytes) txq_check(txq_memcpy_h2d(d_seq.reserve(bytes), seq.data() + first, bytes), "h2d");
        else d_seq.reserve(1);
        txq_check(txq_memcpy_h2d(d_rec.reserve(rebased.size() * 8), rebased.data(), rebased.size() * 8), "h2d");
        d_val.reserve(bound * 8 + 8);
        d_off.reserve((nq + 1) * 8);
        txq_check(txq_translate_device((const uint8_t*)d_seq.p, (const uint64_t*)d_rec.p, nr, k, (const uint8_t*)d_codes.p, (uint64_t*)d_val.p,
                                       (uint64_t*)d_off.p, nullptr), "txq_translate_device");
        off.resize(nq + 1);
        txq_check(txq_memcpy_d2h(off.data(), d_off.p, off.size() * 8), "d2h");
        thr.assign(nq, 0xFFFFFFFFu);  // (no count reaches it: a query that is not searched has no hits)
        bool any = false;
        for (size_t q = 0; q < nq; ++q) {
            const uint64_t n = off[q + 1] - off[q], t = n ? threshold_of(n) : 0;
            n_of[6 * r0 + q] = n;
            thresholds[6 * r0 + q] = t;
            if (t) thr[q] = (uint32_t)std::min<uint64_t>(t, 0xFFFFFFFEull), any = true;
        }
        r0 = r1;
        if (!any) continue;
        txq_check(txq_memcpy_h2d(d_thr.reserve(nq * 4), thr.data(), nq * 4), "h2d");
        d_hit.reserve(nq * W * 8);
        if (with_counts) d_cnt.reserve(nq * W * 64 * 4);
        txq_check(txq_count_device(ix_, (const uint64_t*)d_val.p, (const uint64_t*)d_off.p, nq, (const uint32_t*)d_thr.p, (uint64_t*)d_hit.p,
                                   with_counts ? (uint32_t*)d_cnt.p : nullptr, nullptr), "txq_count_device");
        uint64_t total = 0;
        for (;;) {
            d_list.reserve(list_cap * 12);
            txq_check(txq_hit_list_device((const uint64_t*)d_hit.p, with_counts ? (const uint32_t*)d_cnt.p : nullptr, nq, W, (uint32_t*)d_list.p,
                                          list_cap, (uint64_t*)d_total.p, nullptr), "txq_hit_list_device");
            txq_check(txq_memcpy_d2h(&total, d_total.p, 8), "d2h");
            if (total <= list_cap) break;
            list_cap = total;  // (the list did not fit: once more with room for all of it)
        }
        list.resize(3 * total);
        if (total) txq_check(txq_memcpy_d2h(list.data(), d_list.p, total * 12), "d2h");
        const uint32_t q0 = (uint32_t)(6 * (r1 - nr)), bin0 = (uint32_t)(info_.shard_word0 * 64);
        for (uint64_t i = 0; i < total; ++i) hits.push_back(TranslatedHit{q0 + list[3 * i], bin0 + list[3 * i + 1], list[3 * i + 2]});
        if (!verifier || total == 0) continue;
        // --verify-frames: the batch's hits are candidates, pattern index = query index within the batch
        candidates.resize(total);
        for (uint64_t i = 0; i < total; ++i) candidates[i] = BinVerifier::Candidate{list[3 * i], bin0 + list[3 * i + 1]};
        const auto frame_letters = [&](uint32_t q) {
            return translate_frame(seq.substr(first + rebased[q / 6], rebased[q / 6 + 1] - rebased[q / 6]), q % 6);
        };
        if (frames_on_host) {
            frame_strings.assign(nq, std::string());
            for (const BinVerifier::Candidate& c : candidates)
                if (frame_strings[c.query].empty()) frame_strings[c.query] = frame_letters(c.query);
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
    const uint64_t max_values = (uint64_t)1 << 24;
    size_t max_windows = std::max<size_t>(1, ((size_t)256 << 20) / (W * (with_counts ? 64 * 4 : 8)));
    if (const char* e = std::getenv("TETREX_SEARCH_BATCH_WINDOWS"); e && *e) max_windows = std::min<size_t>(max_windows, std::max<long long>(1, std::atoll(e)));
    const bool trace = std::getenv("TETREX_TRACE") != nullptr;
    GrowBuf d_val, d_beg, d_len, d_thr, d_hit, d_cnt, d_list, d_total;
    d_total.reserve(8);
    size_t list_cap = (size_t)1 << 20;
    std::vector<uint64_t> beg;
    std::vector<uint32_t> thr, list;
    // the batches: windows [cut[i], cut[i + 1]), values [begin of the first, end of the last) (a window longer than the bound
    // on values: a batch of its own).  The buffers are sized for the largest batch before the first one runs, so that no
    // device memory is freed or allocated between the launches of a call.
    std::vector<size_t> cut{0};
    size_t most_windows = 0;
    uint64_t most_values = 0;
    for (size_t j0 = 0; j0 < N;) {
        size_t j1 = j0;
        while (j1 < N && j1 - j0 < max_windows && (j1 == j0 || begins[j1] + lens[j1] - begins[j0] <= max_values)) ++j1;
        most_windows = std::max(most_windows, j1 - j0);
        most_values = std::max(most_values, begins[j1 - 1] + lens[j1 - 1] - begins[j0]);
        cut.push_back(j0 = j1);
    }
    d_val.reserve(most_values * 8 + 8);
    d_beg.reserve(most_windows * 8);
    d_len.reserve(most_windows * 4);
    d_thr.reserve(most_windows * 4);
    d_hit.reserve(most_windows * W * 8);
    if (with_counts) d_cnt.reserve(most_windows * W * 64 * 4);
    d_list.reserve(list_cap * 12);
    for (size_t c = 0; c + 1 < cut.size(); ++c) {
        const size_t first = cut[c], j1 = cut[c + 1], n = j1 - first;
        const uint64_t v0 = begins[first], v1 = begins[j1 - 1] + lens[j1 - 1];
        bool any = false;
        for (size_t j = first; j < j1; ++j) any = any || thresholds[j] > 0;
        if (!any) continue;
        beg.assign(begins.begin() + first, begins.begin() + j1);
        for (uint64_t& b : beg) b -= v0;
        thr.assign(thresholds.begin() + first, thresholds.begin() + j1);
        for (uint32_t& t : thr)
            if (t == 0) t = 0xFFFFFFFFu;  // (no count reaches it: a window that is not searched has no hits)
        if (v1 > v0) txq_check(txq_memcpy_h2d(d_val.p, values.data() + v0, (v1 - v0) * 8), "h2d");
        txq_check(txq_memcpy_h2d(d_beg.p, beg.data(), n * 8), "h2d");
        txq_check(txq_memcpy_h2d(d_len.p, lens.data() + first, n * 4), "h2d");
        txq_check(txq_memcpy_h2d(d_thr.p, thr.data(), n * 4), "h2d");
        txq_check(txq_count_windows_device(ix_, (const uint64_t*)d_val.p, (const uint64_t*)d_beg.p, (const uint32_t*)d_len.p, n, (const uint32_t*)d_thr.p,
                                           (uint64_t*)d_hit.p, with_counts ? (uint32_t*)d_cnt.p : nullptr, nullptr), "txq_count_windows_device");
        uint64_t total = 0;
        for (;;) {
            d_list.reserve(list_cap * 12);
            txq_check(txq_hit_list_device((const uint64_t*)d_hit.p, with_counts ? (const uint32_t*)d_cnt.p : nullptr, n, W, (uint32_t*)d_list.p,
                                          list_cap, (uint64_t*)d_total.p, nullptr), "txq_hit_list_device");
            txq_check(txq_memcpy_d2h(&total, d_total.p, 8), "d2h");
            if (total <= list_cap) break;
            list_cap = total;  // (the list did not fit: once more with room for all of it)
        }
        list.resize(3 * total);
        if (total) txq_check(txq_memcpy_d2h(list.data(), d_list.p, total * 12), "d2h");
        if (trace)
            std::fprintf(stderr, "[tetrex search] window batch: windows %zu..%zu, values %llu..%llu, %llu hits\n", first, j1, (unsigned long long)v0,
                         (unsigned long long)v1, (unsigned long long)total);
        const uint32_t bin0 = (uint32_t)(info_.shard_word0 * 64);
        for (uint64_t i = 0; i < total; ++i) hits.push_back(TranslatedHit{(uint32_t)first + list[3 * i], bin0 + list[3 * i + 1], list[3 * i + 2]});
    }
}

void DeviceIndex::search_translated_windows(std::string_view seq, const std::vector<uint64_t>& rec_offsets, uint32_t window, uint32_t step,
                                            const std::function<uint64_t(uint64_t)>& threshold_of, bool with_counts,
                                            std::vector<uint64_t>& win_offsets, std::vector<uint32_t>& lens, std::vector<uint32_t>& thresholds,
                                            std::vector<TranslatedHit>& hits) {
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
    if (R == 0 || W == 0 || N == 0) return;
    const uint64_t max_values = (uint64_t)1 << 24;
    size_t max_windows = std::max<size_t>(1, ((size_t)256 << 20) / (W * (with_counts ? 64 * 4 : 8)));
    if (const char* e = std::getenv("TETREX_SEARCH_BATCH_WINDOWS"); e && *e) max_windows = std::min<size_t>(max_windows, std::max<long long>(1, std::atoll(e)));
    const bool trace = std::getenv("TETREX_TRACE") != nullptr;
    // the record batches [cut[i], cut[i + 1]): at most 2^24 values by their bound, a larger record alone.  The buffers are sized
    // for the largest batch before the first one runs, so that no device memory of the call is freed or allocated between
    // its launches ("Host").
    std::vector<size_t> cut{0};
    uint64_t most_values = 0, most_bytes = 0, most_windows = 0;
    size_t most_records = 0;
    for (size_t r0 = 0; r0 < R;) {
        size_t r1 = r0;
        uint64_t bound = 0;
        while (r1 < R) {
            const uint64_t b = txq_translate_bound(rec_offsets.data() + r1, 1, k);
            if (b == UINT64_MAX) txq_check(TXQ_ERR_ARG, "txq_translate_bound");
            if (r1 > r0 && bound + b > max_values) break;
            bound += b;
            ++r1;
        }
        most_values = std::max(most_values, bound);
        most_bytes = std::max(most_bytes, rec_offsets[r1] - rec_offsets[r0]);
        most_windows = std::max(most_windows, win_offsets[6 * r1] - win_offsets[6 * r0]);
        most_records = std::max(most_records, r1 - r0);
        cut.push_back(r0 = r1);
    }
    const size_t sub_windows = (size_t)std::min<uint64_t>(most_windows, max_windows);
    GrowBuf d_codes, d_seq, d_rec, d_val, d_off, d_woff, d_beg, d_len, d_thr, d_hit, d_cnt, d_list, d_total;
    txq_check(txq_memcpy_h2d(d_codes.reserve(256), enc_.aa_table().data(), 256), "h2d");
    d_total.reserve(8);
    size_t list_cap = (size_t)1 << 20;
    d_seq.reserve(most_bytes + 16);
    d_rec.reserve((most_records + 1) * 8);
    d_val.reserve(most_values * 8 + 8);
    d_off.reserve((6 * most_records + 1) * 8);
    d_woff.reserve((6 * most_records + 1) * 8);
    d_beg.reserve(most_windows * 8 + 8);
    d_len.reserve(most_windows * 4 + 8);
    d_thr.reserve(most_windows * 4 + 8);
    d_hit.reserve(sub_windows * W * 8);
    if (with_counts) d_cnt.reserve(sub_windows * W * 64 * 4);
    d_list.reserve(list_cap * 12);
    std::vector<uint64_t> rebased;
    std::vector<uint32_t> thr, list;
    const uint32_t bin0 = (uint32_t)(info_.shard_word0 * 64);
    for (size_t c = 0; c + 1 < cut.size(); ++c) {
        const size_t r0 = cut[c], r1 = cut[c + 1], nr = r1 - r0;
        const uint64_t w0 = win_offsets[6 * r0], nw = win_offsets[6 * r1] - w0;
        if (nw == 0) continue;
        const uint64_t first = rec_offsets[r0], bytes = rec_offsets[r1] - first;
        rebased.assign(rec_offsets.begin() + r0, rec_offsets.begin() + r1 + 1);
        for (uint64_t& o : rebased) o -= first;
        txq_check(txq_memcpy_h2d(d_seq.p, seq.data() + first, bytes), "h2d");
        txq_check(txq_memcpy_h2d(d_rec.p, rebased.data(), rebased.size() * 8), "h2d");
        txq_check(txq_translate_windows_device((const uint8_t*)d_seq.p, (const uint64_t*)d_rec.p, nr, k, (const uint8_t*)d_codes.p, window, step,
                                               (uint64_t*)d_val.p, (uint64_t*)d_off.p, (uint64_t*)d_woff.p, (uint64_t*)d_beg.p, (uint32_t*)d_len.p, nullptr),
                  "txq_translate_windows_device");
        txq_check(txq_memcpy_d2h(lens.data() + w0, d_len.p, nw * 4), "d2h");
        thr.assign(nw, 0xFFFFFFFFu);  // (no count reaches it: a window that is not searched has no hits)
        bool any = false;
        for (uint64_t j = 0; j < nw; ++j) {
            const uint64_t w = lens[w0 + j], t = w ? threshold_of(w) : 0;
            if (t) thresholds[w0 + j] = thr[j] = (uint32_t)std::min<uint64_t>(t, 0xFFFFFFFEull), any = true;
        }
        if (!any) continue;
        txq_check(txq_memcpy_h2d(d_thr.p, thr.data(), nw * 4), "h2d");
        // sub-ranges of the batch's windows: the begins are absolute in the batch's values, so nothing is sent again
        for (uint64_t j0 = 0; j0 < nw; j0 += sub_windows) {
            const size_t n = (size_t)std::min<uint64_t>(sub_windows, nw - j0);
            bool some = false;
            for (size_t j = 0; j < n && !some; ++j) some = thr[j0 + j] != 0xFFFFFFFFu;
            if (!some) continue;
            txq_check(txq_count_windows_device(ix_, (const uint64_t*)d_val.p, (const uint64_t*)d_beg.p + j0, (const uint32_t*)d_len.p + j0, n,
                                               (const uint32_t*)d_thr.p + j0, (uint64_t*)d_hit.p, with_counts ? (uint32_t*)d_cnt.p : nullptr, nullptr),
                      "txq_count_windows_device");
            uint64_t total = 0;
            for (;;) {
                d_list.reserve(list_cap * 12);
                txq_check(txq_hit_list_device((const uint64_t*)d_hit.p, with_counts ? (const uint32_t*)d_cnt.p : nullptr, n, W, (uint32_t*)d_list.p,
                                              list_cap, (uint64_t*)d_total.p, nullptr), "txq_hit_list_device");
                txq_check(txq_memcpy_d2h(&total, d_total.p, 8), "d2h");
                if (total <= list_cap) break;
                list_cap = total;  // (the list did not fit: once more with room for all of it)
            }
            list.resize(3 * total);
            if (total) txq_check(txq_memcpy_d2h(list.data(), d_list.p, total * 12), "d2h");
            if (trace)
                std::fprintf(stderr, "[tetrex search] frame window batch: records %zu..%zu, windows %llu..%llu, %llu hits\n", r0, r1,
                             (unsigned long long)(w0 + j0), (unsigned long long)(w0 + j0 + n), (unsigned long long)total);
            for (uint64_t i = 0; i < total; ++i)
                hits.push_back(TranslatedHit{(uint32_t)(w0 + j0) + list[3 * i], bin0 + list[3 * i + 1], list[3 * i + 2]});
        }
    }
}

// ---- tetrex search --verify --------------------------------------------------------------------------------------------

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
    const uint64_t bytes = text.size() + 16 + rec.size() * 8;
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
    const auto reverse_complement = [](const std::string& s) {
        std::string out(s.rbegin(), s.rend());
        for (char& c : out) switch (c & 0xDF) {
            case 'A': c = 'T'; break;
            case 'C': c = 'G'; break;
            case 'G': c = 'C'; break;
            case 'T': case 'U': c = 'A'; break;
            default: c = 'N'; break;  // (no class: matches nothing, as the byte it stands for)
        }
        return out;
    };
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
    DevBuf d_pat(pat.size() + 16), d_po(pat_off.size() * 8);
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

void BinVerifier::run(const DevicePatterns& patterns, size_t strands, const std::vector<Candidate>& candidates, const std::vector<uint32_t>& pattern_of,
                      const std::vector<uint64_t>& lengths, const std::function<std::string(size_t, size_t)>& letters, std::vector<Hit>& hits,
                      std::vector<std::vector<Hit>>* rows) {
    if (rows) return run_targets(patterns, strands, candidates, pattern_of, lengths, letters, *rows);
    n_candidates_ += candidates.size();
    std::vector<size_t> order(candidates.size()), on_host;
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return candidates[x].bin < candidates[y].bin; });
    // candidate of every `strands` pairs, by bin: patterns of up to TXQ_EDIT_MAX_PATTERN letters first, behind them those of up
    // to TXQ_EDIT_LONG_MAX_PATTERN, which the long-pattern kernel answers (TETREX_VERIFY_LONG=0: the host, for A/B runs)
    const size_t longest = device_max();
    std::vector<size_t> on_device, on_long;
    for (size_t i : order) {
        if (lengths[i] == 0 || lengths[i] > longest) on_host.push_back(i);
        else (lengths[i] > TXQ_EDIT_MAX_PATTERN ? on_long : on_device).push_back(i);
    }
    const size_t n_short = on_device.size();
    on_device.insert(on_device.end(), on_long.begin(), on_long.end());
    n_device_ += n_short, n_device_long_ += on_long.size(), n_host_ += on_host.size();
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
    // --align: the alignment of the strand that settle kept.  On the device unless TETREX_VERIFY_ALIGN=host says otherwise; what
    // the device declines, and the pairs of the host route, wait in `pending` for the host twin.
    const char* align_env = std::getenv("TETREX_VERIFY_ALIGN");
    const bool align_on_device = align_ && !(align_env && std::string(align_env) == "host");
    const uint32_t device_errors = std::min<uint32_t>(errors_, TXQ_EDIT_ALIGN_MAX_DISTANCE);  // (the device declines more anyway)
    const size_t stride = TXQ_EDIT_ALIGN_STRIDE(device_errors);
    struct Pending { size_t candidate, strand; uint32_t d, r, j; };
    std::vector<Pending> pending;
    const auto align_on_host = [&](const Pending& p, const std::string& text, const std::vector<uint64_t>& rec) {
        const std::string pattern = letters(p.candidate, p.strand);
        EditAlignment a;
        if (p.r + 1 >= rec.size() ||
            !edit_align((const uint8_t*)pattern.data(), pattern.size(), (const uint8_t*)text.data() + rec[p.r], (size_t)(rec[p.r + 1] - rec[p.r]), p.d, p.j, codes_, a))
            throw std::runtime_error("tetrex search --align: a confirmed pair has no alignment (bin " + std::to_string(candidates[p.candidate].bin) + ")");
        hits[p.candidate].start = a.start;
        hits[p.candidate].runs = std::move(a.runs);
    };
    if (!on_device.empty()) {
        std::vector<uint32_t> pairs;
        pairs.reserve(on_device.size() * strands * 3);
        for (size_t i : on_device)
            for (size_t s = 0; s < strands; ++s) {
                pairs.push_back(pattern_of[i] + (uint32_t)s);
                pairs.push_back(0);
                pairs.push_back(errors_);
            }
        // (the alignments lie behind the triples: one buffer, one copy back)
        const size_t n_pairs = pairs.size() / 3, align_words = align_on_device ? n_pairs * stride : 0;
        DevBuf d_pairs(pairs.size() * 4), d_out((pairs.size() + align_words) * 4);
        uint32_t* const d_align = (uint32_t*)d_out.p + pairs.size();
        static_assert(TXQ_EDIT_LONG_WORKSPACE(7) == TXQ_EDIT_WORKSPACE(7), "one workspace, cut the same way for either call");
        DevBuf d_work(TXQ_EDIT_WORKSPACE(pairs.size() / 3) + 8 * on_device.size());  // (every call its own part: they are all in flight at once)
        size_t n_calls = 0;
        txq_check(txq_memcpy_h2d(d_pairs.p, pairs.data(), pairs.size() * 4), "h2d");
        for (size_t a = 0; a < on_device.size();) {  // one call per bin and kernel: the bin's records are one group
            size_t b = a;
            const uint32_t bin = candidates[on_device[a]].bin;
            const bool is_long = a >= n_short;
            while (b < (is_long ? on_device.size() : n_short) && candidates[on_device[b]].bin == bin) ++b;
            ResidentBins::Bin& e = bins_.resident(bin);
            const uint64_t* d_rec = (const uint64_t*)e.d_rec;
            txq_check((is_long ? txq_edit_search_long_device : txq_edit_search_device)(patterns.d_letters, patterns.d_offsets, patterns.n_patterns, patterns.bytes, (const uint8_t*)e.d_text, d_rec,
                                             e.n_records, e.text_bytes, d_rec + e.n_records + 1, 1, (const uint32_t*)d_pairs.p + 3 * strands * a,
                                             (b - a) * strands, (const uint8_t*)d_codes_, (uint32_t*)d_out.p + 3 * strands * a,
                                             (unsigned char*)d_work.p + 16 * strands * a + 8 * n_calls++, nullptr),
                      is_long ? "txq_edit_search_long_device" : "txq_edit_search_device");
            if (align_on_device)  // behind the search call on its stream: the triples are read where it left them
                txq_check(txq_edit_align_device(patterns.d_letters, patterns.d_offsets, patterns.n_patterns, patterns.bytes, (const uint8_t*)e.d_text, d_rec,
                                                e.n_records, e.text_bytes, d_rec + e.n_records + 1, 1, (const uint32_t*)d_pairs.p + 3 * strands * a,
                                                (b - a) * strands, (const uint32_t*)d_out.p + 3 * strands * a, (const uint8_t*)d_codes_, device_errors,
                                                d_align + stride * strands * a, nullptr, nullptr),
                          "txq_edit_align_device");
            a = b;
        }
        std::vector<uint32_t> out(pairs.size() + align_words);
        txq_check(txq_memcpy_d2h(out.data(), d_out.p, out.size() * 4), "d2h");  // (waits for the kernels)
        for (size_t k = 0; k < on_device.size(); ++k) {
            const uint32_t* res = out.data() + 3 * strands * k;
            const size_t i = on_device[k], kept = settle(i, res, bins_.at(candidates[i].bin).names);
            if (!align_ || kept == strands) continue;
            const uint32_t* words = out.data() + pairs.size() + stride * (strands * k + kept);
            if (align_on_device && words[0] < kEditNotAligned) {
                hits[i].start = words[0];
                hits[i].runs.assign(words + 2, words + 2 + words[1]);
                ++n_align_device_;
            } else pending.push_back({i, kept, res[3 * kept], res[3 * kept + 1], res[3 * kept + 2]});
        }
    }
    // records too long for the device: the bin is read once more, the pairs of a bin run side by side
    for (size_t a = 0; a < on_host.size();) {
        size_t b = a;
        const uint32_t bin = candidates[on_host[a]].bin;
        while (b < on_host.size() && candidates[on_host[b]].bin == bin) ++b;
        std::string text;
        std::vector<uint64_t> rec;
        std::vector<std::string> names;
        bins_.read(bin, text, rec, names);
        if (bins_.at(bin).names.empty()) bins_.at(bin).names = std::move(names);  // (else they are the same, and hits point into them)
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
        for (size_t k = a; k < b; ++k) {
            const uint32_t* res = out.data() + 3 * strands * (k - a);
            const size_t kept = settle(on_host[k], res, bins_.at(bin).names);
            if (!align_ || kept == strands) continue;
            align_on_host({on_host[k], kept, res[3 * kept], res[3 * kept + 1], res[3 * kept + 2]}, text, rec);
            ++n_align_host_;
        }
        a = b;
    }
    // alignments the device did not make: a bin's letters are read once more, its pairs run side by side
    std::stable_sort(pending.begin(), pending.end(), [&](const Pending& x, const Pending& y) { return candidates[x.candidate].bin < candidates[y.candidate].bin; });
    for (size_t a = 0; a < pending.size();) {
        size_t b = a;
        const uint32_t bin = candidates[pending[a].candidate].bin;
        while (b < pending.size() && candidates[pending[b].candidate].bin == bin) ++b;
        std::string text;
        std::vector<uint64_t> rec;
        std::vector<std::string> names;
        bins_.read(bin, text, rec, names);
        std::exception_ptr failed;
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic)
#endif
        for (size_t k = a; k < b; ++k) {
            try {
                align_on_host(pending[k], text, rec);
            } catch (...) {
#ifdef _OPENMP
#pragma omp critical(tetrex_align_failed)
#endif
                failed = std::current_exception();
            }
        }
        if (failed) std::rethrow_exception(failed);
        n_align_host_ += b - a;
        a = b;
    }
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
                              const std::vector<uint64_t>& lengths, const std::function<std::string(size_t, size_t)>& letters,
                              std::vector<std::vector<Hit>>& rows) {
    rows.assign(candidates.size(), {});
    n_candidates_ += candidates.size();
    std::vector<size_t> order(candidates.size()), on_host, on_device, on_long;
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return candidates[x].bin < candidates[y].bin; });
    const char* route_env = std::getenv("TETREX_VERIFY_TARGETS");
    const bool all_on_host = route_env && std::string(route_env) == "host";
    const size_t longest = device_max();
    const uint64_t budget = target_slot_budget();
    for (size_t i : order) {
        if (all_on_host || lengths[i] == 0 || lengths[i] > longest) on_host.push_back(i);
        else (lengths[i] > TXQ_EDIT_MAX_PATTERN ? on_long : on_device).push_back(i);
    }
    // what the routes find: (record, strand, distance, end) of every hit of a candidate; settled below
    struct Found { uint32_t r, strand, d, j; };
    std::vector<std::vector<Found>> found(candidates.size());

    // the device: one call per bin, kernel and at most `budget` slots, queued in rounds with one copy back each
    struct Call { uint32_t bin; bool is_long; size_t first, n_pairs; uint64_t n_records; size_t row0, work0; };
    const auto run_round = [&](const std::vector<Call>& calls, const std::vector<uint32_t>& pairs, const std::vector<size_t>& owner, size_t n_rows, size_t work_bytes) {
        const size_t n_pairs = pairs.size() / 3;
        DevBuf d_pairs(pairs.size() * 4 + 4), d_hits(n_rows * 16 + 16), d_total(calls.size() * 8), d_status(n_pairs * 4 + 4), d_work(work_bytes + 8);
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
        const size_t n_short = on_device.size();
        on_device.insert(on_device.end(), on_long.begin(), on_long.end());
        std::vector<Call> calls;
        std::vector<uint32_t> pairs;
        std::vector<size_t> owner;  // the candidate of every `strands` pairs of the round
        size_t n_rows = 0, work_bytes = 0;
        const auto flush_round = [&]() {
            if (!calls.empty()) run_round(calls, pairs, owner, n_rows, work_bytes);
            calls.clear(), pairs.clear(), owner.clear();
            n_rows = work_bytes = 0;
        };
        for (size_t a = 0; a < on_device.size();) {
            size_t b = a;
            const uint32_t bin = candidates[on_device[a]].bin;
            const bool is_long = a >= n_short;
            while (b < (is_long ? on_device.size() : n_short) && candidates[on_device[b]].bin == bin) ++b;
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
                a = b;
                continue;
            }
            (is_long ? n_device_long_ : n_device_) += b - a;
            const size_t first = pairs.size() / 3;
            for (size_t k = a; k < b; ++k) {
                owner.push_back(on_device[k]);
                for (size_t s = 0; s < strands; ++s) {
                    pairs.push_back(pattern_of[on_device[k]] + (uint32_t)s);
                    pairs.push_back(0);
                    pairs.push_back(errors_);
                }
            }
            const size_t n_pairs = (b - a) * strands, per_call = (size_t)std::max<uint64_t>(1, n_records ? budget / n_records : n_pairs);
            for (size_t p = 0; p < n_pairs; p += per_call) {
                const size_t np = std::min(per_call, n_pairs - p), n_slots = np * n_records;
                calls.push_back({bin, is_long, first + p, np, n_records, n_rows, work_bytes});
                n_rows += n_slots;
                work_bytes += TXQ_EDIT_TARGETS_WORKSPACE(np, n_slots);
            }
            a = b;
            // (pairs of one candidate stay in one round: a round ends between bins)
            if (n_rows >= 8 * budget) flush_round();
        }
        flush_round();
    }
    // the host: what is too long or empty, bins of more records than a call's slots, and with TETREX_VERIFY_TARGETS=host everything
    std::stable_sort(on_host.begin(), on_host.end(), [&](size_t x, size_t y) { return candidates[x].bin < candidates[y].bin; });
    n_host_ += on_host.size();
    for (size_t a = 0; a < on_host.size();) {
        size_t b = a;
        const uint32_t bin = candidates[on_host[a]].bin;
        while (b < on_host.size() && candidates[on_host[b]].bin == bin) ++b;
        std::string text;
        std::vector<uint64_t> rec;
        std::vector<std::string> names;
        bins_.read(bin, text, rec, names);
        if (bins_.at(bin).names.empty()) bins_.at(bin).names = std::move(names);  // (else they are the same, and hits point into them)
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
        a = b;
    }
    // settle: a target's row is its better strand, + on equal distance; rows in the order of the bin's file
    struct ToAlign { size_t candidate, row; uint32_t strand, d, r, j; };
    std::vector<ToAlign> to_align;
    for (size_t i : order) {
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
    const char* align_env = std::getenv("TETREX_VERIFY_ALIGN");
    const bool align_on_device = !(align_env && std::string(align_env) == "host");
    const uint32_t device_errors = std::min<uint32_t>(errors_, TXQ_EDIT_ALIGN_MAX_DISTANCE);
    const size_t stride = TXQ_EDIT_ALIGN_STRIDE(device_errors);
    std::vector<size_t> pending, sent;
    for (size_t t = 0; t < to_align.size(); ++t) {
        const size_t i = to_align[t].candidate;
        const bool reachable = align_on_device && pattern_of[i] != 0xFFFFFFFFu && lengths[i] >= 1 && lengths[i] <= TXQ_EDIT_LONG_MAX_PATTERN &&
                               to_align[t].d <= device_errors;
        (reachable ? sent : pending).push_back(t);
    }
    if (!sent.empty()) {
        std::vector<uint32_t> pairs, triples;
        for (size_t t : sent) {
            const ToAlign& x = to_align[t];
            pairs.insert(pairs.end(), {pattern_of[x.candidate] + x.strand, 0u, errors_});
            triples.insert(triples.end(), {x.d, x.r, x.j});
        }
        DevBuf d_pairs(pairs.size() * 4), d_triples(triples.size() * 4), d_align(sent.size() * stride * 4);
        txq_check(txq_memcpy_h2d(d_pairs.p, pairs.data(), pairs.size() * 4), "h2d");
        txq_check(txq_memcpy_h2d(d_triples.p, triples.data(), triples.size() * 4), "h2d");
        for (size_t a = 0; a < sent.size();) {
            size_t b = a;
            const uint32_t bin = candidates[to_align[sent[a]].candidate].bin;
            while (b < sent.size() && candidates[to_align[sent[b]].candidate].bin == bin) ++b;
            ResidentBins::Bin& e = bins_.resident(bin);
            const uint64_t* d_rec = (const uint64_t*)e.d_rec;
            txq_check(txq_edit_align_device(patterns.d_letters, patterns.d_offsets, patterns.n_patterns, patterns.bytes, (const uint8_t*)e.d_text, d_rec,
                                            e.n_records, e.text_bytes, d_rec + e.n_records + 1, 1, (const uint32_t*)d_pairs.p + 3 * a, b - a,
                                            (const uint32_t*)d_triples.p + 3 * a, (const uint8_t*)d_codes_, device_errors, (uint32_t*)d_align.p + stride * a,
                                            nullptr, nullptr),
                      "txq_edit_align_device");
            a = b;
        }
        std::vector<uint32_t> words(sent.size() * stride);
        txq_check(txq_memcpy_d2h(words.data(), d_align.p, words.size() * 4), "d2h");  // (waits for the kernels)
        for (size_t k = 0; k < sent.size(); ++k) {
            const uint32_t* w = words.data() + stride * k;
            const ToAlign& x = to_align[sent[k]];
            if (w[0] < kEditNotAligned) {
                rows[x.candidate][x.row].start = w[0];
                rows[x.candidate][x.row].runs.assign(w + 2, w + 2 + w[1]);
                ++n_align_device_;
            } else pending.push_back(sent[k]);
        }
    }
    std::stable_sort(pending.begin(), pending.end(), [&](size_t x, size_t y) { return candidates[to_align[x].candidate].bin < candidates[to_align[y].candidate].bin; });
    for (size_t a = 0; a < pending.size();) {
        size_t b = a;
        const uint32_t bin = candidates[to_align[pending[a]].candidate].bin;
        while (b < pending.size() && candidates[to_align[pending[b]].candidate].bin == bin) ++b;
        std::string text;
        std::vector<uint64_t> rec;
        std::vector<std::string> names;
        bins_.read(bin, text, rec, names);
        bool failed = false;
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic)
#endif
        for (size_t k = a; k < b; ++k) {
            const ToAlign& x = to_align[pending[k]];
            const std::string pattern = letters(x.candidate, x.strand);
            EditAlignment al;
            if (x.r + 1 >= rec.size() || !edit_align((const uint8_t*)pattern.data(), pattern.size(), (const uint8_t*)text.data() + rec[x.r],
                                                     (size_t)(rec[x.r + 1] - rec[x.r]), x.d, x.j, codes_, al)) {
#ifdef _OPENMP
#pragma omp atomic write
#endif
                failed = true;
                continue;
            }
            rows[x.candidate][x.row].start = al.start;
            rows[x.candidate][x.row].runs = std::move(al.runs);
        }
        if (failed) throw std::runtime_error("tetrex search --align: a confirmed pair has no alignment (bin " + std::to_string(bin) + ")");
        n_align_host_ += b - a;
        a = b;
    }
}

// ---- tetrex query --gpu-verify -----------------------------------------------------------------------------------------

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
    DevBuf d_arena(arena.size() + 16), d_arena_off(arena_off.size() * 8);
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
        DevBuf d_pairs(n_pairs * 8 + 8), d_out_off(n_pairs * 8 + 8), d_out(n_words * 4 + 4), d_status(n_pairs * 4 + 4),
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
