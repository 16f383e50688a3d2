// C-ABI (include/txq.h) of the MI355X TetRex query engine: index residency in HBM and the
// entry points the reference's seam would bind.  No CPU fallback: without a GPU every call
// that needs one fails with TXQ_ERR_STATE.
#include "../../include/txq.h"
#include "txq_internal.hpp"
#include "txq_count_windows_tree_plan.hpp"
#include "txq_hibf_plan.hpp"

#include <algorithm>
#include <cstdarg>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

namespace txq {

static thread_local std::string g_err;
static std::vector<int> g_devices;  // txq_init: shard r of an index lives on g_devices[r % size]

static std::mutex g_spare_mutex;
static std::map<int, std::vector<hipStream_t>> g_spare_streams;  // per device: streams created at txq_init for the first sessions
hipStream_t take_spare_stream(int device) {
    std::lock_guard<std::mutex> lk(g_spare_mutex);
    auto it = g_spare_streams.find(device);
    if (it == g_spare_streams.end() || it->second.empty()) return nullptr;
    hipStream_t st = it->second.back();
    it->second.pop_back();
    return st;
}

static Knobs g_knobs;
static std::mutex g_knobs_mutex;
Knobs knobs() {
    std::lock_guard<std::mutex> lock(g_knobs_mutex);
    return g_knobs;
}
void read_knobs() {
    auto flag = [](const char* name) { return std::getenv(name) != nullptr; };
    auto is = [](const char* name, char c) { const char* e = std::getenv(name); return e && e[0] == c; };
    auto num = [](const char* name, long long otherwise) { const char* e = std::getenv(name); return e && *e ? std::atoll(e) : otherwise; };
    Knobs k;
    k.trace = flag("TXQ_TRACE");
    k.trace_stages = flag("TXQ_TRACE_STAGES");
    k.trace_sync = flag("TXQ_TRACE_SYNC");
    k.dense_tree = (int)num("TXQ_DENSE_TREE", -1);
    k.dense_unroll = (int)num("TXQ_DENSE_UNROLL", 3);
    k.dense_slices = (int)std::max(1LL, num("TXQ_DENSE_SLICES", 2));
    k.dense_tile_rounds = (int)std::max(1LL, num("TXQ_DENSE_TILE_ROUNDS", 4));
    k.dense_nt = (int)num("TXQ_DENSE_NT", 0) & 3;
    k.fuse_units = !is("TXQ_FUSE_UNITS", '0');
    k.one_stream = flag("TXQ_ONE_STREAM");
    k.sparse_steps = !is("TXQ_SPARSE_STEPS", '0');
    k.sparse_unroll = (int)num("TXQ_SPARSE_UNROLL", 3);
    k.sparse_units = (int)std::min(1536LL, std::max(64LL, num("TXQ_SPARSE_UNITS", 512)));
    k.kmer_table_mb = std::max(0LL, num("TXQ_KMER_TABLE_MB", 512));
    k.kmer_table_min = std::max(1LL, num("TXQ_KMER_TABLE_MIN", 16));
    k.hibf_interleave = !is("TXQ_HIBF_INTERLEAVE", '0');
    k.hibf_interleave_probe = !is("TXQ_HIBF_INTERLEAVE_PROBE", '0');
    k.hibf_levels = is("TXQ_HIBF_LEVELS", '1');
    k.hibf_stationary = !is("TXQ_HIBF_STATIONARY", '0');
    k.hibf_small = !is("TXQ_HIBF_SMALL", '0');
    k.hibf_lane_hash = flag("TXQ_HIBF_LANE_HASH");
    k.hibf_layout_order = !is("TXQ_HIBF_LAYOUT_ORDER", '0');
    k.hibf_layout_fused = !is("TXQ_HIBF_LAYOUT_FUSED", '0');
    k.final_pinned = !is("TXQ_FINAL_PINNED", '0');
    k.hibf_steps_per_group = (int)std::max(0LL, num("TXQ_HIBF_STEPS_PER_GROUP", 0));
    k.hibf_tile = (int)std::max(0LL, num("TXQ_HIBF_TILE", 0));
    k.hibf_unroll = (int)num("TXQ_HIBF_UNROLL", 1);
    k.hibf_store = (int)num("TXQ_HIBF_STORE_KIND", 0) & 3;  // which store instruction writes the rows
#ifdef TXQ_EXPERIMENTS
    // timing experiments of tools/ab_hibf*.sh (`make EXPERIMENTS=1`): bit 4 no row gathers, bit 5 (almost) no stores — WRONG masks,
    // which is why the product build does not contain them
    k.hibf_store |= (int)num("TXQ_HIBF_STORE", 0) & 112;  // (64: the layout-order level kernel without its gate loads)
#endif
    k.hibf_waves = std::max(0LL, num("TXQ_HIBF_WAVES", 0));
    k.hibf_stack_lds = std::max(2LL, num("TXQ_HIBF_STACK_LDS", 128));
    k.hibf_layout_direct = num("TXQ_HIBF_LAYOUT_DIRECT", 1) != 0;
    k.probe_blocks_per_cu = (int)std::max(1LL, num("TXQ_PROBE_BLOCKS_PER_CU", 256));
    k.probe_unroll = (int)num("TXQ_PROBE_UNROLL", 2);
    k.probe_nt = flag("TXQ_PROBE_NT");
    k.probe_table = is("TXQ_PROBE_TABLE", '0') ? 0 : is("TXQ_PROBE_TABLE", '1') ? 1 : -1;
    k.probe_table_keep = !is("TXQ_PROBE_TABLE_KEEP", '0');
    k.probe_table_fused = !is("TXQ_PROBE_TABLE_FUSED", '0');
    k.probe_table_tile = !is("TXQ_PROBE_TABLE_TILE", '0');
    k.probe_sort = !is("TXQ_PROBE_SORT", '0');
    k.probe_sort_min = std::max(1LL, num("TXQ_PROBE_SORT_MIN", kSortMinDefault));
    k.probe_sort_bucket_kb = std::max(1LL, num("TXQ_PROBE_SORT_BUCKET_KB", kSortBucketKbDefault));
#ifdef TXQ_EXPERIMENTS
    // timing experiment of tools/ab_probe_ceiling.sh: the domain table's answer without its row loads (1) or its mask stores (2) - WRONG masks
    k.probe_experiment = (int)num("TXQ_PROBE_EXPERIMENT", 0) & 3;
#endif
    std::lock_guard<std::mutex> lock(g_knobs_mutex);
    g_knobs = k;
}

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
int fail_hip(hipError_t e, const char* what) {
    return fail(e == hipErrorOutOfMemory ? TXQ_ERR_NOMEM : TXQ_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
// The HIP device is a per-thread setting: a thread other than the one that called txq_init (e.g. the host's
// stage-submission threads, one per shard) would otherwise talk to device 0, and the embedding application may
// have selected another device since the last call (torch.cuda.set_device): always ask, never trust a cached answer.
static int bind_device(int device) {
    int current = -1;
    if (hipGetDevice(&current) != hipSuccess || current != device) {
        hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
    }
    return TXQ_OK;
}
int require_init() {
    if (g_devices.empty()) return fail(TXQ_ERR_STATE, "txq_init has not been called (or found no GPU); this library has no CPU fallback");
    return bind_device(g_devices[0]);
}
// calls that work on an index run on the device that holds it
static int bind_index(const Index* ix) {
    if (g_devices.empty()) return fail(TXQ_ERR_STATE, "txq_init has not been called (or found no GPU); this library has no CPU fallback");
    return bind_device(ix ? ix->device : g_devices[0]);
}

static int validate_ibf(const txq_ibf_desc& d, bool need_words) {
    if (d.bins == 0 || d.bin_size == 0) return fail(TXQ_ERR_ARG, "IBF with zero bins or rows");
    if (d.hash_funs < 1 || d.hash_funs > 5) return fail(TXQ_ERR_ARG, "hash_funs %llu outside 1..5", (unsigned long long)d.hash_funs);
    if (d.bin_words != (d.bins + 63) / 64 || d.tech_bins != d.bin_words * 64)
        return fail(TXQ_ERR_ARG, "inconsistent bins/tech_bins/bin_words (%llu/%llu/%llu)", (unsigned long long)d.bins,
                    (unsigned long long)d.tech_bins, (unsigned long long)d.bin_words);
    if (d.hash_shift != (uint64_t)__builtin_clzll(d.bin_size))
        return fail(TXQ_ERR_ARG, "hash_shift %llu != countl_zero(bin_size)", (unsigned long long)d.hash_shift);
    if (d.bin_words >> 31) return fail(TXQ_ERR_ARG, "more than 2^37 bins are not supported");
    if (need_words && !d.words) return fail(TXQ_ERR_ARG, "IBF descriptor without words");
    return TXQ_OK;
}

// Allocate one IBF (column slice [w0, w1) of its rows) in HBM; copies from d.words when given.
int alloc_ibf(Index& ix, const txq_ibf_desc& d, uint64_t w0, uint64_t w1) {
    IbfDev f = ibf_shape(d, w0, w1);
    if (f.shard_words) {
        const size_t nbytes = ibf_bytes(f);
        DeviceBuffer<uint64_t> words;
        if (int rc = reserved(words.reserve(exactly(nbytes), free_now()), "hipMalloc((void**)&f.words, nbytes)")) return rc;
        f.words = words.get();
        hipError_t e = hipSuccess;
        if (f.stride != f.shard_words || !d.words) e = hipMemset(f.words, 0, nbytes);
        if (e == hipSuccess && d.words)
            e = hipMemcpy2D(f.words, (size_t)f.stride * 8, d.words + w0, (size_t)d.bin_words * 8, (size_t)f.shard_words * 8,
                            (size_t)d.bin_size, hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail_hip(e, "uploading IBF words");
        ix.uploaded.push_back(std::move(words));
        ix.device_bytes += nbytes;
    }
    ix.ibf.push_back(f);
    return TXQ_OK;
}

}  // namespace txq

using namespace txq;

struct txq_index : txq::Index {};
struct txq_session : txq::Session {};

extern "C" {

const char* txq_last_error(void) { return g_err.c_str(); }

int txq_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail_hip(e, "hipGetDeviceCount");
    return n;
}

int txq_init(int n_devices, const int* device_ids) {
    read_knobs();
    if (n_devices < 1 || n_devices > 64) return fail(TXQ_ERR_ARG, "n_devices must be 1..64 (got %d)", n_devices);
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_devices.clear();
        return fail(TXQ_ERR_STATE, "no HIP device visible (%s); this library has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    }
    std::vector<int> devices;
    for (int i = 0; i < n_devices; ++i) {
        const int dev = device_ids ? device_ids[i] : i;
        if (dev < 0 || dev >= n) return fail(TXQ_ERR_ARG, "device %d out of range (have %d)", dev, n);
        hipDeviceProp_t prop;
        TXQ_HIP(hipGetDeviceProperties(&prop, dev));
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return fail(TXQ_ERR_STATE, "device %d is %s; this library is built for gfx950 (MI355X) only", dev, prop.gcnArchName);
        devices.push_back(dev);
    }
    for (size_t i = devices.size(); i-- > 0;) {  // load the kernels now, not inside the first query (ends on devices[0])
        TXQ_HIP(hipSetDevice(devices[i]));
        preload_exec_kernels();
        preload_probe_kernels();
        preload_hibf_kernels();
        // A non-blocking stream is a hardware queue of its own: 9 ms to create.  A session needs two; the first session of a
        // process takes them from here instead of paying 18 ms inside its first query (later sessions on an index inherit its streams).
        std::lock_guard<std::mutex> lk(g_spare_mutex);
        while (g_spare_streams[devices[i]].size() < 2) {
            hipStream_t st = nullptr;
            if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); break; }
            g_spare_streams[devices[i]].push_back(st);
        }
    }
    g_devices = devices;
    return TXQ_OK;
}

int txq_shutdown(void) {
    g_devices.clear();
    return TXQ_OK;
}

static int check_desc(const txq_index_desc* desc, int shard_rank, int n_shards, txq_index** out, bool* hibf_out) {
    if (!desc || !out || !desc->ibf || desc->n_ibf == 0) return fail(TXQ_ERR_ARG, "null descriptor");
    if (n_shards < 1 || shard_rank < 0 || shard_rank >= n_shards) return fail(TXQ_ERR_ARG, "bad shard %d/%d", shard_rank, n_shards);
    const bool hibf = desc->next_ibf_id != nullptr || desc->tb_to_user_bin != nullptr || desc->n_ibf > 1;
    if (hibf && (!desc->next_ibf_id || !desc->tb_to_user_bin)) return fail(TXQ_ERR_ARG, "HIBF descriptor needs both maps");
    for (uint64_t i = 0; i < desc->n_ibf; ++i)
        if (int rc = validate_ibf(desc->ibf[i], true)) return rc;
    if (!hibf && desc->user_bins != desc->ibf[0].bins) return fail(TXQ_ERR_ARG, "flat IBF: user_bins must equal ibf[0].bins");
    if (desc->user_bins == 0) return fail(TXQ_ERR_ARG, "user_bins == 0");
    *hibf_out = hibf;
    return TXQ_OK;
}

// the upload itself: the index goes to the device of `device_rank`; it keeps mask columns `range_rank` of `range_shards`
static int upload_impl(const txq_index_desc* desc, bool hibf, int device_rank, int range_rank, int range_shards, txq_index** out, bool cleared_ok = false) {
    const int shard_rank = range_rank, n_shards = range_shards;
    txq_index* ix = new (std::nothrow) txq_index();
    if (!ix) return fail(TXQ_ERR_NOMEM, "out of host memory");
    ix->device = g_devices[(size_t)device_rank % g_devices.size()];  // shards go round-robin over the devices of txq_init
    if (int rc = bind_device(ix->device)) { delete ix; return rc; }
    ix->is_hibf = hibf;
    ix->user_bins = desc->user_bins;
    ix->mask_words = (desc->user_bins + 63) / 64;
    ix->shard_rank = device_rank;
    ix->n_shards = range_shards;
    uint64_t lo, hi;
    shard_range(ix->mask_words, shard_rank, n_shards, &lo, &hi);
    ix->shard_word0 = lo;
    ix->shard_words = hi - lo;
    int rc = TXQ_OK;
    if (!hibf) {
        rc = alloc_ibf(*ix, desc->ibf[0], lo, hi);
    } else {
        rc = hibf_upload(*ix, *desc, cleared_ok);
    }
    if (rc != TXQ_OK) {
        delete ix;
        return rc;
    }
    *out = ix;
    return TXQ_OK;
}

int txq_index_upload(const txq_index_desc* desc, int shard_rank, int n_shards, txq_index** out) {
    read_knobs();
    if (int rc = require_init()) return rc;
    bool hibf = false;
    if (int rc = check_desc(desc, shard_rank, n_shards, out, &hibf)) return rc;
    return upload_impl(desc, hibf, shard_rank, shard_rank, n_shards, out);
}

int txq_index_upload_subtrees(const txq_index_desc* desc, int shard_rank, int n_shards, txq_index** out) {
    read_knobs();
    if (int rc = require_init()) return rc;
    bool hibf = false;
    if (int rc = check_desc(desc, shard_rank, n_shards, out, &hibf)) return rc;
    if (!hibf || n_shards == 1) return upload_impl(desc, hibf, shard_rank, shard_rank, n_shards, out);
    const uint64_t n = desc->n_ibf;
    for (uint64_t i = 0; i < n; ++i)
        if (!desc->next_ibf_id[i] || !desc->tb_to_user_bin[i]) return fail(TXQ_ERR_ARG, "HIBF map %llu is null", (unsigned long long)i);
    if (regular_two_level(*desc)) return upload_impl(desc, hibf, shard_rank, shard_rank, n_shards, out);
    // this shard's tree (txq_hibf_plan.hpp plan_subtree_shard); user bins are checked by the upload of the IBFs the shard keeps
    HibfTree tree;
    if (PlanError e = read_tree(*desc, false, &tree, false)) {
        if (e.kind == PlanError::kBadChild || e.kind == PlanError::kTwoParents)
            return fail(TXQ_ERR_ARG, "HIBF: bad child %llu (out of range or reached twice)", (unsigned long long)e.ibf);
        return fail(e.code, "%s", e.text.c_str());
    }
    const SubtreeShard shard = plan_subtree_shard(tree, *desc, shard_rank, n_shards);
    const std::vector<uint64_t>& kept = shard.kept;
    const txq_ibf_desc& root = desc->ibf[0];
    std::vector<uint64_t> root_words((size_t)root.bin_size * root.bin_words);
    for (uint64_t r = 0; r < root.bin_size; ++r)
        for (uint64_t w = 0; w < root.bin_words; ++w) root_words[r * root.bin_words + w] = root.words[r * root.bin_words + w] & shard.keep_mask[w];
    std::vector<txq_ibf_desc> ibfs;
    std::vector<const uint64_t*> next_p, user_p;
    for (size_t j = 0; j < kept.size(); ++j) {
        txq_ibf_desc d = desc->ibf[kept[j]];
        if (kept[j] == 0) d.words = root_words.data();
        ibfs.push_back(d);
        next_p.push_back(shard.next[j].data());
        user_p.push_back(shard.user[j].data());
    }
    const txq_index_desc pruned{kept.size(), ibfs.data(), next_p.data(), user_p.data(), desc->user_bins};
    if (int rc = upload_impl(&pruned, true, shard_rank, 0, 1, out, true)) return rc;
    (*out)->join_or = true;
    (*out)->n_shards = n_shards;
    return TXQ_OK;
}

int txq_index_create_ibf(uint64_t bins, uint64_t bin_size, uint64_t hash_funs, int shard_rank, int n_shards, txq_index** out) {
    if (int rc = require_init()) return rc;
    if (!out || n_shards < 1 || shard_rank < 0 || shard_rank >= n_shards) return fail(TXQ_ERR_ARG, "bad arguments");
    txq_ibf_desc d{};
    d.bins = bins;
    d.bin_words = (bins + 63) / 64;
    d.tech_bins = d.bin_words * 64;
    d.bin_size = bin_size;
    d.hash_shift = bin_size ? (uint64_t)__builtin_clzll(bin_size) : 0;
    d.hash_funs = hash_funs;
    d.words = nullptr;
    if (int rc = validate_ibf(d, false)) return rc;
    txq_index* ix = new (std::nothrow) txq_index();
    if (!ix) return fail(TXQ_ERR_NOMEM, "out of host memory");
    ix->device = g_devices[(size_t)shard_rank % g_devices.size()];
    if (int rc = bind_device(ix->device)) { delete ix; return rc; }
    ix->user_bins = bins;
    ix->mask_words = d.bin_words;
    ix->shard_rank = shard_rank;
    ix->n_shards = n_shards;
    uint64_t lo, hi;
    shard_range(ix->mask_words, shard_rank, n_shards, &lo, &hi);
    ix->shard_word0 = lo;
    ix->shard_words = hi - lo;
    if (int rc = alloc_ibf(*ix, d, lo, hi)) { delete ix; return rc; }
    *out = ix;
    return TXQ_OK;
}

int txq_index_get_info(const txq_index* ix, txq_index_info* info) {
    if (!ix || !info) return fail(TXQ_ERR_ARG, "null argument");
    info->user_bins = ix->user_bins;
    info->mask_words = ix->mask_words;
    info->shard_word0 = ix->shard_word0;
    info->shard_words = ix->shard_words;
    info->n_ibf = ix->ibf.size();
    info->device_bytes = ix->device_bytes;
    info->is_hibf = ix->is_hibf ? 1 : 0;
    info->device = ix->device;
    info->join_or = ix->join_or ? 1 : 0;
    info->shard_rank = ix->shard_rank;
    info->n_shards = ix->n_shards;
    info->reserved = 0;
    return TXQ_OK;
}

int txq_index_supports_dense(const txq_index* ix) {
    read_knobs();
    if (!ix || ix->ibf.empty() || ix->shard_words == 0) return 0;
    if (!ix->is_hibf) return (ix->ibf[0].bin_size >> 32) == 0 ? 2 : 0;
    return index_fuses_tree_steps(*ix, knobs()) || ix->layout_order(knobs()) ? 2 : 1;  // other HIBFs: steps run as k-mer batches through the descent
}

int txq_index_free(txq_index* ix) {
    if (!ix) return TXQ_OK;
    if (ix->open_sessions > 0)
        return fail(TXQ_ERR_STATE, "the index still has %d open session(s): end them first (txq_session_end)", ix->open_sessions);
    if (!g_devices.empty()) (void)bind_device(ix->device);
    delete ix;
    return TXQ_OK;
}

int txq_index_memory(const txq_index* ix, uint64_t* free_bytes, uint64_t* kept_bytes) {
    if (!ix || !free_bytes || !kept_bytes) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = bind_index(ix)) return rc;
    size_t free_b = 0, total_b = 0;
    TXQ_HIP(hipMemGetInfo(&free_b, &total_b));
    uint64_t kept = 0;
    for (const ArenaChunk& c : ix->session_cache.chunks) kept += (uint64_t)c.cap * 8;
    for (const ArenaChunk& c : ix->session_cache.block_chunks) kept += (uint64_t)c.cap * 8;
    *free_bytes = free_b;
    *kept_bytes = kept;
    return TXQ_OK;
}

int txq_index_set_tag(txq_index* ix, uint64_t tag) {
    if (!ix) return fail(TXQ_ERR_ARG, "null argument");
    ix->user_tag = tag;
    return TXQ_OK;
}
int txq_index_get_tag(const txq_index* ix, uint64_t* tag) {
    if (!ix || !tag) return fail(TXQ_ERR_ARG, "null argument");
    *tag = ix->user_tag;
    return TXQ_OK;
}

int txq_index_download_words(const txq_index* ix, uint64_t* words, size_t n_words) {
    if (!ix) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = bind_index(ix)) return rc;
    if (!ix || !words) return fail(TXQ_ERR_ARG, "null argument");
    if (ix->is_hibf) return fail(TXQ_ERR_ARG, "download_words is for flat IBFs");
    const IbfDev& f = ix->ibf[0];
    if (n_words != (size_t)f.bin_size * f.shard_words) return fail(TXQ_ERR_ARG, "expected %zu words", (size_t)f.bin_size * f.shard_words);
    if (!f.shard_words) return TXQ_OK;
    TXQ_HIP(hipMemcpy2D(words, (size_t)f.shard_words * 8, f.words, (size_t)f.stride * 8, (size_t)f.shard_words * 8,
                        (size_t)f.bin_size, hipMemcpyDeviceToHost));
    return TXQ_OK;
}

int txq_probe_device(txq_index* ix, const uint64_t* d_kmers, size_t n, uint64_t* d_masks, uint64_t* d_alive, void* stream) {
    read_knobs();
    if (!ix) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = bind_index(ix)) return rc;
    if (!ix || (n && (!d_kmers || !d_masks))) return fail(TXQ_ERR_ARG, "null argument");
    if (n >> 32) return fail(TXQ_ERR_ARG, "at most 2^32-1 k-mers per call");
    hipStream_t s = (hipStream_t)stream;
    if (ix->is_hibf) return hibf_probe(*ix, knobs(), d_kmers, n, d_masks, d_alive, s);
    hipError_t e = probe_flat(*ix, knobs(), d_kmers, n, d_masks, d_alive, s);
    if (e != hipSuccess) return fail_hip(e, "probe kernel launch");
    return TXQ_OK;
}

// What the flat probe's sorted answer did so far (tests tell its paths apart by it); waits for the index's last table call.
int txq_index_probe_sorted(txq_index* ix, uint64_t out[2]) {
    if (!ix || !out) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = bind_index(ix)) return rc;
    Index::ProbeTable& pt = ix->probe_table;
    std::lock_guard<std::mutex> lock(pt.mutex);
    out[0] = pt.sort_planned;
    out[1] = 0;
    if (pt.recorded && pt.state) {
        uint32_t ran = 0;
        TXQ_HIP(hipEventSynchronize(pt.done.get()));
        TXQ_HIP(hipMemcpy(&ran, pt.state.get() + kStateSorted, sizeof ran, hipMemcpyDeviceToHost));
        out[1] = ran;
    }
    return TXQ_OK;
}

// Host-buffer probe: chunks are pipelined over two streams — while chunk c's masks travel back
// (device -> pinned bounce buffer -> caller's memory, or straight into the caller's memory when
// that is pinned, e.g. from txq_host_alloc), chunk c+1 is probed.
int txq_probe(txq_index* ix, const uint64_t* kmers, size_t n, uint64_t* masks) {
    if (!ix) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = bind_index(ix)) return rc;
    if (!ix || (n && (!kmers || !masks))) return fail(TXQ_ERR_ARG, "null argument");
    const size_t W = ix->shard_words;
    if (W == 0 || n == 0) return TXQ_OK;
    // chunk: about 32 MiB of masks, at most 2^20 k-mers
    size_t chunk = ((size_t)32 << 20) / (W * 8);
    if (chunk > ((size_t)1 << 20)) chunk = (size_t)1 << 20;
    if (chunk < 1024) chunk = 1024;
    if (chunk > n) chunk = n;
    Index::HostPipe& hp = ix->host_pipe;
    for (int i = 0; i < 2; ++i) {
        TXQ_HIP(make(hp.stream[i]));
        TXQ_HIP(make(hp.done[i]));
        if (int rc = reserved(hp.d_kmers[i].reserve(exactly(chunk * 8), after_device_wait()), "hipMalloc(scratch)")) return rc;
        if (int rc = reserved(hp.d_masks[i].reserve(exactly(chunk * W * 8), after_device_wait()), "hipMalloc(scratch)")) return rc;
    }
    hipPointerAttribute_t attr{};
    const bool pinned_out = hipPointerGetAttributes(&attr, masks) == hipSuccess && attr.type == hipMemoryTypeHost;
    (void)hipGetLastError();  // an unregistered pointer is reported as an error: not one of ours
    if (!pinned_out) {
        for (int i = 0; i < 2; ++i)  // (every chunk of an earlier call was drained before that call returned)
            if (int rc = reserved(hp.bounce[i].reserve(exactly(chunk * W * 8), free_now()), "hipHostMalloc(bounce buffer)")) return rc;
    }
    size_t pending_off[2] = {0, 0}, pending_m[2] = {0, 0};
    auto drain = [&](int b) -> int {  // wait for buffer b's chunk and hand it to the caller
        if (!pending_m[b]) return TXQ_OK;
        TXQ_HIP(hipEventSynchronize(hp.done[b].get()));
        if (!pinned_out) std::memcpy(masks + pending_off[b] * W, hp.bounce[b].get(), pending_m[b] * W * 8);
        pending_m[b] = 0;
        return TXQ_OK;
    };
    int b = 0;
    for (size_t off = 0; off < n; off += chunk, b ^= 1) {
        const size_t m = n - off < chunk ? n - off : chunk;
        if (int rc = drain(b)) return rc;  // this buffer's previous chunk
        // the HIBF descent has per-index scratch (frontiers): its chunks share one stream
        hipStream_t st = hp.stream[ix->is_hibf ? 0 : b].get();
        TXQ_HIP(hipMemcpyAsync(hp.d_kmers[b].get(), kmers + off, m * 8, hipMemcpyHostToDevice, st));
        if (int rc = txq_probe_device(ix, hp.d_kmers[b].get(), m, hp.d_masks[b].get(), nullptr, st)) return rc;
        TXQ_HIP(hipMemcpyAsync(pinned_out ? (void*)(masks + off * W) : (void*)hp.bounce[b].get(), hp.d_masks[b].get(), m * W * 8, hipMemcpyDeviceToHost, st));
        TXQ_HIP(hipEventRecord(hp.done[b].get(), st));
        pending_off[b] = off;
        pending_m[b] = m;
    }
    if (int rc = drain(b)) return rc;
    if (int rc = drain(b ^ 1)) return rc;
    return TXQ_OK;
}

int txq_count_device(txq_index* ix, const uint64_t* d_values, const uint64_t* d_offsets, size_t n_queries, const uint32_t* d_thresholds,
                     uint64_t* d_hits, uint32_t* d_counts, void* stream) {
    if (!ix) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = bind_index(ix)) return rc;
    if (n_queries && (!d_values || !d_offsets || !d_thresholds || !d_hits)) return fail(TXQ_ERR_ARG, "null argument");
    if (ix->join_or) return fail(TXQ_ERR_ARG, "txq_count does not support sub-tree shards (txq_index_upload_subtrees)");
    if (n_queries >= 0xFFFFFFFFull) return fail(TXQ_ERR_ARG, "at most 2^32-2 queries per call");
    return count_device(*ix, d_values, d_offsets, n_queries, d_thresholds, d_hits, d_counts, (hipStream_t)stream);
}

// Host buffers: the offsets are checked here, then the call's values, offsets (rebased to 0), thresholds and results go through
// one device buffer of the index, on the index's first host-pipe stream.
int txq_count(txq_index* ix, const uint64_t* values, const uint64_t* offsets, size_t n_queries, const uint32_t* thresholds, uint64_t* hits,
              uint32_t* counts) {
    if (!ix) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = bind_index(ix)) return rc;
    if (!offsets || (n_queries && (!thresholds || !hits))) return fail(TXQ_ERR_ARG, "null argument");
    if (ix->join_or) return fail(TXQ_ERR_ARG, "txq_count does not support sub-tree shards (txq_index_upload_subtrees)");
    if (n_queries >= 0xFFFFFFFFull) return fail(TXQ_ERR_ARG, "at most 2^32-2 queries per call");
    for (size_t q = 0; q < n_queries; ++q)
        if (offsets[q + 1] < offsets[q]) return fail(TXQ_ERR_ARG, "offsets are not ascending at query %zu", q);
    const uint64_t n_values = n_queries ? offsets[n_queries] - offsets[0] : 0;
    if (n_values >> 32) return fail(TXQ_ERR_ARG, "%llu values: at most 2^32-1 per call", (unsigned long long)n_values);
    if (n_values && !values) return fail(TXQ_ERR_ARG, "null argument");
    const size_t W = ix->shard_words;
    if (n_queries == 0 || W == 0) return TXQ_OK;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_val = up(n_values * 8), b_off = up((n_queries + 1) * 8), b_thr = up(n_queries * 4), b_hit = up(n_queries * W * 8);
    const size_t b_cnt = counts ? up(n_queries * W * 64 * 4) : 0;
    if (int rc = reserved(ix->scratch_count_io.reserve(exactly(b_val + b_off + b_thr + b_hit + b_cnt), after_device_wait()), "hipMalloc(scratch)")) return rc;
    unsigned char* base = ix->scratch_count_io.get();
    uint64_t* d_val = (uint64_t*)base;
    uint64_t* d_off = (uint64_t*)(base + b_val);
    uint32_t* d_thr = (uint32_t*)(base + b_val + b_off);
    uint64_t* d_hit = (uint64_t*)(base + b_val + b_off + b_thr);
    uint32_t* d_cnt = counts ? (uint32_t*)(base + b_val + b_off + b_thr + b_hit) : nullptr;
    std::vector<uint64_t> rebased(offsets, offsets + n_queries + 1);
    for (uint64_t& o : rebased) o -= offsets[0];
    Index::HostPipe& hp = ix->host_pipe;
    TXQ_HIP(make(hp.stream[0]));
    hipStream_t st = hp.stream[0].get();
    if (n_values) TXQ_HIP(hipMemcpyAsync(d_val, values + offsets[0], n_values * 8, hipMemcpyHostToDevice, st));
    TXQ_HIP(hipMemcpyAsync(d_off, rebased.data(), rebased.size() * 8, hipMemcpyHostToDevice, st));
    TXQ_HIP(hipMemcpyAsync(d_thr, thresholds, n_queries * 4, hipMemcpyHostToDevice, st));
    if (int rc = count_device(*ix, d_val, d_off, n_queries, d_thr, d_hit, d_cnt, st)) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    TXQ_HIP(hipMemcpyAsync(hits, d_hit, n_queries * W * 8, hipMemcpyDeviceToHost, st));
    if (counts) TXQ_HIP(hipMemcpyAsync(counts, d_cnt, n_queries * W * 64 * 4, hipMemcpyDeviceToHost, st));
    TXQ_HIP(hipStreamSynchronize(st));
    return TXQ_OK;
}

int txq_count_windows_device(txq_index* ix, const uint64_t* d_values, const uint64_t* d_win_begin, const uint32_t* d_win_len, size_t n_windows,
                             const uint32_t* d_thresholds, uint64_t* d_hits, uint32_t* d_counts, void* stream) {
    if (!ix) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = bind_index(ix)) return rc;
    if (n_windows && (!d_values || !d_win_begin || !d_win_len || !d_thresholds || !d_hits)) return fail(TXQ_ERR_ARG, "null argument");
    if (ix->join_or) return fail(TXQ_ERR_ARG, "txq_count_windows does not support sub-tree shards (txq_index_upload_subtrees)");
    if (n_windows >= 0xFFFFFFFFull) return fail(TXQ_ERR_ARG, "at most 2^32-2 windows per call");
    return count_windows_device(*ix, d_values, d_win_begin, d_win_len, n_windows, d_thresholds, d_hits, d_counts, (hipStream_t)stream);
}

// Host buffers: the windows are checked here, then the values they span, the windows (rebased to the first one's begin),
// thresholds and results go through the device buffer of txq_count, on the index's first host-pipe stream.
int txq_count_windows(txq_index* ix, const uint64_t* values, size_t n_values, const uint64_t* win_begin, const uint32_t* win_len, size_t n_windows,
                      const uint32_t* thresholds, uint64_t* hits, uint32_t* counts) {
    if (!ix) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = bind_index(ix)) return rc;
    if (n_windows && (!win_begin || !win_len || !thresholds || !hits)) return fail(TXQ_ERR_ARG, "null argument");
    if (ix->join_or) return fail(TXQ_ERR_ARG, "txq_count_windows does not support sub-tree shards (txq_index_upload_subtrees)");
    if (n_windows >= 0xFFFFFFFFull) return fail(TXQ_ERR_ARG, "at most 2^32-2 windows per call");
    for (size_t j = 0; j < n_windows; ++j) {
        if (win_begin[j] > n_values || win_len[j] > n_values - win_begin[j])
            return fail(TXQ_ERR_ARG, "window %zu runs past the %zu values", j, n_values);
        if (j && win_begin[j] < win_begin[j - 1]) return fail(TXQ_ERR_ARG, "window begins are not ascending at window %zu", j);
        if (j && win_begin[j] + win_len[j] < win_begin[j - 1] + win_len[j - 1]) return fail(TXQ_ERR_ARG, "window ends are not ascending at window %zu", j);
    }
    const size_t W = ix->shard_words;
    if (n_windows == 0 || W == 0) {
        ix->count_windows_trace.recorded = false;  // (txq_count_windows_trace: nothing of the call before)
        return TXQ_OK;
    }
    const uint64_t v0 = win_begin[0], span = win_begin[n_windows - 1] + win_len[n_windows - 1] - v0;
    if (span >> 32) return fail(TXQ_ERR_ARG, "%llu values: at most 2^32-1 per call", (unsigned long long)span);
    if (span && !values) return fail(TXQ_ERR_ARG, "null argument");
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_val = up(span * 8), b_beg = up(n_windows * 8), b_len = up(n_windows * 4), b_thr = up(n_windows * 4), b_hit = up(n_windows * W * 8);
    const size_t b_cnt = counts ? up(n_windows * W * 64 * 4) : 0;
    if (int rc = reserved(ix->scratch_count_io.reserve(exactly(b_val + b_beg + b_len + b_thr + b_hit + b_cnt), after_device_wait()), "hipMalloc(scratch)")) return rc;
    unsigned char* base = ix->scratch_count_io.get();
    uint64_t* d_val = (uint64_t*)base;
    uint64_t* d_beg = (uint64_t*)(base + b_val);
    uint32_t* d_len = (uint32_t*)(base + b_val + b_beg);
    uint32_t* d_thr = (uint32_t*)(base + b_val + b_beg + b_len);
    uint64_t* d_hit = (uint64_t*)(base + b_val + b_beg + b_len + b_thr);
    uint32_t* d_cnt = counts ? (uint32_t*)(base + b_val + b_beg + b_len + b_thr + b_hit) : nullptr;
    std::vector<uint64_t> begins(win_begin, win_begin + n_windows);
    for (uint64_t& b : begins) b -= v0;
    Index::HostPipe& hp = ix->host_pipe;
    TXQ_HIP(make(hp.stream[0]));
    hipStream_t st = hp.stream[0].get();
    if (span) TXQ_HIP(hipMemcpyAsync(d_val, values + v0, span * 8, hipMemcpyHostToDevice, st));
    TXQ_HIP(hipMemcpyAsync(d_beg, begins.data(), n_windows * 8, hipMemcpyHostToDevice, st));
    TXQ_HIP(hipMemcpyAsync(d_len, win_len, n_windows * 4, hipMemcpyHostToDevice, st));
    TXQ_HIP(hipMemcpyAsync(d_thr, thresholds, n_windows * 4, hipMemcpyHostToDevice, st));
    if (int rc = count_windows_device(*ix, d_val, d_beg, d_len, n_windows, d_thr, d_hit, d_cnt, st)) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    TXQ_HIP(hipMemcpyAsync(hits, d_hit, n_windows * W * 8, hipMemcpyDeviceToHost, st));
    if (counts) TXQ_HIP(hipMemcpyAsync(counts, d_cnt, n_windows * W * 64 * 4, hipMemcpyDeviceToHost, st));
    TXQ_HIP(hipStreamSynchronize(st));
    return TXQ_OK;
}

// What the index's last txq_count_windows* call on an HIBF did (tests and measurements tell its routes apart by it); waits for that call.
int txq_count_windows_trace(txq_index* ix, uint64_t out[4]) {
    if (!ix || !out) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = bind_index(ix)) return rc;
    Index::CountWindowsTrace& tr = ix->count_windows_trace;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (tr.recorded && tr.totals) {
        unsigned long long totals[kCwTraceSlots * kCwTraceWords];  // (the waves add to kCwTraceSlots sets of totals)
        TXQ_HIP(hipEventSynchronize(tr.done.get()));
        TXQ_HIP(hipMemcpy(totals, tr.totals.get(), sizeof totals, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < kCwTraceSlots * kCwTraceWords; ++i) out[i % kCwTraceWords] += totals[i];
    }
    return TXQ_OK;
}

int txq_host_alloc(void** ptr, size_t bytes) {
    if (int rc = require_init()) return rc;
    if (!ptr) return fail(TXQ_ERR_ARG, "null argument");
    TXQ_HIP(hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault));
    return TXQ_OK;
}

int txq_host_free(void* ptr) {
    if (!ptr) return TXQ_OK;
    TXQ_HIP(hipHostFree(ptr));
    return TXQ_OK;
}

int txq_emplace_device(txq_index* ix, const uint64_t* d_values, const uint32_t* d_bins_of, size_t n, void* stream) {
    if (!ix) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = bind_index(ix)) return rc;
    if (!ix || (n && (!d_values || !d_bins_of))) return fail(TXQ_ERR_ARG, "null argument");
    if (ix->is_hibf) return fail(TXQ_ERR_ARG, "emplace is for flat IBFs");
    if (ix->open_sessions > 0)
        return fail(TXQ_ERR_STATE, "the index has %d open session(s): its bits cannot change under them (txq_session_end first)", ix->open_sessions);
    {   // what was derived from the old bits goes: the table of all k-mers' masks (dense steps would read stale rows), the host's
        // verdict on how states fare on the index (tag) stays — it is advisory
        std::lock_guard<std::mutex> lock(ix->table_mutex);
        if (ix->kmer_table) {
            TXQ_HIP(hipDeviceSynchronize());  // (kernels of ended sessions may still be reading it)
            ix->kmer_table.reset();
            ix->kmer_table_bits = 0;
        }
        ix->kmer_table_refused = false;
    }
    // ... and the flat probe's domain table: the next probe call finds another generation and starts its rows over.  A probe
    // enqueued earlier, on whatever stream, has left rows of the old bits behind; the kernel below waits for it, so that none of
    // them is written after the bits changed (no device-wide wait: the event of the last table call is enough).
    Index::ProbeTable& pt = ix->probe_table;
    std::lock_guard<std::mutex> lock(pt.mutex);
    ++ix->generation;
    if (pt.recorded) TXQ_HIP(hipStreamWaitEvent((hipStream_t)stream, pt.done.get(), 0));
    hipError_t e = launch_emplace(ix->ibf[0], d_values, d_bins_of, n, (hipStream_t)stream);
    if (e != hipSuccess) return fail_hip(e, "emplace kernel launch");
    return TXQ_OK;
}

int txq_run_programs_device(txq_index* ix, const void* blob, size_t blob_bytes, size_t n_programs, uint64_t* d_final_masks, void* stream) {
    read_knobs();
    if (!ix) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = bind_index(ix)) return rc;
    if (!ix || !blob || (n_programs && !d_final_masks)) return fail(TXQ_ERR_ARG, "null argument");
    return run_programs(*ix, blob, blob_bytes, n_programs, d_final_masks, false, (hipStream_t)stream);
}

int txq_run_programs(txq_index* ix, const void* blob, size_t blob_bytes, size_t n_programs, uint64_t* final_masks) {
    read_knobs();
    if (!ix) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = bind_index(ix)) return rc;
    if (!ix || !blob || (n_programs && !final_masks)) return fail(TXQ_ERR_ARG, "null argument");
    if (n_programs * ix->shard_words == 0) return TXQ_OK;
    return run_programs(*ix, blob, blob_bytes, n_programs, final_masks, true, nullptr);
}

int txq_session_begin(txq_index* ix, size_t n_programs, txq_session** out) {
    read_knobs();
    if (!ix) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = bind_index(ix)) return rc;
    if (!ix || !out) return fail(TXQ_ERR_ARG, "null argument");
    Session* s = nullptr;
    if (int rc = session_begin(*ix, n_programs, &s)) return rc;
    *out = static_cast<txq_session*>(s);
    return TXQ_OK;
}

int txq_session_set_aux_index(txq_session* s, txq_index* aux) {
    if (!s) return fail(TXQ_ERR_ARG, "null argument");
    if (aux) {
        if (aux->is_hibf) return fail(TXQ_ERR_ARG, "the auxiliary index must be a flat IBF");
        if (aux->user_bins != s->ix->user_bins || aux->shard_word0 != s->ix->shard_word0 || aux->shard_words != s->ix->shard_words ||
            aux->device != s->ix->device)
            return fail(TXQ_ERR_ARG, "the auxiliary index must cover the same bins and the same shard (on the same device) as the main index");
    }
    if (aux && s->vspace) {  // d-gram masks come in user-bin order: the session cannot work in layout order then
        if (s->n_stages) return fail(TXQ_ERR_STATE, "attach the auxiliary index before the session's first stage");
        s->vspace = false;
        s->W = (uint32_t)s->ix->shard_words;
    }
    if (s->aux) --s->aux->open_sessions;
    s->aux = aux;
    if (aux) ++aux->open_sessions;
    return TXQ_OK;
}

int txq_session_stage(txq_session* s, const void* blob, size_t blob_bytes, const uint32_t* query_program,
                      const uint32_t* query_slot, size_t n_queries, uint8_t* alive) {
    if (!s) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = bind_index(s->ix)) return rc;
    if ( !blob || (n_queries && (!query_program || !query_slot || !alive))) return fail(TXQ_ERR_ARG, "null argument");
    if (s->failed) return fail(TXQ_ERR_STATE, "an earlier stage of this session failed: end the session");
    const int rc = session_stage(*s, blob, blob_bytes, query_program, query_slot, n_queries, alive, nullptr);
    if (rc != TXQ_OK) {
        // Kernels of the stage may already be running (on either stream) and the stage's bookkeeping is half done: nothing of
        // this session may be in flight when its buffers change hands, and no further stage may build on it
        const std::string why = g_err;
        (void)hipDeviceSynchronize();
        s->failed = true;
        g_err = why;
    }
    return rc;
}

int txq_session_end(txq_session* s, uint64_t* final_masks) {
    if (!s) return TXQ_OK;
    int rc = bind_index(s->ix);  // the calling thread may never have selected the device
    if (rc != TXQ_OK) { delete static_cast<Session*>(s); return rc; }
    const bool trace = s->kn.trace;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    double t_finish = t0, t_copy = t0;
    if (final_masks && s->failed) {
        // a stage of this session failed: its slots hold half-executed state, there are no final masks to hand out
        rc = fail(TXQ_ERR_STATE, "a stage of this session failed: it has no final masks");
    } else if (final_masks && s->n_programs && s->W) {
        // (layout-order rows are first put back in user-bin order, with atomics: on the device)
        const size_t bytes = s->n_programs * (size_t)s->ix->shard_words * 8;  // (a layout-order session hands out user-bin masks too)
        rc = session_finish_host(*s, final_masks, s->kn.final_pinned && !s->vspace && bytes <= ((size_t)64 << 20), &t_finish);
        t_copy = now();
    }
    (void)hipDeviceSynchronize();
    const double t_sync = now();
    delete static_cast<Session*>(s);
    if (trace)
        fprintf(stderr, "[txq] session end: last launches %.2f ms, masks to the host %.2f ms, device idle after %.2f ms, session released in %.2f ms\n",
                (t_finish - t0) * 1e3, (t_copy - t_finish) * 1e3, (t_sync - t_copy) * 1e3, (now() - t_sync) * 1e3);
    return rc;
}

int txq_malloc(void** dptr, size_t bytes) {
    if (int rc = require_init()) return rc;
    if (!dptr) return fail(TXQ_ERR_ARG, "null argument");
    TXQ_HIP(hipMalloc(dptr, bytes ? bytes : 8));
    return TXQ_OK;
}
int txq_free(void* dptr) {
    if (dptr) TXQ_HIP(hipFree(dptr));
    return TXQ_OK;
}
int txq_memcpy_h2d(void* dst, const void* src, size_t bytes) {
    if (int rc = require_init()) return rc;
    TXQ_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return TXQ_OK;
}
int txq_memcpy_d2h(void* dst, const void* src, size_t bytes) {
    if (int rc = require_init()) return rc;
    TXQ_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return TXQ_OK;
}
int txq_synchronize(void) {
    if (int rc = require_init()) return rc;
    TXQ_HIP(hipDeviceSynchronize());
    return TXQ_OK;
}

}  // extern "C"
