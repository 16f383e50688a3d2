// Internal (non-ABI) declarations shared by the translation units of libtxq.so.
#pragma once
#include "txq_kernels.hpp"
#include "txq_records.hpp"
#include "txq_exec_plan.hpp"
#include "txq_probe_plan.hpp"
#include "txq_buffers.hpp"
#include "../../include/txq.h"
#include <cstdlib>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

// a HIP call whose failure ends the calling function with TXQ_ERR_HIP (functions that return a TXQ_* code)
#define TXQ_HIP(call)                                        \
    do {                                                     \
        hipError_t e_ = (call);                              \
        if (e_ != hipSuccess) return fail_hip(e_, #call);    \
    } while (0)

namespace txq {

// A run-time value as a compile-time constant: f(std::integral_constant<int, V>{}) for the V of the list that equals v.
// Returns false, with f not called, when v is none of them.  Kernel templates are instantiated for exactly the listed values
// (fewer where f itself leaves combinations out with `if constexpr`).
template <int... Vs, class F>
inline bool with_value(int v, F&& f) {
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}
// the number of hash functions of an IBF: 1 .. 5; false: outside that range
template <class F>
inline bool with_hash_funs(uint32_t h, F&& f) {
    return h <= 5 && with_value<1, 2, 3, 4, 5>((int)h, f);
}
template <class F>
inline void with_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// Every environment variable libtxq.so reads (all of them A/B and test switches between code paths that give the
// SAME results; listed in include/txq.h).  They are parsed in ONE place (txq_api.hip read_knobs) at the library's entry
// points — txq_init, txq_index_upload, txq_session_begin and the probe calls — and everything below works from
// that snapshot: nothing in the library reads the environment while it runs a stage.
struct Knobs {
    bool trace = false, trace_stages = false, trace_sync = false;  // TXQ_TRACE, TXQ_TRACE_STAGES, TXQ_TRACE_SYNC
    // executor (txq_exec.hip)
    int dense_tree = -1;        // TXQ_DENSE_TREE: 0 generic HIBF steps, 1 TreeRows, 2 TreeRowsByLane where it applies; -1: best fit
    int dense_unroll = 3;       // TXQ_DENSE_UNROLL: predecessors in flight per lane (2, 3, 5)
    int dense_slices = 2;       // TXQ_DENSE_SLICES: lane groups sharing the predecessors of one suffix
    int dense_tile_rounds = 4;  // TXQ_DENSE_TILE_ROUNDS: destination suffixes per lane-group set and tile (profiles/r3_dense_tile_shapes_ab.txt)
    int dense_nt = 0;           // TXQ_DENSE_NT: bit 0 non-temporal stores, bit 1 non-temporal loads of a dense step's destination entries
    bool fuse_units = true;     // TXQ_FUSE_UNITS=0: a level's ordinary ops get a launch of their own
    bool one_stream = false;    // TXQ_ONE_STREAM: independent stages do not run beside each other
    int sparse_units = 512;     // TXQ_SPARSE_UNITS: (entry x residue) units per chunk of sparse_units_kernel, 64 .. 1536
    int sparse_unroll = 3;      // TXQ_SPARSE_UNROLL: units in flight per lane group in sparse_units_kernel (2 or 3)
    bool sparse_steps = true;   // TXQ_SPARSE_STEPS=0: pushed steps on narrow masks run in sparse_kernel (rounds of one entry per lane group), not by units (sparse_units_kernel)
    long long kmer_table_mb = 512;  // TXQ_KMER_TABLE_MB: most an index's table of ALL k-mers' masks may take (0: dense steps always gather rows)
    long long kmer_table_min = 16;  // TXQ_KMER_TABLE_MIN: the session of fewest programs that builds the table (a single query does not pay for it; once built it is used)
    // HIBF (txq_hibf.hip)
    bool hibf_interleave = true;        // TXQ_HIBF_INTERLEAVE=0: no interleaved copy of uniform children (at upload)
    bool hibf_interleave_probe = true;  // TXQ_HIBF_INTERLEAVE_PROBE=0: plain probes descend the tree
    bool hibf_levels = false;           // TXQ_HIBF_LEVELS=1: level-synchronous descent
    bool hibf_stationary = true;        // TXQ_HIBF_STATIONARY=0: no child-stationary descent
    bool hibf_small = true;             // TXQ_HIBF_SMALL=0: no lane-per-k-mer kernel for small trees
    bool hibf_lane_hash = false;        // TXQ_HIBF_LANE_HASH: per-lane hashing on a uniform tree
    bool final_pinned = true;           // TXQ_FINAL_PINNED=0: a session's final masks through a device buffer and hipMemcpy
    bool hibf_layout_fused = true;      // TXQ_HIBF_LAYOUT_FUSED=0: the layout-order rows of plain k-mers level by level (hibf_layout_level_kernel), not one wave per k-mer
    bool hibf_layout_order = true;      // TXQ_HIBF_LAYOUT_ORDER=0: sessions on general trees work in user-bin order (descent kernels)
    int hibf_steps_per_group = 0, hibf_tile = 0, hibf_unroll = 1, hibf_store = 0;  // TXQ_HIBF_STEPS_PER_GROUP / _TILE / _UNROLL / _STORE_KIND (store instruction: 0-3)
    long long hibf_waves = 0;           // TXQ_HIBF_WAVES
    bool hibf_layout_direct = true;     // TXQ_HIBF_LAYOUT_DIRECT=0: hibf_fused_kernel<G, LAYOUT> keeps the row in LDS instead of writing it directly
    long long hibf_stack_lds = 128;     // TXQ_HIBF_STACK_LDS: entries of hibf_fused_kernel's IBF stack kept in LDS (the rest: in the k-mer's output row)
    // probe (txq_probe.hip)
    int probe_blocks_per_cu = 256, probe_unroll = 2;  // TXQ_PROBE_BLOCKS_PER_CU, TXQ_PROBE_UNROLL
    bool probe_nt = false;                            // TXQ_PROBE_NT
    int probe_table = -1;  // TXQ_PROBE_TABLE: 0 never the domain table of a flat probe, 1 whenever it fits (tests), unset: where it pays
    bool probe_table_keep = true;  // TXQ_PROBE_TABLE_KEEP=0: the domain table is built from row 0 on every call (A/B and tests)
    bool probe_table_fused = true;  // TXQ_PROBE_TABLE_FUSED=0: a call on kept rows runs sample, build and answer, not the one launch that does all three (A/B and tests)
    bool probe_table_tile = true;   // TXQ_PROBE_TABLE_TILE=0: no table-only tile body, every tile of an answer takes probe_tile (A/B and tests)
    bool probe_sort = true;         // TXQ_PROBE_SORT=0: a large kept call is never answered from a value-bucketed batch (txq_probe_plan.hpp plan_probe_sort)
    long long probe_sort_min = kSortMinDefault;             // TXQ_PROBE_SORT_MIN: the smallest batch that is bucketed
    long long probe_sort_bucket_kb = kSortBucketKbDefault;  // TXQ_PROBE_SORT_BUCKET_KB: table rows per bucket, in KiB
    int probe_experiment = 0;       // TXQ_PROBE_EXPERIMENT, TXQ_EXPERIMENTS builds only: bit 0 the answer loads no rows, bit 1 it stores no masks (timing, wrong masks)
};
Knobs knobs();      // a copy of the snapshot taken at the last entry point (published under a lock: entry points run on several threads)
void read_knobs();  // take it (txq_api.hip)

// The owners of txq_buffers.hpp on HIP's primitives.  Every allocation libtxq keeps has exactly one of them as its owner, and
// changes hands by move only; an outgrown buffer is freed by one of four rules, named where it grows: after_device_wait(),
// after an event the caller names (free_after), retire_to(list), or free_now() where the caller has already waited.
struct DeviceMem {
    static int alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
    static void free(void* p) { (void)hipFree(p); }
};
struct PinnedMem {
    static int alloc(void** p, size_t bytes) { return (int)hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void free(void* p) { (void)hipHostFree(p); }
};
struct EventKind { static void destroy(hipEvent_t e) { (void)hipEventDestroy(e); } };
struct StreamKind { static void destroy(hipStream_t s) { (void)hipStreamDestroy(s); } };
template <class T> using DeviceBuffer = Buffer<T, DeviceMem>;
template <class T> using PinnedBuffer = Buffer<T, PinnedMem>;
using Event = Handle<hipEvent_t, EventKind>;    // made by make(): no timing
using Stream = Handle<hipStream_t, StreamKind>;  // made by make(): non-blocking
// kernels in flight, on whatever stream, may still use the outgrown buffer
inline auto after_device_wait() {
    return free_after([] { (void)hipDeviceSynchronize(); });
}
// the event or stream if there is none yet
inline hipError_t make(Event& e) {
    hipEvent_t h = nullptr;
    const hipError_t rc = e ? hipSuccess : hipEventCreateWithFlags(&h, hipEventDisableTiming);
    if (h) e.reset(h);
    return rc;
}
inline hipError_t make(Stream& s) {
    hipStream_t h = nullptr;
    const hipError_t rc = s ? hipSuccess : hipStreamCreateWithFlags(&h, hipStreamNonBlocking);
    if (h) s.reset(h);
    return rc;
}

// (the records an index keeps in HBM — HibfNode, ChildRec, VChunk, VPath, VSplit, VSplitRange — and VLevel: txq_records.hpp)

// One HIBF work item: k-mer `kmer` (index into the batch) must be looked up in IBF `ibf`.
struct WorkItem { uint32_t kmer; uint32_t ibf; };

struct Index {
    int device = 0;
    bool is_hibf = false;
    uint64_t user_bins = 0, mask_words = 0, shard_word0 = 0, shard_words = 0, device_bytes = 0;
    std::vector<IbfDev> ibf;  // host copies of the device descriptors ([0] = flat IBF / HIBF root)
    // The IBFs' words (IbfDev::words: the record goes to kernels by value and owns nothing) and every array below that an HIBF
    // upload sends to the device (txq_hibf.hip device_array) are owned through this list: a new one needs its field here and its
    // call there.  The fields that point at them die with the index.
    std::vector<DeviceBuffer<void>> uploaded;

    // HIBF tree in HBM
    IbfDev* d_ibf = nullptr;         // [n_ibf]
    uint64_t* d_next = nullptr;      // flattened next_ibf_id
    uint64_t* d_tb_user = nullptr;   // flattened tb_to_user_bin (TXQ_MERGED_BIN for merged)
    uint64_t* d_map_off = nullptr;   // [n_ibf] offset of IBF i's maps in the flattened arrays
    uint64_t* d_merged = nullptr;    // merged-bin bitmask words of every IBF, flattened
    HibfNode* d_nodes = nullptr;     // [total technical bins + 1] for the fused descent (txq_hibf.hip)
    uint64_t* d_descend = nullptr;   // same layout: merged bins worth descending into for this shard
    uint64_t* d_merged_off = nullptr;
    // Regular two-level trees (root of merged bins over leaf IBFs that each map an aligned run of user bins, all of
    // one row width): the child-stationary descent of txq_hibf.hip (rows of >= 2 words) and the fused dense steps of
    // txq_exec.hip.  d_children = ChildRec[n_children] in mask-column
    // order for THIS shard's columns; empty when the tree does not have that shape.
    ChildRec* d_children = nullptr;
    uint32_t n_children = 0;         // children whose columns this shard owns
    uint32_t child_row_words = 0;    // mask words per child (a power of two)
    // Small regular trees with uniform children (root of <= 64 merged bins, mask of <= 32 words): the children's matrices
    // once more, row r of all children side by side ([rows][stride] like a flat IBF over the children's hash parameters),
    // so that a dense step gathers one row segment per hash function instead of one cache line per child.
    IbfDev interleaved{};
    // plain k-mer probes go to the interleaved children too (TXQ_HIBF_INTERLEAVE_PROBE=0: the tree descent kernels; A/B and tests)
    bool probes_interleaved(const Knobs& kn) const {
        return is_hibf && interleaved.words && interleaved.stride >= 2 && !(interleaved.stride & 1) && interleaved.shard_words == shard_words &&
               root_node.bins <= 64 && kn.hibf_interleave_probe;
    }
    HibfNode root_node{};            // host copy of the root's record
    uint32_t tree_hash_max = 0;      // most hash functions of any IBF of the tree (every HIBF: set at upload)
    bool children_uniform = false;   // same rows / hash shift / hash count in every child: scalar hashing
    uint64_t children_bytes = 0;     // their matrices
    DeviceBuffer<uint32_t> scratch_crows;  // uniform children: per k-mer its row indexes in a child
    DeviceBuffer<uint64_t> scratch_cm;  // root pass output: per k-mer the root row (which children to visit)
    // layout order (see VChunk): built at upload for trees that are not regular, one shard, fewer than 2^32 rows per IBF
    VChunk* d_vchunks = nullptr;
    VPath* d_vpaths = nullptr;
    uint64_t* d_vleaf = nullptr;     // [v_words] bits of technical bins that are user bins (the ONES of a layout-order session)
    uint32_t* d_vuser = nullptr;     // [v_words * 64] user bin of a layout-order bit (kNoGate: none)
    uint32_t* d_vgroups = nullptr;   // per level its groups' first chunks, concatenated (+ end)
    uint64_t* d_vnonrep = nullptr;   // [v_words] bits of the parts of split user bins that are not their representative (null: no split bins)
    uint32_t* d_vrep = nullptr;      // [v_words * 64] for such a bit: the representative's bit position in the row
    VSplitRange* d_vsplit_range = nullptr;  // [n_vchunks]
    VSplit* d_vsplits = nullptr;
    uint64_t* d_vside = nullptr;     // the side matrices of all IBFs with split bins
    HibfNode* d_vnodes = nullptr;    // records as d_nodes whose ident_word is the IBF's first word in the layout-order row
    uint32_t v_inner_words = 0;  // of a row: the words of IBFs with merged bins (what the next level reads as gates)
    uint32_t v_words = 0, n_vchunks = 0, v_depth = 0, v_chunk_words = 2;  // (chunks of 16 bytes, or of 8 for trees of narrow IBFs)
    std::vector<VLevel> vlevels;
    bool layout_order(const Knobs& kn) const;  // sessions on this index work in layout order
    uint32_t depth = 1;              // levels of the tree
    uint64_t hibf_total_tbs = 0;     // technical bins over all IBFs of the tree
    uint64_t max_level_width = 1;    // max number of IBFs on one level (bounds the frontier)
    uint32_t max_stride = 1;         // widest row over all IBFs (words)

    // grow-only scratch of the descent and of txq_count (owned by the index; one host thread at a time).  No buffer of a session
    // is among them, and none is shared between two sessions of one index: what a session uses it owns (SessionBuffers below).
    DeviceBuffer<WorkItem> frontier[2];
    DeviceBuffer<uint32_t> d_counts;
    DeviceBuffer<uint64_t> scratch_dense_kmers;      // dense steps on an HIBF: the pairs' k-mers ...
    DeviceBuffer<uint64_t> scratch_dense_masks;      // ... and their descended masks
    // txq_count_windows on an HIBF: what the last call did (txq_count_windows_trace), kCwTraceSlots sets of four u64 totals the waves add to
    struct CountWindowsTrace {
        DeviceBuffer<unsigned long long> totals;
        Event done;             // behind the last call's last kernel
        bool recorded = false;
    } count_windows_trace;
    DeviceBuffer<uint32_t> scratch_count_acc;        // txq_count on a flat index: long queries' partial counts
    DeviceBuffer<unsigned char> scratch_count_io;    // txq_count (host buffers): the call's inputs and results
    // A flat index's masks of ALL k-mers, M[v] at kmer_table + v * shard_words for every packed value v < 2^(bits * k) (txq_exec.hip
    // ensure_kmer_table): where that fits TXQ_KMER_TABLE_MB, a dense step reads ONE row per k-mer instead of gathering hash_funs.
    DeviceBuffer<uint64_t> kmer_table; uint32_t kmer_table_bits = 0;  // bits = bits per residue * k of the table that is built
    bool kmer_table_refused = false;                               // (the allocation failed once: not tried again)
    std::mutex table_mutex;                                        // building / dropping the table (sessions of one index may run on several threads)
    // Calls that changed a flat index's bits after it was made: txq_emplace_device, the only writer of ibf[0].words besides upload
    // and create (which make a new Index).  What is derived from the bits and kept remembers the generation it was derived from.
    uint64_t generation = 0;  // (read and written under probe_table.mutex)
    // The flat probe's table of its batches' k-mer domain (txq_probe.hip probe_flat): T[v] = the mask of value v, for v below
    // a device word `built`.  The rows depend on the index's bits alone, so they are kept from call to call and extended when
    // a batch's domain is larger; they are started over (txq_probe_plan.hpp plan_probe_call) when `generation` — the calls
    // that changed the bits, txq_emplace_device — is not the one they were built for, when the table was just (re)allocated,
    // and on every call under TXQ_PROBE_TABLE_KEEP=0.  `done` is recorded behind a call's last kernel and the next call, on
    // whatever stream, waits for it; so does txq_emplace_device before it changes the bits.  Everything here is read and
    // written under `mutex`.
    struct ProbeTable {
        DeviceBuffer<uint64_t> rows; size_t cap_rows = 0;  // [cap_rows][stride]
        DeviceBuffer<uint32_t> state;                   // [kStateWords]: sample accumulators, the valid-rows word twice, statistics (txq_probe_plan.hpp)
        ProbeKeep keep;                                 // the generation the rows belong to, the calls so far
        Event done;
        bool recorded = false, refused = false;         // (refused: the allocation failed once, not tried again)
        // scratch of the sorted answer (plan_probe_sort): the batch's records in bucket order; counts[bucket][chunk] and,
        // behind them, kSortMaxBuckets bucket totals.  Grown like `rows`; sort_refused: an allocation failed once.
        DeviceBuffer<uint64_t> sort_records;
        DeviceBuffer<uint32_t> sort_counts;
        bool sort_refused = false;
        uint64_t sort_planned = 0;                      // calls that launched the partition since the state words were last zeroed (txq_index_probe_sorted)
        std::mutex mutex;
    } probe_table;

    // Device buffers of the last session, kept for the next one: a single query must not pay
    // hipMalloc/hipFree (they cost more than its kernels).  One session at a time may hold them.
    // (the chunks and dense blocks an index keeps for the next session — ArenaChunk, DenseBlock, BlockBins, BookCache: txq_exec_plan.hpp)
    // What one stage of a session uploads: the blob, and `aux` = program table, lists, units, tiles, region moves and the
    // table of region bases.  A session alternates between two sets, so stage n+1 is uploaded (on its own stream) while
    // the kernels of stage n still read theirs; `done` is recorded behind a stage's last kernel.
    struct StagingSet {
        DeviceBuffer<unsigned char> d_blob, d_aux;
        DeviceBuffer<uint64_t> d_masks;  // M[k-mer] of the stage's k-mer table (the probe's output)
        Event done;
        bool pending = false;
    };
    // The buffers and streams a session works with.  A session that gets the cache takes them over by move and moves them
    // back at its end; one that does not makes its own and frees them: no two sessions ever share one.
    struct SessionBuffers {
        StagingSet set[2];                  // stage n uses set[n & 1]
        Stream upload;                      // the uploads' stream (non-blocking: independent of the stream the kernels run on)
        Stream side;                        // a stage that continues nothing of the stage in flight runs beside it, on this stream
        PinnedBuffer<uint64_t> host_final;  // the final masks are gathered straight into host memory ...
        DeviceBuffer<uint64_t> dev_final;   // ... or (TXQ_FINAL_PINNED=0, layout order, more than 64 MiB) here and copied
        DeviceBuffer<uint64_t> layout_rows; // a layout-order session's RESULT rows before they are put in user-bin order
    };
    struct SessionCache : BookCache, SessionBuffers {
        bool in_use = false;
        ~SessionCache() {
            free_chunks<DeviceMem>(chunks);
            free_chunks<DeviceMem>(block_chunks);
        }
    } session_cache;
    static constexpr size_t kArenaKeepBytes = (size_t)64 << 30;
    uint64_t user_tag = 0;  // txq_index_set_tag
    int open_sessions = 0;  // txq_index_free refuses while a session still points at this index
    bool join_or = false;   // a sub-tree shard of a general HIBF (txq_index_upload_subtrees): full-width masks, ORed with the other shards'
    int shard_rank = 0, n_shards = 1;

    // txq_probe (host buffers): two streams with their device and pinned bounce buffers
    struct HostPipe {
        Stream stream[2];
        Event done[2];
        DeviceBuffer<uint64_t> d_kmers[2], d_masks[2];
        PinnedBuffer<uint64_t> bounce[2];
    } host_pipe;
};

// Does a session on this index run dense steps fused on the tree (txq_exec.hip TreeRows / InterleavedRows)?  A regular
// two-level HIBF whose children tile this shard's mask columns.  TXQ_DENSE_TREE=0 (A/B and tests) sends steps through
// the generic HIBF path instead.
inline bool Index::layout_order(const Knobs& kn) const {
    return is_hibf && d_vchunks && v_words && kn.hibf_layout_order && shard_words == mask_words && shard_word0 == 0;
}
inline bool index_fuses_tree_steps(const Index& ix, const Knobs& kn) {
    return ix.is_hibf && ix.d_children && ix.n_children && kn.dense_tree != 0 && ix.tree_hash_max >= 1 && ix.tree_hash_max <= 5 &&
           (uint64_t)ix.n_children * ix.child_row_words == ix.shard_words;
}

// A batch of programs whose slot masks persist in HBM across stages (txq_exec.hip).
struct Session : Index::SessionBuffers {
    Index* ix = nullptr;
    Index* aux = nullptr;  // optional d-gram index (flat IBF, same bins and shard as ix)
    Knobs kn;              // the environment switches as they were when the session began
    size_t n_programs = 0;
    uint32_t W = 0;        // words of a slot mask: the shard's mask words, or (vspace) the words of a layout-order row
    bool failed = false;   // a stage failed after it may have launched kernels: the device was drained, further stages are refused
    bool vspace = false;   // the index is a general HIBF: masks are rows in layout order, final masks are converted (Index::layout_order)
    SlotBook book;         // the programs' slot regions and dense blocks (txq_exec_plan.hpp)
    double block_alloc_seconds = 0;  // spent in hipMalloc for block chunks (TXQ_TRACE)
    size_t n_block_memsets = 0, n_sparse_launches = 0, n_sparse_groups = 0;
    int stream_of_last = 0;            // 0: the caller's stream, 1: `side`
    uint64_t** d_base = nullptr;  // device copy of `base` as of the last stage (lives in that stage's staging set)
    bool owns_cache = false;      // the SessionBuffers and the book's chunks came from / go back to ix->session_cache
    std::vector<DeviceBuffer<void>> retired;  // staging buffers that were outgrown while another stage was running: freed with the session
    DeviceBuffer<unsigned long long> d_step_ctr;  // TXQ_TRACE: what sparse_units_kernel did (entries, units, non-empty products, units that left a bit)
    std::vector<unsigned char> host_aux;  // a small stage is packed here and sent as one copy
    // where a stage's wall time goes (reported on stderr at session end when TXQ_TRACE is set)
    double t_validate = 0, t_upload = 0, t_device = 0;
    double t_grow = 0, t_plan = 0, t_wait = 0, t_alloc = 0;  // parts of t_upload: slot regions, units/tiles, waiting for the staging set, scratch
    const char* row_source = "none";  // where the dense steps of the last stage took M[k-mer] from
    // what the dense ops of the session amount to (TXQ_TRACE): predecessor visits and destination suffixes of the steps,
    // slots zeroed, entries reduced — the algorithmic bytes of dense_kernel follow from these and the mask width
    uint64_t n_step_pairs = 0, n_step_suffixes = 0, n_zero_slots = 0, n_reduce_entries = 0;
    size_t n_beside = 0;  // stages that ran on the other stream than their predecessor
    size_t n_stages = 0, bytes_uploaded = 0, n_dense_tiles = 0, n_levels = 0, n_unit_launches = 0, n_units = 0, n_dense_launches = 0;
    ~Session();
};

// The device code of a translation unit is loaded when one of its kernels is first needed — 14 ms for the executor's
// kernels, which a single `tetrex query` would pay inside its query time.  txq_init asks for them right away (the CLI
// calls it on a helper thread while the index file is parsed).
void preload_exec_kernels();
void preload_probe_kernels();
void preload_hibf_kernels();

hipStream_t take_spare_stream(int device);  // a non-blocking stream made at txq_init, or null (txq_api.hip)

int require_init();  // txq_init has run; binds the calling thread to the first device
int fail(int code, const char* fmt, ...);
int fail_hip(hipError_t e, const char* what);
// what Buffer::reserve returned, as a TXQ_* code
inline int reserved(int e, const char* what) { return e ? fail_hip((hipError_t)e, what) : TXQ_OK; }
// one IBF (column slice [w0, w1) of its rows) in HBM, appended to ix.ibf and counted in ix.device_bytes (txq_api.hip)
int alloc_ibf(Index& ix, const txq_ibf_desc& d, uint64_t w0, uint64_t w1);

// An environment variable as a number in [lo, hi]; `def` where it is unset or empty.  For the knobs that are read per call
// (TXQ_EDIT_CHUNK, TXQ_REGEX_CHUNK, TXQ_REGEX_MAX_SERIAL: tests change them between calls), not at the entry points above.
inline uint32_t env_u32(const char* name, uint32_t def, uint32_t lo, uint32_t hi) {
    const char* e = std::getenv(name);
    const long long c = e && *e ? std::atoll(e) : (long long)def;
    return (uint32_t)(c < (long long)lo ? lo : c > (long long)hi ? hi : c);
}

// off[0 .. n] ascend — and stay at or below `upper`, the size of the array `within` that they point into, where one is given
inline int check_ascending(const uint64_t* off, size_t n, const char* what, const char* within = nullptr, uint64_t upper = UINT64_MAX) {
    for (size_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i] || off[i + 1] > upper)
            return within ? fail(TXQ_ERR_ARG, "%s offsets are not ascending within the %s at %s %zu", what, within, what, i)
                          : fail(TXQ_ERR_ARG, "%s offsets are not ascending at %s %zu", what, what, i);
    return TXQ_OK;
}
// off[0 .. n] as the device form takes them: counted from off[0]
inline std::vector<uint64_t> rebased(const uint64_t* off, size_t n) {
    std::vector<uint64_t> v(off, off + n + 1);
    for (uint64_t& o : v) o -= off[0];
    return v;
}

// The device side of a host-buffer call (txq_translate, txq_edit_search, txq_regex_filter): add() the buffers' sizes, alloc()
// makes ONE allocation and every buffer a 256-byte aligned slice of it, upload / download are synchronous copies that do
// nothing once a call has failed — error() is the first failure —, and the destructor frees.
class DeviceStage {
public:
    size_t add(size_t bytes) {
        const size_t at = total_;
        total_ += (bytes + 255) & ~(size_t)255;
        return at;
    }
    hipError_t alloc() { return err_ = hipMalloc((void**)&base_, total_); }
    template <class T>
    T* at(size_t slice) const { return reinterpret_cast<T*>(base_ + slice); }
    void upload(size_t slice, const void* src, size_t bytes) {
        if (err_ == hipSuccess && bytes) err_ = hipMemcpy(base_ + slice, src, bytes, hipMemcpyHostToDevice);
    }
    void download(void* dst, size_t slice, size_t bytes) {
        if (err_ == hipSuccess && bytes) err_ = hipMemcpy(dst, base_ + slice, bytes, hipMemcpyDeviceToHost);
    }
    hipError_t error() const { return err_; }
    ~DeviceStage() { (void)hipFree(base_); }
    DeviceStage() = default;
    DeviceStage(const DeviceStage&) = delete;
    DeviceStage& operator=(const DeviceStage&) = delete;

private:
    unsigned char* base_ = nullptr;
    size_t total_ = 0;
    hipError_t err_ = hipSuccess;
};

// txq_probe.hip
hipError_t launch_probe(const IbfDev& f, const uint64_t* kmers, size_t n, uint64_t* masks, uint64_t* alive, hipStream_t s);
// txq_probe_device on a flat index: launch_probe, or the domain-table path where the batch's k-mer domain is small
hipError_t probe_flat(Index& ix, const Knobs& kn, const uint64_t* kmers, size_t n, uint64_t* masks, uint64_t* alive, hipStream_t s);
hipError_t launch_probe_interleaved(const IbfDev& interleaved, const HibfNode& root, const void* children, uint32_t wpr_log2, const uint64_t* kmers,
                                    size_t n, uint64_t* masks, uint64_t* alive, hipStream_t s);
hipError_t launch_emplace(const IbfDev& f, const uint64_t* values, const uint32_t* bins_of, size_t n, hipStream_t s);

// txq_hibf.hip
int hibf_upload(Index& ix, const txq_index_desc& desc, bool cleared_ok = false);
int hibf_probe(Index& ix, const Knobs& kn, const uint64_t* d_kmers, size_t n, uint64_t* d_masks, uint64_t* d_alive, hipStream_t s);
// layout-order rows of n k-mers: d_rows[n][v_words]
int hibf_probe_layout_order(Index& ix, const uint64_t* d_kmers, size_t n, uint64_t* d_rows, hipStream_t s);
// final masks of a layout-order session -> user-bin order: d_out[n][shard_words] (zeroed here)
int hibf_layout_to_user(const Index& ix, const uint64_t* d_rows, size_t n, uint64_t* d_out, hipStream_t s);

// txq_count.hip: threshold membership of n_queries value sets (include/txq.h txq_count_device; arguments checked by the caller)
int count_device(Index& ix, const uint64_t* d_values, const uint64_t* d_offsets, size_t n_queries, const uint32_t* d_thr,
                 uint64_t* d_hits, uint32_t* d_counts, hipStream_t s);
// the same of n_windows sliding windows [d_begin[j], d_begin[j] + d_len[j]) (txq_count_windows_device)
int count_windows_device(Index& ix, const uint64_t* d_values, const uint64_t* d_begin, const uint32_t* d_len, size_t n_windows,
                         const uint32_t* d_thr, uint64_t* d_hits, uint32_t* d_counts, hipStream_t s);

// txq_exec.hip
// (final_on_host: `final` is host memory, filled through the session's device buffer)
int run_programs(Index& ix, const void* blob, size_t blob_bytes, size_t n_programs, uint64_t* final, bool final_on_host, hipStream_t s);
int session_begin(Index& ix, size_t n_programs, Session** out);
int session_stage(Session& s, const void* blob, size_t bytes, const uint32_t* q_prog, const uint32_t* q_slot, size_t n_q,
                  uint8_t* alive, hipStream_t st);
int session_finish(Session& s, uint64_t* d_final, hipStream_t st);
// the final masks in host memory (null stream): gathered straight into the session's pinned buffer, or (pinned == false)
// into its device buffer and copied; *t_finish (if given): when the last launch was issued
int session_finish_host(Session& s, uint64_t* final_masks, bool pinned, double* t_finish = nullptr);

}  // namespace txq
