// What a stage of a session works out on the host before anything is uploaded or launched: plain C++ on the blob and a few
// vectors (no HIP, no Index, no Session), so that all of it runs without a GPU (tests/native/exec_plan_dump.cpp).  The phases of
// txq_exec.hip session_stage call these in order and add timing, trace counters and fail(); DESIGN.md "Executor: stage planning"
// says what each planned list is for and who reads it.
//   validate_blob        the gate: nothing malformed may reach the GPU; normalises the program table (BlobView)
//   check_questions      feedback questions: program and slot in range
//   SlotBook             the books on the programs' slot regions and dense blocks: grow, recycling, the pool an index keeps
//   plan_units           a stage's ops -> units, tile groups, sparse groups, HIBF steps; every dense op's block pointers
//   chunk_hibf_steps     HIBF steps in chunks whose masks fit the scratch
// Device addresses are only ever computed here, never followed: a new chunk of memory comes from a callable the caller passes.
#pragma once
#include "txq_records.hpp"
#include "../../include/txq.h"
#include "../../include/txq_program.h"
#include <algorithm>
#include <atomic>
#include <functional>
#include <thread>
#include <utility>

namespace txq {

// ---- the stage records shared by host and kernels -----------------------------------------------------------------------
// Normalised program descriptor the executor kernel reads (both blob versions map onto it).
struct DevProgram { uint32_t first_op, n_ops, first_level, n_levels; };

// Big programs: one launch per dependency level, the level's ops of ALL big programs cut into units of <= unit_ops(W) ops.
struct ExecUnit { uint32_t program, begin, end; };
static constexpr uint32_t kUnitWords = 2048;  // mask words one unit moves per operand: 128 ops of a 1024-bin index, 2 ops at 65536 bins
static inline uint32_t unit_ops(uint32_t W) { return W >= kUnitWords ? 1u : kUnitWords / W; }

// One workgroup per tile: `count` work entries of one dense op, starting at `first`.
//   ZERO    entries = slots of the block
//   REDUCE  entries = suffixes inside shape[0] x .. x shape[k-2]
//   STEP    entries = destination suffixes (x1 .. x_{k-2}, r) inside shape[1] x .. x shape[k-2] x R; each is
//           handled by G lanes (a lane owns 16 bytes of the mask: WIDE, or one word) which loop over the
//           predecessors a in shape[0], two at a time: 2 * (H row gathers + 1 source mask) loads in flight
struct DenseTile { uint32_t program, op, first, count; };
// The host does not spell the tiles of a stage out (the bench batch: 210 000 of them for 6 800 dense ops): it sends one
// group per dense op — its tiles are [first_tile, first_tile + ceil(entries / per_tile)) of the stage's tile array, the
// groups of one level back to back — and make_tiles_kernel writes them (one workgroup per group).
struct TileGroup { uint32_t program, op, entries, per_tile; uint64_t first_tile; };
struct DenseParams { uint32_t k, bits, A, canonical, pos; uint32_t pow_a[TXQ_DENSE_MAX_POSITIONS + 1]; uint32_t nt; };  // nt: A/B bits (TXQ_DENSE_NT): 1 destination stores, 2 destination loads
// Where the blocks (and slots) of a stage's dense op live, resolved by the host side when it plans the stage:
// dst = the block written (ZERO, STEP, FILL) or the slot accumulated into (REDUCE); src = the block read (STEP, REDUCE) or
// the slot spread (FILL).  A tile reads this next to the op itself: no pointer chase through the program's tables.
struct DenseOpPtr { uint64_t* dst; const uint64_t* src; uint32_t dst_cap, src_cap; };  // (capacities of the blocks: where their live lists sit)

// The dense ops of tracked programs: one group per op, its work follows the block's live list (sparse_kernel).
struct SparseGroup { uint32_t op; uint32_t fixed; };  // fixed != kNotFixed: the host knows the entries (FILL: its shape)
static constexpr uint32_t kNotFixed = 0xFFFFFFFFu;
static constexpr uint32_t kSparseChunk = 64;
static constexpr uint32_t kMaxSparseGroups = 1024;  // per launch (the chunk totals sit in LDS)

// grown slot regions keep their contents (move_regions_kernel); blocks a tracked program takes over start all zero
// (clear_blocks_kernel: src unused)
struct RegionMove { uint64_t* dst; const uint64_t* src; size_t words; };

// A dense block in HBM: [cap][W] mask words, then its live list (include/txq_program.h, tracked programs): a 64-byte
// header — number of listed entries, capacity, the block's geometry —, a bitmap of cap bits ("entry is listed"), the list.
static constexpr uint32_t kBlockHeaderWords = 8;
TXQ_HOST_DEVICE inline size_t block_meta_words(uint32_t cap) { return kBlockHeaderWords + ((size_t)cap + 63) / 64 + ((size_t)cap + 1) / 2; }
inline size_t block_alloc_words(uint32_t cap, uint32_t W) { return ((size_t)cap * W + block_meta_words(cap) + 1) & ~(size_t)1; }

// ---- the blob -------------------------------------------------------------------------------------------------------------
// Host-side validation: nothing malformed may reach the GPU (a stray slot or k-mer index would
// be an out-of-bounds access there).  Accepts version 1 (op order), 2 (levels) and 4 (levels + dense
// ops) blobs and normalises the program table.
struct BlobView {
    uint32_t n_kmers = 0, n_ops = 0, n_levels = 0, n_dense = 0;
    uint64_t kmers_offset = 0, ops_offset = 0, levels_offset = 0, n_aux_kmers = 0, dense_offset = 0;
    DenseParams dense{};       // (nt: set by the caller)
    uint32_t block_slots = 0;  // A^(k-1) when the blob has dense ops
    std::vector<DevProgram> programs;
    std::vector<uint32_t> n_slots, n_blocks;  // per program: ordinary slots; dense blocks (ids 0 .. n-1)
    std::vector<uint8_t> has_dense;  // the program has dense ops in this stage
    std::vector<uint8_t> tracked;    // TXQ_PROGRAM_TRACKED_BIT
};

inline PlanError validate_blob(const unsigned char* blob, size_t bytes, size_t n_programs, BlobView* out) {
    const int bad_blob = TXQ_ERR_PROGRAM;
    if (bytes < sizeof(txq_blob_header)) return plan_refusal(bad_blob, "blob shorter than its header");
    if ((uintptr_t)blob % 8) return plan_refusal(bad_blob, "blob must be 8-byte aligned");
    const txq_blob_header* h1 = (const txq_blob_header*)blob;
    if (h1->magic != TXQ_PROGRAM_MAGIC) return plan_refusal(bad_blob, "bad blob magic");
    const bool v3 = h1->version == TXQ_PROGRAM_VERSION_DENSE;  // (levels + dense ops)
    const bool v2 = v3 || h1->version == TXQ_PROGRAM_VERSION_LEVELS;
    if (!v2 && h1->version != TXQ_PROGRAM_VERSION) return plan_refusal(bad_blob, "unsupported blob version %u", h1->version);
    if (bytes < (v3 ? sizeof(txq_blob_header_v3) : v2 ? sizeof(txq_blob_header_v2) : sizeof(txq_blob_header)))
        return plan_refusal(bad_blob, "blob shorter than its header");
    const txq_blob_header_v2* h2 = (const txq_blob_header_v2*)blob;
    const txq_blob_header_v3* h3 = (const txq_blob_header_v3*)blob;
    BlobView v;
    uint64_t programs_offset;
    if (v2) {
        v.n_kmers = h2->n_kmers; v.n_ops = h2->n_ops; v.n_levels = h2->n_levels;
        v.kmers_offset = h2->kmers_offset; v.ops_offset = h2->ops_offset; v.levels_offset = h2->levels_offset;
        v.n_aux_kmers = h2->n_aux_kmers;
        if (v.n_aux_kmers > v.n_kmers) return plan_refusal(bad_blob, "more auxiliary k-mers than k-mers");
        programs_offset = h2->programs_offset;
        if (h2->n_programs != n_programs) return plan_refusal(bad_blob, "blob holds %u programs, caller says %zu", h2->n_programs, n_programs);
    } else {
        v.n_kmers = h1->n_kmers; v.n_ops = h1->n_ops;
        v.kmers_offset = h1->kmers_offset; v.ops_offset = h1->ops_offset;
        programs_offset = h1->programs_offset;
        if (h1->n_programs != n_programs) return plan_refusal(bad_blob, "blob holds %u programs, caller says %zu", h1->n_programs, n_programs);
    }
    auto in_range = [&](uint64_t off, uint64_t count, uint64_t elem) {
        return off % 4 == 0 && off <= bytes && count <= (bytes - off) / elem;
    };
    if (v.kmers_offset % 8 || !in_range(v.kmers_offset, v.n_kmers, 8) || !in_range(v.ops_offset, v.n_ops, sizeof(txq_op)) ||
        !in_range(programs_offset, n_programs, v2 ? sizeof(txq_program_v2) : sizeof(txq_program)) ||
        (v2 && !in_range(v.levels_offset, v.n_levels, 4)))
        return plan_refusal(bad_blob, "blob table outside the blob");
    if (v3) {
        v.n_dense = h3->n_dense;
        v.dense_offset = h3->dense_offset;
        if (v.dense_offset % 8 || !in_range(v.dense_offset, v.n_dense, sizeof(txq_dense_op))) return plan_refusal(bad_blob, "dense table outside the blob");
        DenseParams& P = v.dense;
        P.k = h3->k; P.bits = h3->bits; P.A = h3->alphabet; P.canonical = h3->canonical ? 1u : 0u;
        if (P.k < 2 || P.k - 1 > TXQ_DENSE_MAX_POSITIONS || P.bits < 1 || P.bits > 8 || (uint64_t)P.bits * P.k > 64 || P.A < 1 || P.A > 32 ||
            P.A > (1u << P.bits) || (P.canonical && P.bits != 2))
            return plan_refusal(bad_blob, "dense parameters out of range (k %u, %u bits, alphabet %u)", P.k, P.bits, P.A);
        P.pos = P.k - 1;
        uint64_t n = 1;
        P.pow_a[0] = 1;
        for (uint32_t j = 1; j <= P.pos; ++j) {
            n *= P.A;
            if (n > (1u << 22)) return plan_refusal(bad_blob, "dense block of %u^%u slots is too large", P.A, P.pos);
            P.pow_a[j] = (uint32_t)n;
        }
        v.block_slots = (uint32_t)n;
    }
    v.programs.resize(n_programs);
    v.n_slots.resize(n_programs);
    v.n_blocks.assign(n_programs, 0);
    v.has_dense.assign(n_programs, 0);
    v.tracked.assign(n_programs, 0);
    const txq_op* ops = (const txq_op*)(blob + v.ops_offset);
    const txq_dense_op* dops = v3 ? (const txq_dense_op*)(blob + v.dense_offset) : nullptr;
    const uint32_t* levels = v2 ? (const uint32_t*)(blob + v.levels_offset) : nullptr;
    for (uint32_t p = 0; p < n_programs; ++p) {
        DevProgram d{};
        if (v2) {
            const txq_program_v2& s = ((const txq_program_v2*)(blob + programs_offset))[p];
            d = DevProgram{s.first_op, s.n_ops, s.first_level, s.n_levels};
            v.n_slots[p] = s.n_slots;
            if (v3) {
                v.tracked[p] = (s.reserved & TXQ_PROGRAM_TRACKED_BIT) != 0;
                v.n_blocks[p] = s.reserved & ~TXQ_PROGRAM_TRACKED_BIT;
                if (v.n_blocks[p] > TXQ_DENSE_MAX_BLOCKS) return plan_refusal(bad_blob, "program %u: more than %u dense blocks", p, TXQ_DENSE_MAX_BLOCKS);
            }
        } else {
            const txq_program& s = ((const txq_program*)(blob + programs_offset))[p];
            d = DevProgram{s.first_op, s.n_ops, 0, 0};
            v.n_slots[p] = s.n_slots;
        }
        const uint32_t n_slots = v.n_slots[p];
        if (n_slots < TXQ_SLOT_FIRST_FREE || n_slots >= TXQ_DENSE_SLOT_BIT) return plan_refusal(bad_blob, "program %u: n_slots out of range", p);
        if (d.first_op > v.n_ops || d.n_ops > v.n_ops - d.first_op) return plan_refusal(bad_blob, "program %u: ops out of range", p);
        if (d.n_levels) {
            if (d.first_level > v.n_levels || d.n_levels > v.n_levels - d.first_level) return plan_refusal(bad_blob, "program %u: levels out of range", p);
            uint32_t prev = 0;
            for (uint32_t l = 0; l < d.n_levels; ++l) {
                const uint32_t e = levels[d.first_level + l];
                if (e < prev || e > d.n_ops) return plan_refusal(bad_blob, "program %u: level table not ascending", p);
                prev = e;
            }
            if (prev != d.n_ops) return plan_refusal(bad_blob, "program %u: levels do not cover the ops", p);
        }
        v.programs[p] = d;
    }
    // every op of every program: operands inside the program's slot regions, k-mer inside the table, dense ops on
    // whole blocks.  Large stages (hundreds of MB of ops) are checked by several threads, each taking whole programs.
    struct Bad { uint32_t program = 0xFFFFFFFFu, op = 0; int kind = 0; };
    auto check_program = [&](uint32_t p, Bad& bad) {
        const DevProgram& d = v.programs[p];
        const uint32_t n_slots = v.n_slots[p], n_blocks = v.n_blocks[p];
        const bool tracked = v.tracked[p] != 0;
        const txq_op* o = ops + d.first_op;
        // a dense slot: an existing block id; its index inside A^(k-1) for untracked blocks (a tracked block's capacity is only
        // known to the session: plan_units checks those)
        auto slot_ok = [&](uint32_t s) {
            if (s & 0x80000000u) return false;
            if (!(s & TXQ_DENSE_SLOT_BIT)) return s < n_slots;
            return ((s & ~TXQ_DENSE_SLOT_BIT) >> TXQ_DENSE_BLOCK_SHIFT) < n_blocks && (tracked || (s & TXQ_DENSE_INDEX_MASK) < v.block_slots);
        };
        auto block_ok = [&](uint32_t s) {
            return !(s & 0x80000000u) && (s & TXQ_DENSE_SLOT_BIT) && (s & TXQ_DENSE_INDEX_MASK) == 0 && ((s & ~TXQ_DENSE_SLOT_BIT) >> TXQ_DENSE_BLOCK_SHIFT) < n_blocks;
        };
        for (uint32_t i = 0; i < d.n_ops; ++i) {
            int kind = 0;
            if (o[i].kmer == TXQ_DENSE_OP) {
                if (!v3 || o[i].dst >= v.n_dense || d.n_levels == 0) kind = 4;
                else {
                    const txq_dense_op& x = dops[o[i].dst];
                    const uint32_t code_mask = v.dense.A >= 32 ? 0xFFFFFFFFu : ((1u << v.dense.A) - 1u);
                    bool ok = x.kind <= TXQ_DENSE_FILL;
                    if (ok) ok = ((x.reserved & TXQ_DENSE_TRACKED) != 0) == (v.tracked[p] != 0) && (x.reserved & ~(TXQ_DENSE_TRACKED | TXQ_DENSE_NOPROBE)) == 0;
                    if (ok && (x.reserved & TXQ_DENSE_NOPROBE)) ok = x.kind == TXQ_DENSE_STEP && v.tracked[p] != 0;  // (only the pushed steps of tracked programs)
                    if (ok && x.kind != TXQ_DENSE_REDUCE) ok = block_ok(x.dst);
                    if (ok && (x.kind == TXQ_DENSE_STEP || x.kind == TXQ_DENSE_REDUCE)) ok = block_ok(x.src);
                    if (ok && x.kind == TXQ_DENSE_FILL) ok = !(x.src & TXQ_DENSE_SLOT_BIT) && x.src < n_slots;
                    if (ok && (x.kind != TXQ_DENSE_ZERO || x.r_mask))
                        for (uint32_t j = 0; ok && j < v.dense.pos; ++j) ok = (x.shape[j] & ~code_mask) == 0;
                    if (ok && x.kind == TXQ_DENSE_STEP) ok = x.src != x.dst && (x.r_mask & ~code_mask) == 0;
                    if (ok && x.kind == TXQ_DENSE_REDUCE) ok = slot_ok(x.dst) && x.dst != TXQ_SLOT_ZERO && x.dst != TXQ_SLOT_ONES && !(tracked && (x.dst & TXQ_DENSE_SLOT_BIT));
                    if (ok && x.kind == TXQ_DENSE_ZERO && tracked) {  // (re)creates the block: geometry in shape[], capacity in src
                        uint64_t entries = 1;
                        for (uint32_t j = 0; j < v.dense.pos; ++j) entries *= (uint64_t)__builtin_popcount(x.shape[j]);
                        ok = entries >= 1 && entries <= x.src && x.src <= (1u << TXQ_DENSE_BLOCK_SHIFT);
                    }
                    if (!ok) kind = 4;
                    v.has_dense[p] = 1;
                }
            } else if (!slot_ok(o[i].dst) || !slot_ok(o[i].a) || !slot_ok(o[i].b)) kind = 1;
            else if (o[i].dst == TXQ_SLOT_ZERO || o[i].dst == TXQ_SLOT_ONES) kind = 2;
            else if (o[i].kmer != TXQ_NO_KMER && o[i].kmer >= v.n_kmers) kind = 3;
            else if ((o[i].dst | o[i].a | o[i].b) & TXQ_DENSE_SLOT_BIT) {  // an ordinary op on block entries: the program runs level by level, like one with dense ops
                if (d.n_levels == 0) kind = 4;
                v.has_dense[p] = 1;
            }
            if (kind) { if (p < bad.program) bad = Bad{p, i, kind}; return; }
        }
    };
    Bad bad;
    unsigned n_threads = v.n_ops >= (1u << 20) ? std::min(8u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
    if (n_threads <= 1) {
        for (uint32_t p = 0; p < n_programs && bad.program == 0xFFFFFFFFu; ++p) check_program(p, bad);
    } else {
        std::vector<Bad> found(n_threads);
        std::atomic<uint32_t> next{0};
        std::vector<std::thread> workers;
        for (unsigned t = 0; t < n_threads; ++t)
            workers.emplace_back([&, t]() {
                for (uint32_t p; (p = next.fetch_add(1)) < n_programs;) check_program(p, found[t]);
            });
        for (auto& w : workers) w.join();
        for (const Bad& b : found) if (b.program < bad.program) bad = b;
    }
    if (bad.program != 0xFFFFFFFFu) {
        static const char* const what[] = {"", "slot out of range", "writes a constant slot", "k-mer index out of range", "malformed dense op"};
        return plan_refusal(bad_blob, "program %u op %u: %s", bad.program, bad.op, what[bad.kind]);
    }
    *out = std::move(v);
    return PlanError{};
}

// feedback questions "is slot s of program p all zero?": the program exists, the slot is one of its ordinary slots
inline PlanError check_questions(const BlobView& bv, size_t n_programs, const uint32_t* q_prog, const uint32_t* q_slot, size_t n_q) {
    for (size_t i = 0; i < n_q; ++i) {
        if (q_prog[i] >= n_programs) return plan_refusal(TXQ_ERR_ARG, "feedback query %zu: program out of range", i);
        if (q_slot[i] >= bv.n_slots[q_prog[i]]) return plan_refusal(TXQ_ERR_ARG, "feedback query %zu: slot out of range", i);
    }
    return PlanError{};
}

// ---- the books on the programs' memory --------------------------------------------------------------------------------------
struct ArenaChunk { uint64_t* p; size_t cap; };  // cap in 64-bit words
// A dense block as it is handed on: [cap][W] mask words, then its live list.  state: kGarbage (fresh memory, or left by an
// untracked program), kListed (left by a tracked program: all zero except the entries in its list, which is intact — the
// ZERO that re-creates it for a tracked program clears exactly those, so such a block needs no clearing at all).
struct DenseBlock { uint64_t* p; uint32_t cap; uint8_t state; };
enum : uint8_t { kGarbage = 0, kListed = 1 };
// blocks by capacity: a handful of capacities (powers of two for tracked blocks, A^(k-1) for untracked ones) with thousands
// of blocks each — a vector per capacity (a multimap's node per block made releasing a 10 000-query session 2.5 ms)
struct BlockBins {
    std::vector<std::pair<uint32_t, std::vector<DenseBlock>>> bins;
    std::vector<DenseBlock>& of(uint32_t cap) {
        for (auto& b : bins) if (b.first == cap) return b.second;
        bins.emplace_back(cap, std::vector<DenseBlock>());
        return bins.back().second;
    }
    void put(const DenseBlock& b) { of(b.cap).push_back(b); }
    bool take(uint32_t cap, DenseBlock* out) {
        for (auto& b : bins)
            if (b.first == cap) {
                if (b.second.empty()) return false;
                *out = b.second.back();
                b.second.pop_back();
                return true;
            }
        return false;
    }
    void absorb(BlockBins& other) {  // everything of `other` moves in
        for (auto& b : other.bins) {
            std::vector<DenseBlock>& mine = of(b.first);
            if (mine.empty()) mine.swap(b.second);
            else { mine.insert(mine.end(), b.second.begin(), b.second.end()); b.second.clear(); }
        }
    }
    void swap(BlockBins& o) { bins.swap(o.bins); }
    size_t size() const { size_t n = 0; for (const auto& b : bins) n += b.second.size(); return n; }
    void clear() { bins.clear(); }
};
// What an index keeps of a session's memory for the next one (Index::SessionCache): a single query must not pay
// hipMalloc/hipFree (they cost more than its kernels).
struct BookCache {
    std::vector<ArenaChunk> chunks;  // slot-arena chunks, at most Index::kArenaKeepBytes in all
    // dense blocks live in chunks of their own, and ALL blocks of a session go back into a pool by capacity when it ends:
    // the next batch on this index takes its blocks from there — no allocation, and for tracked programs no clearing
    // (5.3 GB of memset per 200-motif batch at k = 6 before)
    std::vector<ArenaChunk> block_chunks;
    size_t block_cur = 0, block_used = 0;
    BlockBins blocks;
    uint32_t blocks_W = 0;  // the mask width the pooled blocks were laid out for
};

// Chunks of device memory with bump allocation in chunks[cur].  The owner of the list frees the chunks.
struct BumpArena {
    std::vector<ArenaChunk> chunks;
    size_t cur = 0, used = 0, words = 0;  // words: of all chunks
};
// A new chunk of `words` 64-bit words for the slot arena (blocks == false) or the blocks' arena: the pointer, or why not.
using ChunkAlloc = std::function<PlanError(bool blocks, size_t words, uint64_t** out)>;

// The books a session keeps on its programs' memory.  It never allocates, frees or touches device memory itself.
struct SlotBook {
    size_t n_programs = 0;
    BumpArena slots;                // slot regions
    std::vector<uint64_t*> base;    // [2 * n_programs]: per program its slot region [cap][W], then (device address of) its row of the stage's block table
    std::vector<uint32_t> cap;      // per program: slots allocated
    // Dense blocks (include/txq_program.h, version 4): block b of program p is blocks[p][b], an allocation of its own —
    // [N][W] mask words, then the block's live list (tracked programs): count | bitmap of N bits | list of N entries.
    // A program that needs more blocks just gets more (nothing ever moves); kernels find a block through the stage's
    // block table (ordinary ops on dense slots) or through the per-op pointers the host side resolves (DenseOpPtr).
    BumpArena block_mem;            // the blocks' own arena; kept with the index
    BlockBins pool;                 // blocks earlier sessions on this index left behind, by capacity
    std::vector<std::vector<DenseBlock>> blocks;  // per program, by block id (p == nullptr: a tracked block no ZERO has created yet)
    std::vector<uint8_t> tracked;                 // per program: TXQ_PROGRAM_TRACKED_BIT (fixed with its first block)
    BlockBins free_blocks;          // blocks of finished programs by capacity, reusable ...
    // ... two stages after they were given back: the stage before the current one may still be running, on another stream
    std::vector<DenseBlock> given_back[2];
    uint32_t block_slots = 0;       // N = A^(k-1) of this session's blobs (0: no dense blob seen yet): the capacity of untracked blocks
    std::vector<uint32_t> last_stage;  // per program: the last stage (1-based) that had ops for it
    size_t n_blocks_live = 0, n_blocks_made = 0, block_bytes_made = 0, n_blocks_relisted = 0;  // TXQ_TRACE

    void begin(size_t n) {
        n_programs = n;
        base.assign(2 * n, nullptr);
        cap.assign(n, 0);
        blocks.assign(n, {});
        tracked.assign(n, 0);
        last_stage.assign(n, 0);
    }
    // the previous session's memory: the chunks, and the pooled blocks where they fit this session's masks (else the
    // blocks' chunks are reused from their beginning).  Leaves `c` empty.
    void adopt(BookCache& c, uint32_t W) {
        slots.chunks.swap(c.chunks);
        for (const ArenaChunk& k : slots.chunks) slots.words += k.cap;
        block_mem.chunks.swap(c.block_chunks);
        for (const ArenaChunk& k : block_mem.chunks) block_mem.words += k.cap;
        if (c.blocks_W == W) {  // take them over, go on allocating behind them
            pool.swap(c.blocks);
            block_mem.cur = c.block_cur;
            block_mem.used = c.block_used;
        }
        c = BookCache{};
    }
    // Hand the memory back for the next session: the slot chunks up to `keep_bytes` in all; every block this session holds
    // goes into the index's pool (a tracked program's are all zero outside their lists), unless a stage failed (their state
    // is unknown) or slots and blocks together outgrow `keep_bytes`.  Returns the chunks that are not kept: the caller frees them.
    std::vector<ArenaChunk> hand_back(BookCache& c, uint32_t W, bool failed, size_t keep_bytes) {
        std::vector<ArenaChunk> dropped;
        size_t kept = 0;
        for (const ArenaChunk& k : slots.chunks) {
            if (kept + k.cap * 8 <= keep_bytes) { c.chunks.push_back(k); kept += k.cap * 8; }
            else dropped.push_back(k);
        }
        slots.chunks.clear();
        size_t block_bytes = 0;
        for (const ArenaChunk& k : block_mem.chunks) block_bytes += k.cap * 8;
        if (!failed && kept + block_bytes <= keep_bytes) {
            c.block_chunks.swap(block_mem.chunks);
            c.block_cur = block_mem.cur;
            c.block_used = block_mem.used;
            c.blocks_W = W;
            c.blocks.swap(pool);
            for (size_t p = 0; p < blocks.size(); ++p)
                for (const DenseBlock& b : blocks[p])
                    if (b.p) c.blocks.put(DenseBlock{b.p, b.cap, (uint8_t)(tracked[p] ? kListed : kGarbage)});
            c.blocks.absorb(free_blocks);
            for (const std::vector<DenseBlock>& v : given_back)
                for (const DenseBlock& b : v) c.blocks.put(b);
        } else {
            dropped.insert(dropped.end(), block_mem.chunks.begin(), block_mem.chunks.end());
            block_mem.chunks.clear();
        }
        return dropped;
    }

    // does the stage continue a program of the stage before it?  Notes which programs have ops in stage `stage` (1-based).
    bool continues_previous(const BlobView& bv, size_t stage) {
        bool continues = false;
        for (size_t p = 0; p < n_programs; ++p)
            if (bv.programs[p].n_ops) {
                continues = continues || last_stage[p] + 1 == stage;
                last_stage[p] = (uint32_t)stage;
            }
        return continues;
    }

    // Bump allocation of `words` 64-bit words in the slot arena (an even number wherever W is even: 16-byte lanes) or in the
    // blocks' own arena (kept with the index between sessions together with the pool of blocks inside it).  Few, large chunks:
    // as much again as the arena already holds, at least 64 MiB — the slot arena's first chunk: 8 MiB.
    PlanError arena_alloc(bool for_blocks, size_t words, const ChunkAlloc& chunk, uint64_t** out) {
        BumpArena& a = for_blocks ? block_mem : slots;
        while (a.cur < a.chunks.size() && a.used + words > a.chunks[a.cur].cap) { ++a.cur; a.used = 0; }  // adopted chunks
        if (a.cur >= a.chunks.size()) {
            size_t chunk_words = !for_blocks && a.chunks.empty() ? (size_t)1 << 20 : std::max((size_t)8 << 20, a.words);
            if (words > chunk_words) chunk_words = words;
            uint64_t* c = nullptr;
            if (PlanError e = chunk(for_blocks, chunk_words, &c)) return e;
            a.chunks.push_back(ArenaChunk{c, chunk_words});
            a.words += chunk_words;
            a.cur = a.chunks.size() - 1;
            a.used = 0;
        }
        *out = a.chunks[a.cur].p + a.used;
        a.used += words;
        return PlanError{};
    }
    PlanError take_block(uint32_t cap_, uint32_t W, const ChunkAlloc& chunk, DenseBlock* out) {
        for (auto* from : {&free_blocks, &pool})  // given back in this session; left by earlier sessions on this index
            if (from->take(cap_, out)) return PlanError{};
        DenseBlock b{nullptr, cap_, kGarbage};
        if (PlanError e = arena_alloc(true, block_alloc_words(cap_, W), chunk, &b.p)) return e;
        ++n_blocks_made;
        block_bytes_made += block_alloc_words(cap_, W) * 8;
        *out = b;
        return PlanError{};
    }

    // (re)size the programs' slot regions to what the stage needs; a grown region keeps its contents
    // (host side only: the caller uploads `moves` and the base table with the stage and launches move_regions_kernel).
    // Dense blocks: an untracked program gets the blocks it counts (A^(k-1) entries each); a tracked program gets a block
    // when a ZERO of this stage creates it, with the capacity the op names (a block id keeps its capacity).  Blocks come
    // from those that finished programs gave back, or from the arena; `to_clear` = blocks that go to a tracked program and
    // must be all zero first (the caller clears them on the stage's stream).  fresh: programs that got their first region.
    PlanError grow(const BlobView& bv, const unsigned char* blob, uint32_t W, const ChunkAlloc& chunk, std::vector<uint32_t>* fresh,
                   std::vector<RegionMove>* moves_out, std::vector<RegionMove>* to_clear) {
        std::vector<RegionMove>& moves = *moves_out;
        if (bv.block_slots) {
            if (!block_slots) block_slots = bv.block_slots;
            else if (block_slots != bv.block_slots)
                return plan_refusal(TXQ_ERR_PROGRAM, "the block size changed within a session (%u -> %u slots)", block_slots, bv.block_slots);
        }
        // Blocks given back two stages ago serve other programs now: whatever used them has finished (a stage waits for the
        // stage before the previous one, whose staging set it takes over), so a recycled block ties its new owner to nobody.
        for (const DenseBlock& b : given_back[1]) free_blocks.put(b);
        given_back[1].swap(given_back[0]);
        given_back[0].clear();
        // a program that reports no dense blocks any more is finished with them
        if (bv.block_slots)
            for (size_t p = 0; p < n_programs; ++p)
                if (bv.n_blocks[p] == 0 && !blocks[p].empty()) {
                    for (const DenseBlock& b : blocks[p])
                        if (b.p) {
                            given_back[0].push_back(DenseBlock{b.p, b.cap, (uint8_t)(tracked[p] ? kListed : kGarbage)});
                            --n_blocks_live;
                        }
                    blocks[p].clear();
                    base[n_programs + p] = nullptr;
                }
        const txq_op* ops = (const txq_op*)(blob + bv.ops_offset);
        const txq_dense_op* dops = bv.n_dense ? (const txq_dense_op*)(blob + bv.dense_offset) : nullptr;
        for (size_t p = 0; p < n_programs; ++p) {
            // a program gets its region with its first ops (a query of a later wave would otherwise get eight slots now and
            // outgrow them — a move, tied to this stage's init kernel — the moment it begins)
            const uint32_t need = cap[p] || bv.programs[p].n_ops ? bv.n_slots[p] : 0;
            if (need > cap[p]) {
                uint32_t cap_ = cap[p] ? cap[p] * 2 : 8;
                if (cap_ < need) cap_ = need;
                uint64_t* region = nullptr;
                if (PlanError e = arena_alloc(false, (size_t)cap_ * W, chunk, &region)) return e;
                if (cap[p]) moves.push_back(RegionMove{region, base[p], (size_t)cap[p] * W});
                else fresh->push_back((uint32_t)p);
                base[p] = region;
                cap[p] = cap_;
            }
            const size_t bneed = bv.block_slots ? bv.n_blocks[p] : 0;
            if (!bneed) continue;
            if (blocks[p].empty()) tracked[p] = bv.tracked[p];
            else if (tracked[p] != bv.tracked[p]) return plan_refusal(TXQ_ERR_PROGRAM, "program %zu: tracked and untracked blocks in one program", p);
            if (blocks[p].size() < bneed) blocks[p].resize(bneed, DenseBlock{nullptr, 0, kGarbage});
            if (!tracked[p]) {
                for (DenseBlock& b : blocks[p])
                    if (!b.p) {
                        if (PlanError e = take_block(bv.block_slots, W, chunk, &b)) return e;
                        ++n_blocks_live;
                    }
                continue;
            }
            if (!bv.has_dense[p]) continue;
            const DevProgram& d = bv.programs[p];
            for (uint32_t i = 0; i < d.n_ops; ++i) {
                const txq_op& o = ops[d.first_op + i];
                if (o.kmer != TXQ_DENSE_OP || dops[o.dst].kind != TXQ_DENSE_ZERO) continue;
                const txq_dense_op& z = dops[o.dst];
                DenseBlock& b = blocks[p][(z.dst & ~TXQ_DENSE_SLOT_BIT) >> TXQ_DENSE_BLOCK_SHIFT];
                if (b.p) {
                    if (b.cap != z.src) return plan_refusal(TXQ_ERR_PROGRAM, "program %zu: a tracked block changed its capacity (%u -> %u entries)", p, b.cap, z.src);
                    continue;
                }
                if (PlanError e = take_block(z.src, W, chunk, &b)) return e;
                ++n_blocks_live;
                // a block a tracked program left behind is all zero outside its list, and the ZERO that creates the block here
                // clears what is listed (sparse_plan_kernel resets the count, the chunks clear entries and bitmap bits): as it is
                if (b.state == kListed) ++n_blocks_relisted;
                else to_clear->push_back(RegionMove{b.p, nullptr, block_alloc_words(b.cap, W)});
                b.state = kGarbage;  // (what it is while its program runs; tracked[p] decides what it is given back as)
            }
        }
        return PlanError{};
    }

    // a program that is asked about has a region: it has run an op (after grow)
    PlanError check_questions_ran(const uint32_t* q_prog, size_t n_q) const {
        for (size_t i = 0; i < n_q; ++i)
            if (!base[q_prog[i]]) return plan_refusal(TXQ_ERR_ARG, "feedback query %zu: program %u has not run an op yet", i, q_prog[i]);
        return PlanError{};
    }

    // The stage's block table: per program with blocks a row [flags | block 0 | its capacity | block 1 | ..] (flags bit 0:
    // tracked; DenseRow in txq_exec.hip), row_of[p] = where program p's row begins.
    void block_table(std::vector<uint64_t*>* table, std::vector<size_t>* row_of) const {
        row_of->assign(n_programs, 0);
        for (size_t p = 0; p < n_programs; ++p)
            if (!blocks[p].empty()) {
                (*row_of)[p] = table->size();
                table->push_back(reinterpret_cast<uint64_t*>((uintptr_t)(tracked[p] ? 1 : 0)));
                for (const DenseBlock& b : blocks[p]) {
                    table->push_back(b.p);
                    table->push_back(reinterpret_cast<uint64_t*>((uintptr_t)b.cap));
                }
            }
    }
};

// ---- a stage's launches ---------------------------------------------------------------------------------------------------
// Big level-scheduled programs, and every program with dense ops, leave the one-workgroup-per-program kernel:
// their ops are cut into units per dependency level (units of level l, all programs, are contiguous in `units`),
// their dense ops into tiles, and every level becomes one launch of each kind over the whole GPU.
struct LevelPlan {
    size_t units = 0, tiles = 0, hsteps = 0, sparse = 0, sparse_chunks = 0;
    // the level's sparse groups are ordered [others | STEPs]: the first sparse_misc go to the sparse_kernel without step code,
    // the STEPs to the one with it (sparse_chunks counts the others' chunks)
    size_t sparse_misc = 0, step_chunks = 0;
};
// What plan_units makes of a stage's programs: the lists a stage uploads and the launches of its levels.
struct StagePlan {
    std::vector<ExecUnit> units;          // ordinary ops, level by level
    std::vector<TileGroup> tile_groups;   // untracked dense ops; make_tiles_kernel cuts them into n_tiles tiles
    size_t n_tiles = 0;
    std::vector<DenseTile> hsteps;        // HIBF descent: the STEP tiles ...
    std::vector<uint32_t> hstep_na;       // ... and their predecessors per suffix
    std::vector<SparseGroup> sparse_groups;
    std::vector<DenseOpPtr> optr;         // every dense op's blocks, indexed like the stage's dense table
    std::vector<LevelPlan> levels;
    size_t n_small = 0;                   // programs left to exec_kernel
    uint64_t work[4] = {0, 0, 0, 0};      // step pairs, step suffixes, slots zeroed or filled, entries reduced (TXQ_TRACE)
    // chunk_hibf_steps: chunk c = hsteps [chunk_first[c], chunk_first[c + 1]), pair_base[tile] = first pair of the tile within its chunk
    std::vector<uint32_t> pair_base, chunk_pairs;
    std::vector<size_t> chunk_first;
    size_t most_pairs = 0;
};
// hibf: STEP tiles go to their own list (`hsteps`, with the number of predecessors per suffix in `hstep_na`): on an
// HIBF a step is three launches (dense_hibf_*), not a tile of dense_kernel.
// The dense ops of tracked programs become sparse groups (one per op; sparse_kernel), and every dense op's blocks are
// resolved to pointers here (`optr`, indexed like the stage's dense table).
// G_dense: lanes of a workgroup that share one destination suffix; dense_tile_rounds: TXQ_DENSE_TILE_ROUNDS.
inline PlanError plan_units(const SlotBook& s, BlobView& bv, const unsigned char* blob, uint32_t W, uint32_t G_dense, int dense_tile_rounds, bool hibf,
                            StagePlan* out) {
    const uint32_t per_unit = unit_ops(W);
    const uint32_t* levels_host = bv.n_levels ? (const uint32_t*)(blob + bv.levels_offset) : nullptr;
    const txq_op* ops = (const txq_op*)(blob + bv.ops_offset);
    const txq_dense_op* dops = bv.n_dense ? (const txq_dense_op*)(blob + bv.dense_offset) : nullptr;
    out->optr.assign(bv.n_dense, DenseOpPtr{nullptr, nullptr, 0, 0});
    std::vector<std::vector<ExecUnit>> per_level;
    std::vector<std::vector<TileGroup>> groups_level;
    std::vector<std::vector<DenseTile>> hsteps_level;
    std::vector<std::vector<SparseGroup>> sparse_level, step_level;  // (step_level: the STEP groups)
    std::vector<size_t> sparse_chunks, step_chunks;
    // entries per tile: every lane-group set of the workgroup gets two destination suffixes of a step (TXQ_DENSE_TILE_ROUNDS)
    const uint32_t step_tile = (uint32_t)dense_tile_rounds * (256 / (G_dense ? G_dense : 1));
    size_t n_small = 0;
    int bad_program = -1;
    for (size_t p = 0; p < bv.programs.size(); ++p) {
        DevProgram& d = bv.programs[p];
        const bool dense = bv.has_dense[p] != 0;
        // small = less work than a unit launch is worth: 2048 ops of a 1024-bin index, 32 ops at 65536 bins
        if (!dense && (d.n_levels == 0 || (uint64_t)d.n_ops * W < 2048u * 16u)) { n_small += d.n_ops != 0; continue; }
        if (per_level.size() < d.n_levels) {
            per_level.resize(d.n_levels); groups_level.resize(d.n_levels); hsteps_level.resize(d.n_levels);
            sparse_level.resize(d.n_levels); sparse_chunks.resize(d.n_levels, 0);
            step_level.resize(d.n_levels); step_chunks.resize(d.n_levels, 0);
        }
        // (validate_blob has checked that block operands name existing block ids; SlotBook::grow has given the program its
        // blocks — a tracked block exists once a ZERO has created it: an op on one that was never created is refused here)
        auto block_of = [&](uint32_t slot) -> const DenseBlock& {
            const DenseBlock& b = s.blocks[p][(slot & ~TXQ_DENSE_SLOT_BIT) >> TXQ_DENSE_BLOCK_SHIFT];
            if (!b.p) bad_program = (int)p;
            return b;
        };
        auto slot_of = [&](uint32_t slot) -> uint64_t* {
            if (!(slot & TXQ_DENSE_SLOT_BIT)) return s.base[p] + (size_t)slot * W;
            const DenseBlock& b = block_of(slot);
            if ((slot & TXQ_DENSE_INDEX_MASK) >= b.cap) bad_program = (int)p;
            return b.p + (size_t)(slot & TXQ_DENSE_INDEX_MASK) * W;
        };
        const bool check_slots = dense && bv.tracked[p];  // ordinary ops on dense slots of tracked blocks: inside the block's capacity?
        uint32_t begin = 0;
        for (uint32_t l = 0; l < d.n_levels; ++l) {
            const uint32_t end = levels_host[d.first_level + l];
            auto cut = [&](uint32_t from, uint32_t to) {  // a run of ordinary ops -> units
                for (uint32_t at = from; at < to; at += per_unit)
                    per_level[l].push_back(ExecUnit{(uint32_t)p, d.first_op + at, d.first_op + (to - at < per_unit ? to : at + per_unit)});
            };
            if (!dense) cut(begin, end);
            else {
                uint32_t run = begin;
                for (uint32_t i = begin; i < end; ++i) {
                    const txq_op& o = ops[d.first_op + i];
                    if (o.kmer != TXQ_DENSE_OP) {
                        if (check_slots)
                            for (uint32_t operand : {o.dst, o.a, o.b})
                                if (operand & TXQ_DENSE_SLOT_BIT) (void)slot_of(operand);
                        continue;
                    }
                    cut(run, i);
                    run = i + 1;
                    const txq_dense_op& x = dops[o.dst];
                    DenseOpPtr& q = out->optr[o.dst];
                    if (x.kind == TXQ_DENSE_REDUCE) q.dst = slot_of(x.dst);
                    else { const DenseBlock& b = block_of(x.dst); q.dst = b.p; q.dst_cap = b.cap; }
                    if (x.kind == TXQ_DENSE_STEP || x.kind == TXQ_DENSE_REDUCE) { const DenseBlock& b = block_of(x.src); q.src = b.p; q.src_cap = b.cap; }
                    else if (x.kind == TXQ_DENSE_FILL) q.src = slot_of(x.src);
                    uint64_t shape_entries = 1;
                    for (uint32_t j = 0; j < bv.dense.pos; ++j) shape_entries *= (uint64_t)__builtin_popcount(x.shape[j]);
                    if (x.reserved & TXQ_DENSE_TRACKED) {  // work follows the block's live list (FILL: its shape)
                        const bool fixed = x.kind == TXQ_DENSE_FILL;
                        if (fixed && !shape_entries) continue;
                        const bool to_steps = x.kind == TXQ_DENSE_STEP;
                        (to_steps ? step_level : sparse_level)[l].push_back(SparseGroup{o.dst, fixed ? (uint32_t)shape_entries : kNotFixed});
                        // most chunks this group can turn out to have: a list never outgrows its block
                        const uint64_t most = fixed ? shape_entries : x.kind == TXQ_DENSE_ZERO ? q.dst_cap : q.src_cap;
                        (to_steps ? step_chunks : sparse_chunks)[l] += (size_t)((most + kSparseChunk - 1) / kSparseChunk);
                        continue;
                    }
                    uint64_t entries = 1, per_tile = step_tile;
                    if (x.kind == TXQ_DENSE_ZERO || x.kind == TXQ_DENSE_FILL) {
                        per_tile = std::max<uint64_t>(1, 8192 / W);
                        entries = x.kind == TXQ_DENSE_ZERO && !x.r_mask ? bv.block_slots : shape_entries;
                    } else {
                        for (uint32_t j = x.kind == TXQ_DENSE_STEP ? 1 : 0; j < bv.dense.pos; ++j) entries *= (uint64_t)__builtin_popcount(x.shape[j]);
                        if (x.kind == TXQ_DENSE_STEP) entries *= (uint64_t)__builtin_popcount(x.r_mask) * (__builtin_popcount(x.shape[0]) ? 1 : 0);
                        else per_tile = 1024;
                    }
                    if (x.kind == TXQ_DENSE_STEP) { out->work[0] += entries * (uint64_t)__builtin_popcount(x.shape[0]); out->work[1] += entries; }
                    else if (x.kind == TXQ_DENSE_REDUCE) out->work[3] += entries;
                    else out->work[2] += entries;
                    const bool hstep = hibf && x.kind == TXQ_DENSE_STEP;
                    if (hstep) per_tile = 256;  // 256 suffixes x up to 32 predecessors: at most 8192 k-mers per tile
                    if (!hstep) {
                        if (entries) groups_level[l].push_back(TileGroup{(uint32_t)p, o.dst, (uint32_t)entries, (uint32_t)per_tile, 0});
                        continue;
                    }
                    for (uint64_t at = 0; at < entries; at += per_tile)
                        hsteps_level[l].push_back(DenseTile{(uint32_t)p, o.dst, (uint32_t)at, (uint32_t)std::min<uint64_t>(per_tile, entries - at)});
                }
                cut(run, end);
            }
            begin = end;
        }
        d.n_ops = 0;  // the per-program kernel skips it
    }
    if (bad_program >= 0)
        return plan_refusal(TXQ_ERR_PROGRAM, "program %d: an op on a dense block that no ZERO has created, or beyond its capacity", bad_program);
    out->levels.resize(per_level.size());
    for (size_t l = 0; l < per_level.size(); ++l) {
        out->levels[l].units = per_level[l].size();
        size_t level_tiles = 0;
        for (TileGroup& g : groups_level[l]) {
            g.first_tile = out->n_tiles + level_tiles;
            level_tiles += (g.entries + g.per_tile - 1) / g.per_tile;
        }
        out->levels[l].tiles = level_tiles;
        out->n_tiles += level_tiles;
        out->tile_groups.insert(out->tile_groups.end(), groups_level[l].begin(), groups_level[l].end());
        out->levels[l].hsteps = hsteps_level[l].size();
        out->levels[l].sparse = sparse_level[l].size() + step_level[l].size();
        out->levels[l].sparse_misc = sparse_level[l].size();
        out->levels[l].sparse_chunks = sparse_chunks[l];
        out->levels[l].step_chunks = step_chunks[l];
        out->sparse_groups.insert(out->sparse_groups.end(), sparse_level[l].begin(), sparse_level[l].end());
        out->sparse_groups.insert(out->sparse_groups.end(), step_level[l].begin(), step_level[l].end());
        out->units.insert(out->units.end(), per_level[l].begin(), per_level[l].end());
        for (const DenseTile& t : hsteps_level[l]) {
            out->hsteps.push_back(t);
            out->hstep_na.push_back((uint32_t)__builtin_popcount(dops[t.op].shape[0]));
        }
    }
    out->n_small = n_small;
    return PlanError{};
}

// HIBF steps run in chunks of tiles whose masks fit the scratch (2 GiB), never across a level.
inline void chunk_hibf_steps(StagePlan& plan, uint32_t W) {
    plan.pair_base.assign(plan.hsteps.size(), 0);
    const uint64_t budget = std::max<uint64_t>(((uint64_t)2 << 30) / ((uint64_t)W * 8), 8192);
    size_t at = 0;
    for (const LevelPlan& lp : plan.levels) {
        uint64_t pairs = 0;
        for (size_t i = 0; i < lp.hsteps; ++i, ++at) {
            const uint64_t mine = (uint64_t)plan.hsteps[at].count * plan.hstep_na[at];
            if (i == 0 || pairs + mine > budget) {
                plan.chunk_first.push_back(at);
                plan.chunk_pairs.push_back(0);
                pairs = 0;
            }
            plan.pair_base[at] = (uint32_t)pairs;
            pairs += mine;
            plan.chunk_pairs.back() = (uint32_t)pairs;
        }
    }
    for (uint32_t c : plan.chunk_pairs) plan.most_pairs = std::max<size_t>(plan.most_pairs, c);
    plan.chunk_first.push_back(plan.hsteps.size());
}

}  // namespace txq
