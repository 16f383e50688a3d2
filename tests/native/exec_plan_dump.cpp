// Everything a stage of a session plans on the host (tetrex_amd/csrc/txq_exec_plan.hpp), printed by name: a script of sessions
// comes in on stdin, and for every stage either its refusal ("rc", "error") or everything the stage would upload goes out as
// "name value" (arrays: byte count and hex); tests/test_exec_plan.py compares them with tests/golden/exec_plan_expected.json.
// No GPU: chunk i of the slot arena "lives" at address (i + 1) << 40, chunk i of the blocks' arena at (0x100 + i + 1) << 40,
// counted over the whole script — which is what every planned pointer then contains.
//   input:  n_sessions, then per session:  W  G_dense  dense_tile_rounds  hibf  n_programs  n_stages
//           per stage:  blob_bytes  blob as hex ("-" for none, "@path" for a file's bytes)  n_questions  [program slot] x n_questions
//   The sessions run one after the other on ONE index: each adopts what the one before it handed back (its chunks, and its
//   pool of blocks where the mask width is the same), as session_begin and ~Session do.  A refused stage ends its session.
//   output: names are prefixed "s<session>.t<stage>.", a session's adoption and hand-back "s<session>.begin." / ".end."
#include "../../tetrex_amd/csrc/txq_exec_plan.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace txq;

// ---- made-up device memory
static uint64_t g_chunks_made[2] = {0, 0};
static PlanError made_up_chunk(bool blocks, size_t, uint64_t** out) {
    *out = (uint64_t*)(uintptr_t)(((blocks ? 0x100ull : 0ull) + ++g_chunks_made[blocks ? 1 : 0]) << 40);
    return PlanError{};
}
static const size_t kKeepBytes = (size_t)64 << 30;  // Index::kArenaKeepBytes

// ---- a session, the device left out: what session_begin, the phases of session_stage and ~Session do with the book
struct StageOut {
    BlobView bv;
    bool continues = false;
    std::vector<uint32_t> fresh;
    std::vector<RegionMove> moves, clears;
    StagePlan plan;
    std::vector<uint64_t*> block_table;
    std::vector<size_t> row_of;
};
struct Run {
    SlotBook book;
    uint32_t W = 0, G_dense = 1;
    int rounds = 4;
    bool hibf = false;
    size_t n_stages = 0;
    void begin(BookCache& cache, size_t n_programs) {
        book.begin(n_programs);
        book.adopt(cache, W);
    }
    // stage_decide, stage_regions, stage_plan: everything is refused before a region is grown
    PlanError stage(const unsigned char* blob, size_t bytes, const uint32_t* q_prog, const uint32_t* q_slot, size_t n_q, StageOut* o) {
        if (PlanError e = validate_blob(blob, bytes, book.n_programs, &o->bv)) return e;
        ++n_stages;
        if (PlanError e = check_questions(o->bv, book.n_programs, q_prog, q_slot, n_q)) return e;
        o->continues = book.continues_previous(o->bv, n_stages);
        if (PlanError e = book.grow(o->bv, blob, W, made_up_chunk, &o->fresh, &o->moves, &o->clears)) return e;
        if (PlanError e = book.check_questions_ran(q_prog, n_q)) return e;
        if (PlanError e = plan_units(book, o->bv, blob, W, G_dense, rounds, hibf, &o->plan)) return e;
        book.block_table(&o->block_table, &o->row_of);
        chunk_hibf_steps(o->plan, W);
        return PlanError{};
    }
    std::vector<ArenaChunk> end(BookCache& cache) { return book.hand_back(cache, W, false, kKeepBytes); }
    std::vector<uint64_t*> bases() const { return std::vector<uint64_t*>(book.base.begin(), book.base.begin() + book.n_programs); }
    std::vector<uint64_t> counters() const { return {book.n_blocks_live, book.n_blocks_made, book.block_bytes_made, book.n_blocks_relisted}; }
    std::vector<uint64_t> arenas() const {
        return {book.slots.chunks.size(), book.slots.cur, book.slots.used, book.slots.words, book.block_mem.chunks.size(), book.block_mem.cur, book.block_mem.used,
                book.block_mem.words, book.block_slots};
    }
    const BlockBins& pool() const { return book.pool; }
};

// ---- reading the script, printing by name
static std::string g_prefix;
static void scalar(const char* name, uint64_t v) { printf("%s%s %" PRIu64 "\n", g_prefix.c_str(), name, v); }
static void bytes(const char* name, const void* p, size_t n) {
    printf("%s%s %zu ", g_prefix.c_str(), name, n);
    for (size_t i = 0; i < n; ++i) printf("%02x", ((const unsigned char*)p)[i]);
    printf("\n");
}
template <class T>
static void array(const char* name, const std::vector<T>& v) { bytes(name, v.data(), v.size() * sizeof(T)); }
static void pool_blocks(const char* name, const BlockBins& b) {  // (address, capacity, state) of every block, as the bins hold them
    std::vector<uint64_t> flat;
    for (const auto& bin : b.bins)
        for (const DenseBlock& x : bin.second) flat.insert(flat.end(), {(uint64_t)(uintptr_t)x.p, x.cap, x.state});
    array(name, flat);
}
static uint64_t number() {
    unsigned long long v = 0;
    if (scanf("%llu", &v) != 1) { fprintf(stderr, "exec_plan_dump: short input\n"); exit(2); }
    return v;
}
static int nibble(int c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

static void print_stage(const Run& run, const StageOut& o) {
    const BlobView& bv = o.bv;
    const StagePlan& P = o.plan;
    scalar("rc", 0);
    scalar("n_kmers", bv.n_kmers);
    scalar("n_ops", bv.n_ops);
    scalar("n_levels", bv.n_levels);
    scalar("n_dense", bv.n_dense);
    scalar("n_aux_kmers", bv.n_aux_kmers);
    scalar("block_slots", bv.block_slots);
    bytes("dense_params", &bv.dense, sizeof bv.dense);
    array("programs", bv.programs);  // normalised, as uploaded: what plan_units took is left to no op of exec_kernel
    array("n_slots", bv.n_slots);
    array("n_blocks", bv.n_blocks);
    array("has_dense", bv.has_dense);
    array("tracked", bv.tracked);
    scalar("continues", o.continues);
    array("fresh", o.fresh);
    array("moves", o.moves);
    array("clears", o.clears);
    array("base", run.bases());
    array("block_table", o.block_table);
    array("row_of", o.row_of);
    array("units", P.units);
    array("tile_groups", P.tile_groups);
    scalar("n_tiles", P.n_tiles);
    array("hsteps", P.hsteps);
    array("hstep_na", P.hstep_na);
    array("sparse_groups", P.sparse_groups);
    array("optr", P.optr);
    array("levels", P.levels);  // per level: units, tiles, hsteps, sparse, sparse_chunks, sparse_misc, step_chunks
    scalar("n_small", P.n_small);
    bytes("work", P.work, sizeof P.work);
    array("pair_base", P.pair_base);
    array("chunk_pairs", P.chunk_pairs);
    array("chunk_first", P.chunk_first);
    scalar("most_pairs", P.most_pairs);
    array("counters", run.counters());  // n_blocks_live, n_blocks_made, block_bytes_made, n_blocks_relisted
    array("arenas", run.arenas());      // per arena: chunks, cur, used, words; then block_slots
}

int main() {
    static_assert(sizeof(LevelPlan) == 7 * sizeof(size_t) && sizeof(DenseOpPtr) == 24 && sizeof(TileGroup) == 24 && sizeof(RegionMove) == 24 &&
                      sizeof(DenseParams) == 18 * 4,
                  "the records are printed as their bytes: no padding");
    BookCache cache;  // the index's
    const size_t n_sessions = number();
    for (size_t si = 0; si < n_sessions; ++si) {
        Run run;
        run.W = (uint32_t)number();
        run.G_dense = (uint32_t)number();
        run.rounds = (int)number();
        run.hibf = number() != 0;
        const size_t n_programs = number(), n_stages = number();
        g_prefix = "s" + std::to_string(si) + ".begin.";
        scalar("cached_blocks", cache.blocks.size());
        scalar("cached_W", cache.blocks_W);
        run.begin(cache, n_programs);
        scalar("pool", run.pool().size());
        array("arenas", run.arenas());
        bool refused = false;
        for (size_t ti = 0; ti < n_stages; ++ti) {
            const size_t n_bytes = number();
            std::vector<uint64_t> blob((n_bytes + 7) / 8 + 1, 0);  // (8-byte aligned, as txq_session_stage asks)
            unsigned char* b = (unsigned char*)blob.data();
            int c;
            while ((c = getchar()) == ' ' || c == '\n') {}
            if (c == '@') {  // the blob's bytes lie in a file (a stage too large to spell out)
                char path[4096];
                if (scanf("%4095s", path) != 1) return 2;
                FILE* f = fopen(path, "rb");
                if (!f || fread(b, 1, n_bytes, f) != n_bytes) { fprintf(stderr, "exec_plan_dump: cannot read %s\n", path); return 2; }
                fclose(f);
            } else if (c != '-')
                for (size_t i = 0; i < n_bytes; ++i, c = getchar()) { const int lo = getchar(); b[i] = (unsigned char)(nibble(c) << 4 | nibble(lo)); }
            std::vector<uint32_t> q_prog, q_slot;
            for (size_t n_q = number(); n_q; --n_q) { q_prog.push_back((uint32_t)number()); q_slot.push_back((uint32_t)number()); }
            if (refused) continue;  // (read, not run)
            g_prefix = "s" + std::to_string(si) + ".t" + std::to_string(ti) + ".";
            StageOut o;
            if (PlanError e = run.stage(b, n_bytes, q_prog.data(), q_slot.data(), q_prog.size(), &o)) {
                printf("%src %d\n%serror %s\n", g_prefix.c_str(), e.code, g_prefix.c_str(), e.text.c_str());
                refused = true;
                continue;
            }
            print_stage(run, o);
        }
        g_prefix = "s" + std::to_string(si) + ".end.";
        const std::vector<ArenaChunk> dropped = run.end(cache);
        scalar("dropped_chunks", dropped.size());
        scalar("kept_slot_chunks", cache.chunks.size());
        scalar("kept_block_chunks", cache.block_chunks.size());
        scalar("block_cur", cache.block_cur);
        scalar("block_used", cache.block_used);
        scalar("blocks_W", cache.blocks_W);
        pool_blocks("pool", cache.blocks);
    }
    return 0;
}
