// The records libtxq.so keeps in HBM for an index, as plain C++: no HIP here, so that the host code which fills them
// (txq_hibf_plan.hpp; a stage's records: txq_exec_plan.hpp) compiles and is tested without a GPU.  The kernels read them through txq_kernels.hpp.
#pragma once
#include <stdint.h>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

// accessors that kernels call too
#if defined(__HIPCC__)
#define TXQ_HOST_DEVICE __host__ __device__
#else
#define TXQ_HOST_DEVICE
#endif

namespace txq {

// why the host-side planning of an upload or a stage was refused (txq_hibf_plan.hpp, txq_exec_plan.hpp): handed to
// fail(code, "%s", text)
struct PlanError {
    int code = 0;  // TXQ_OK
    std::string text;
    enum Kind { kNone, kOther, kBadChild, kTwoParents } kind = kNone;  // (the sub-tree entry point words two of them its own way)
    uint64_t ibf = 0;                                                  // kBadChild / kTwoParents: the child
    explicit operator bool() const { return code != 0; }
};
inline PlanError plan_refusal(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return PlanError{code, buf, PlanError::kOther, 0};
}

struct IbfDev {
    uint64_t* words;      // device pointer, [bin_size][stride]
    uint64_t bin_size;    // rows
    uint32_t hash_shift;  // countl_zero(bin_size)
    uint32_t hash_funs;   // 1..5
    uint32_t stride;      // words per row in HBM
    uint32_t shard_words; // mask words this shard owns (<= stride)
    uint32_t word0;       // first full-mask word owned by this shard
    uint32_t bins;        // technical bins in use (unsharded)
    // HIBF leaves whose technical bin b is user bin 64*ident_word + b (no merged bins): a hit word
    // of the row IS a word of the result mask.  ident_word == kNoIdent otherwise.
    uint32_t ident_word;
    uint32_t reserved;
};
static constexpr uint32_t kNoIdent = 0xFFFFFFFFu;

// stride (bits 0-19) | hash_shift (20-25) | hash_funs (26-28) of an IBF, as HibfNode::packed and VChunk::packed begin
// (bits 29 and 30 are the record's own flags)
inline uint32_t pack_ibf_params(const IbfDev& f) { return f.stride | (f.hash_shift << 20) | (f.hash_funs << 26); }

// Everything about one IBF of an HIBF tree in one 32-byte record (txq_hibf.hip: nodes[e] = the child behind merged
// technical bin e; the dense steps on a regular tree take the root as a kernel argument).
struct HibfNode {  // 32 bytes = two 16-byte loads per lane
    uint64_t words;       // device pointer to the IBF's rows
    uint32_t bin_size;    // rows (< 2^32: the fused kernel is not used for larger IBFs)
    uint32_t packed;      // stride (bits 0-19) | hash_shift (20-25) | hash_funs (26-28) | has merged bins (29)
    uint32_t off;         // first entry of the IBF's technical bins in the flattened maps
    uint32_t moff;        // first word of the IBF in `merged` / `descend`
    uint32_t ident_word;  // see IbfDev::ident_word
    uint32_t bins;        // technical bins
    TXQ_HOST_DEVICE uint32_t stride() const { return packed & 0xFFFFFu; }
    TXQ_HOST_DEVICE uint32_t hash_shift() const { return (packed >> 20) & 63u; }
    TXQ_HOST_DEVICE uint32_t hash_funs() const { return (packed >> 26) & 7u; }
    TXQ_HOST_DEVICE bool has_merged() const { return (packed >> 29) & 1u; }
    TXQ_HOST_DEVICE uint32_t words_per_row() const { return (bins + 63u) >> 6; }
};
static_assert(sizeof(HibfNode) == 32, "two 16-byte pieces per node");
static constexpr uint32_t kRootEntry = 0xFFFFFFFFu;  // stack entry of the root IBF (every other entry is a technical-bin index)

// Regular two-level trees: one record per child in mask-column order (child-stationary descent in txq_hibf.hip, dense
// steps on the tree in txq_exec.hip).
struct ChildRec {   // 16 bytes, one per child in mask-column order
    uint64_t words;     // device pointer to the child's rows (stride = row words, a power of two >= 2)
    uint32_t bin_size;  // rows
    uint32_t packed;    // hash_shift (bits 0-7) | hash_funs (8-11) | root technical bin (12-31)
};
static_assert(sizeof(ChildRec) == 16, "one 16-byte load per lane");

// General HIBFs in LAYOUT ORDER (sessions on trees that are not regular: three and more levels, user bins next to merged
// bins, split bins, user bins in any order — what seqan::hibf's layout produces, reference include/index_hibf.h:114-129).
// A session on such a tree does not work on masks in user-bin order but on rows in the order of the tree's own
// technical bins: the row of every IBF, one after the other (levels ascending, every IBF padded to an even number of
// words), W_v words in all.  In that order every IBF owns an aligned segment of the row, so a k-mer's mask is written
// segment by segment with coalesced stores and no atomics (child-stationary, level by level), and a dense step gathers a
// lane's 16 bytes from ONE IBF.  Every operation of the collector is bin-wise, so the order of the bins does not matter
// until the final masks are handed out: those are converted to user-bin order (split bins ORed) once per query.
// Merged bins keep their bits in the rows (the next level reads them as its gates); they never reach a result because
// the ONES slot of a layout-order session only has the bits of technical bins that ARE user bins.
struct VChunk {          // one chunk of the layout-order row: two row words (16 bytes) of one IBF, or one (Index::v_chunk_words)
    uint64_t words;      // the IBF's rows
    uint32_t bin_size;   // rows (< 2^32)
    uint32_t packed;     // stride (bits 0-19) | hash_shift (20-25) | hash_funs (26-28) | single-word rows (29) | holds representatives of split user bins (30)
    uint32_t col;        // word column of the chunk within the IBF's row
    uint32_t gate_word;  // layout-order word that holds the parent's merged bin leading here (kNoGate: the root)
    uint32_t gate_bit;
    uint32_t ibf;        // IBF id (its VPath)
};
static_assert(sizeof(VChunk) == 32, "two 16-byte loads per lane");
static constexpr uint32_t kNoGate = 0xFFFFFFFFu;
static constexpr uint32_t kMaxVDepth = 3;  // ancestors a fused dense step follows (trees of up to 4 levels)
struct VPath {           // the ancestors of an IBF, root first: whose merged bin (row word, bit) leads towards it
    uint32_t depth, pad;
    struct { uint64_t words; uint32_t bin_size, packed, word, bit; } anc[kMaxVDepth];
};
// Split user bins in layout order.  A user bin that the layout spreads over several technical bins of one IBF holds a k-mer when
// ANY of its parts does, and masks are combined per USER bin (reference include/index_hibf.h:132-147 ORs the parts before the
// collector ANDs anything) — so in a layout-order row a split bin is ONE bit, its first part's (the representative), which
// stands for the OR of the parts; the other parts' bits are always zero.  Rows of plain k-mers are put into that form as they
// are written (hibf_fused_kernel<G, LAYOUT>) or right after (unify_split_rows_kernel behind the level kernels).  A fused step
// (PathRows) works on one 16-byte chunk of an IBF's row and does not see the other parts: for them every IBF with split bins has
// a SIDE matrix — the columns of its non-representative parts once more, packed so that the parts belonging to one chunk's
// representatives are consecutive bits of one 64-bit word per row.  ANDing the k-mer's h side rows gives those parts' hits
// exactly (they are the IBF's own columns), and a hit sets its representative: VSplit entry e of the chunk (sorted by
// representative) is side bit `bit0 + e`.
struct VSplit { uint32_t part_word; uint16_t rep_bit, part_bit; };  // word column and bit of the part in the IBF's row; its representative's bit in the chunk
struct VSplitRange {
    uint32_t first, count;   // the chunk's entries in Index::d_vsplits (any number: every part of a split bin whose representative is in the chunk)
    uint32_t reps[4];        // the chunk's bits that are representatives (bit b of the 128: reps[b >> 5] >> (b & 31))
    uint64_t side;           // device pointer: row 0 of the chunk's (first) word in the IBF's side matrix — entry e is bit bit0 + e from there
    uint32_t side_stride;    // words per side row
    uint32_t bit0;           // the chunk's first bit in that word
};
struct VLevel { uint32_t first_chunk, n_chunks; std::vector<uint32_t> group_first; };  // groups: chunk ranges whose IBFs share an L2's worth of rows

// A technical bin of a sub-tree shard's root whose column was cleared because another shard owns it (txq_index_upload_subtrees):
// internal only, accepted by read_tree with `cleared_ok`; it is no user bin and no merged bin, and it never fires.
static constexpr uint64_t kClearedBin = 0xFFFFFFFFFFFFFFFEull;

}  // namespace txq
