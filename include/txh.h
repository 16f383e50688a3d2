/* txh.h — C view of the C++ host front-end (libtetrex_host.so): regex -> postfix -> k-graph ->
 * mask-DAG programs, k-mer encoders, .ibf codec.  It exists so that tests (and foreign-language
 * callers) can drive the host stages one by one; the `tetrex` CLI links the same C++ directly.
 * Reference interfaces mirrored: translate() src/utils.cpp:3-15; preprocess_query()
 * include/query.h:80-94; construct_kgraph()/construct_reduced_kgraph() src/construct_nfa.cpp:265,
 * src/construct_reduced_nfa.cpp:313; OTFCollector::collect() include/otf_collector.h:341-393;
 * MoleculeDecomposer::decompose_record() include/molecule_decomposer.h:92-96;
 * load_ibf()/store_ibf() include/index_base.h:181-195.
 * All functions return 0 / a non-negative count on success and a negative value on error
 * (message via txh_last_error()). */
#ifndef TXH_H
#define TXH_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

const char* txh_last_error(void);

/* string outputs: returns the length written (excluding NUL) or <0 */
int txh_translate(const char* regex, char* out, size_t cap);
int txh_preprocess(const char* regex, int dna, unsigned k, unsigned reduction, char* preprocessed, size_t cap1,
                   char* postfix, size_t cap2);

/* k-graph of a postfix string: labels[n], next_a[n], next_b[n]; returns n or <0 */
int txh_kgraph(const char* postfix, unsigned k, int reduced, int32_t* labels, int32_t* next_a, int32_t* next_b,
               int32_t cap);

/* The k-graph the EXPANSION works on (base alphabet, no -a): unions of single residues — `.`, `[LIVM]`, `(A|G)` — are one
 * node each (label >= 260) instead of the reference's Split / Ghost tree over one node per residue; it accepts the same
 * strings.  members: per node one line — the residues it stands for, in the query's order (empty for Ghost / Split / Match
 * nodes).  Returns n or <0.  (tetrex_amd/csrc/host/kgraph.hpp KGraph::kClass; TETREX_FUSE_CLASSES=0 switches fusing off.) */
int txh_kgraph_fused(const char* postfix, unsigned k, int32_t* labels, int32_t* next_a, int32_t* next_b, int32_t cap,
                     char* members, size_t members_cap);

/* Graphviz text of the k-graph (`tetrex query -d`); augment != 0 applies -a first */
int txh_kgraph_dot(const char* postfix, unsigned k, int reduced, int augment, char* out, size_t cap);

/* Compile a batch of queries for an index with `bins` bins into one program blob.
 * status[i] receives 0 or a negative code for query i (a failed query becomes an empty program
 * whose result mask is zero); the blob is owned by the library until txh_blob_free. */
typedef struct txh_blob txh_blob;
int txh_compile_batch(const char* const* regex, size_t n, int dna, unsigned k, unsigned reduction, uint64_t bins,
                      txh_blob** out, int* status);
const void* txh_blob_data(const txh_blob* b, size_t* bytes);
/* stats4[i*4..]: ops, slots, states, probe ops of query i */
int txh_blob_stats(const txh_blob* b, uint64_t* stats4, size_t n);
void txh_blob_free(txh_blob* b);

/* Staged expansion against a caller-supplied executor (the GPU session in production, a
 * simulator in CPU tests).  `fn` runs one stage: blob = the NEW ops of all n programs
 * (txq_program.h format), and must fill alive[i] for the n_q feedback questions
 * (program qp[i], slot qs[i]); it returns 0 on success.  stats6 (8 entries): stages, ops,
 * kmers, states, pruned states, feedback questions, host expansion us, stage execution us. */
/* -a / -g of `tetrex query` (reference include/arg_parse.h:64,68) */
typedef struct {
    int augment;       /* bypass catastrophic sub-graphs with Gap nodes */
    int dgram_loaded;  /* a d-gram index is attached: probe across gaps */
    uint64_t min_gap, max_gap;
} txh_gap_options;

typedef int (*txh_stage_fn)(void* user, const void* blob, size_t bytes, const uint32_t* qp, const uint32_t* qs, size_t n_q,
                            uint8_t* alive);
int txh_run_staged(const char* const* regex, size_t n, int dna, unsigned k, unsigned reduction, uint64_t bins,
                   size_t ops_per_query_per_stage, size_t ops_per_stage, const txh_gap_options* gaps, txh_stage_fn fn,
                   void* user, int* status, uint64_t* stats6);
/* The same with dense DP steps switched on (include/txq_program.h version 3): the executor then receives
 * version-3 blobs.  min_states / sparse_below: 0 = the product's defaults; slot_bytes: bytes of one mask. */
typedef struct {
    int enabled;
    uint32_t min_states, sparse_below, max_blocks;
    uint64_t slot_bytes, pool_bytes;
    int tracked; /* 0: the executor keeps no live lists; 1: it does (queries use tracked blocks where the run learns that
                    states thin out on the index); 2: every query uses tracked blocks */
} txh_dense_options;
int txh_run_staged_dense(const char* const* regex, size_t n, int dna, unsigned k, unsigned reduction, uint64_t bins,
                         size_t ops_per_query_per_stage, size_t ops_per_stage, const txh_gap_options* gaps,
                         const txh_dense_options* dense, txh_stage_fn fn, void* user, int* status, uint64_t* stats6);
/* Join of column shards (host/compiler.hpp join_shard_masks): shard r holds words [word0[r], word0[r] + words[r]) of
 * each of the n masks; out receives n x mask_words words.  <0 when the shards do not tile the mask exactly. */
int txh_join_shard_masks(size_t n, uint64_t mask_words, size_t n_shards, const uint64_t* word0, const uint64_t* words,
                         const uint64_t* const* shard_masks, uint64_t* out);
/* the d-gram codes one record contributes (DGramIndex::process_sequence, include/dGramIndex.h:159-211) */
int64_t txh_dgram_values(const char* seq, size_t len, uint64_t min_gap, uint64_t max_gap, uint64_t* out, size_t cap);

/* End-to-end candidate masks on an index that already lives on the GPU (a txq_index* from
 * include/txq.h, passed as void* so this header stays free of txq types): host expansion +
 * staged device execution.  masks: n x shard_words words.  stats6 (8 entries) as in txh_run_staged.
 * Exported by libtetrex_query.so (which links libtxq.so), not by libtetrex_host.so. */
int txe_query_masks(void* txq_index_handle, int dna, unsigned k, unsigned reduction, const char* const* regex, size_t n,
                    size_t ops_per_query_per_stage, uint64_t* masks, int* status, uint64_t* stats6);
/* The same for motifs given the way `tetrex query` receives a batch — one text, one motif per line (the reference's motif file,
 * src/query.cpp:318-327, without the name column): text[0, text_bytes) holds n lines separated by '\n' (a final '\n' is optional).
 * For bindings whose strings are not C strings: no array of n pointers to build (6 ms per 10 000 motifs from Python). */
int txe_query_masks_text(void* txq_index_handle, int dna, unsigned k, unsigned reduction, const char* text, size_t text_bytes, size_t n,
                         size_t ops_per_query_per_stage, uint64_t* masks, int* status, uint64_t* stats6);
/* the same with -a/-g: aux_index_handle is the GPU-resident d-gram index (or NULL) */
int txe_query_masks_gapped(void* txq_index_handle, void* aux_index_handle, const txh_gap_options* gaps, int dna, unsigned k,
                           unsigned reduction, const char* const* regex, size_t n, size_t ops_per_query_per_stage,
                           uint64_t* masks, int* status, uint64_t* stats6);
/* The same on an index that is column-sharded over several GPUs (or several shards on one GPU): handles[r] is shard r
 * of n_shards as uploaded with txq_index_upload(desc, r, n_shards, ..).  ONE frontier expansion feeds all shards (the
 * ops are shard-independent), every stage runs on all shards at the same time, a state is pruned when it is dead in
 * every shard, and the final masks are joined: masks receives n x mask_words words (the FULL mask).  aux_handles (or NULL):
 * the d-gram index, sharded the same way. */
int txe_query_masks_sharded(void* const* handles, void* const* aux_handles, size_t n_shards, const txh_gap_options* gaps, int dna,
                            unsigned k, unsigned reduction, const char* const* regex, size_t n, size_t ops_per_query_per_stage,
                            uint64_t* masks, int* status, uint64_t* stats6);
const char* txe_last_error(void);
/* dense DP ops (include/txq_program.h version 3) the calling thread's last txe_query_masks* run sent to the device */
uint64_t txe_last_dense_ops(void);
/* queries of that run whose blocks carried live lists (tracked programs, include/txq_program.h) */
uint64_t txe_last_tracked_queries(void);

/* The verification matcher (host/matcher.hpp; stands where the reference has RE2, include/query.h:103,148): successive
 * non-overlapping matches of `pattern` in text[0..len), the RE2::FindAndConsume loop of src/query.cpp:206-216.
 * posix != 0: leftmost-longest (RE2::POSIX, peptides); 0: leftmost-first (RE2 default, DNA).  out receives (start, length)
 * pairs; returns the number of matches (may exceed cap / 2 pairs; nothing written past cap), <0 on a syntax error. */
int64_t txh_regex_find_all(const char* pattern, int posix, const char* text, size_t len, uint64_t* out, size_t cap);
/* The matcher's prefilter: the longest run of plain bytes that every match of the pattern contains (memmem in front of the
 * automata; may be empty).  Writes at most `cap` bytes, returns the literal's length, < 0 on a syntax error. */
int64_t txh_regex_required_literal(const char* pattern, int posix, char* out, size_t cap);

/* The pattern as a flat automaton (include/txq_regex.h, where the layout and the semantics are; Matcher::export_dfa): what the
 * record filter of `tetrex query --gpu-verify` runs.  strand 0: the automaton accepts a record exactly when
 * txh_regex_find_all reports a match in it.  strand 1: built from the reversed pattern — it accepts T exactly when the
 * pattern matches reverse(T); with the nucleotide complement as byte_map that is a match on T's reverse complement, found by
 * scanning T forward.  byte_map (256 bytes, or NULL for the identity) is applied to a text byte before the pattern sees it
 * and is folded into the automaton's class table.  Returns the blob's bytes (nothing is written where they exceed cap),
 * 0 where the automaton has more than 65 535 states ("too large": determinisation stops there), < 0 on a syntax error. */
int64_t txh_regex_automaton(const char* pattern, int posix, int strand, const uint8_t* byte_map, uint8_t* out, size_t cap);
/* the byte -> letter table of a peptide reduction (0 none, 1 murphy, 2 li): what verification applies to a bin's text on a
 * reduced index before matching, and what txh_regex_automaton takes as byte_map there */
int txh_reduce_table(unsigned reduction, uint8_t out[256]);
/* The host twin of txq_regex_filter_device (include/txq.h, where the arguments are described), on the inline interpreter
 * of include/txq_regex.h: bit r - group start of the bitmap at out[out_offsets[i]] is set iff the automaton of pair i matches
 * record r; out[0 .. out_words) is zeroed first; status[i] = 0, or 0xFFFFFFFE for a pair that names an automaton or a group
 * out of range, offsets that leave their arrays or a malformed blob (such a pair sets no bit).  max_serial: 0, or
 * TXQ_REGEX_MAX_SERIAL — a record longer than that is flagged without being scanned where the automaton is unbounded, as
 * the device does it.  Returns 0, or a negative number for null pointers. */
int txh_regex_filter(const uint8_t* automata, const uint64_t* auto_offsets, size_t n_automata, size_t automata_bytes, const uint8_t* text,
                     const uint64_t* rec_offsets, size_t n_records, size_t text_bytes, const uint64_t* group_offsets, size_t n_groups,
                     const uint32_t* pairs, size_t n_pairs, const uint64_t* out_offsets, uint32_t* out, size_t out_words, uint64_t max_serial,
                     uint32_t* status);

/* values inserted for one record; returns the count (may exceed cap; nothing written past cap) */
int64_t txh_record_values(int dna, unsigned k, unsigned reduction, const char* seq, size_t len, int wraparound,
                          uint64_t* out, size_t cap);

/* Six-frame translation of one nucleotide record into the k-mer values of a peptide index (the CPU restatement of
 * txq_translate_device, include/txq.h, where the semantics are spelled out): frames +1 +2 +3 -1 -2 -3 one after the other,
 * offsets[f] .. offsets[f+1] the values of frame f.  Returns the number of values (may exceed cap; nothing written past cap),
 * or a negative number where k is outside 1..12 or the reduction unknown. */
int64_t txh_translated_values(unsigned k, unsigned reduction, const char* seq, size_t len, uint64_t* out, size_t cap,
                              uint64_t offsets[7]);
/* one frame (0..5) as residue letters, X for an ambiguous codon and * for a stop; returns the length (may exceed cap) */
int64_t txh_translate_frame(const char* seq, size_t len, unsigned frame, char* out, size_t cap);
/* the 256-byte residue code table of the peptide encoder of a reduction (what txq_translate takes as `codes`) */
int txh_peptide_codes(unsigned reduction, uint8_t out[256]);

/* Approximate matching by edit distance on the host (host/edit_distance.hpp): the semantics of txq_edit_search
 * (include/txq.h, where they are spelled out: class table, Sellers' recurrence, the (distance, record, end) of a pair or
 * three times 0xFFFFFFFF above the cap) with NO limit on the pattern length.  The CPU twin of the kernel: `tetrex search
 * --verify` answers patterns longer than TXQ_EDIT_MAX_PATTERN with it, and the kernel is measured against it.  Pattern p is
 * patterns[pat_offsets[p] .. pat_offsets[p+1]), record r is text[rec_offsets[r] .. rec_offsets[r+1]), group g is records
 * group_offsets[g] .. group_offsets[g+1] - 1; pairs: 3 u32 each (pattern, group, cap); out: 3 u32 each; the pairs are
 * dealt over `threads` threads (0: one).  Returns 0, or a negative number (offsets not ascending, a pair out of range, an
 * empty pattern, null pointers). */
int txh_edit_search(const uint8_t* patterns, const uint64_t* pat_offsets, size_t n_patterns, const uint8_t* text, const uint64_t* rec_offsets,
                    size_t n_records, const uint64_t* group_offsets, size_t n_groups, const uint32_t* pairs, size_t n_pairs,
                    const uint8_t* codes, unsigned threads, uint32_t* out);
/* Every record of a group that a pattern matches within its cap, on the host (host/edit_distance.hpp): the semantics of
 * txq_edit_targets_device (include/txq.h: a hit is (pair, d, r, j) for every record r of the pair's group with d <= e, empty
 * records included, listed by pair, then by record) with NO limit on the pattern length.  The CPU twin of those kernels:
 * `tetrex search --verify --all-targets` answers patterns longer than TXQ_EDIT_LONG_MAX_PATTERN with it and the kernels are
 * compared with it.  hits: room for `capacity` quadruples of u32; *total receives the number of hits whatever the capacity
 * and the first `capacity` of them are written.  Buffers, threads, checks and the return value as txh_edit_search: a pair
 * out of range or an empty pattern is an error, so there are no status words. */
int txh_edit_targets(const uint8_t* patterns, const uint64_t* pat_offsets, size_t n_patterns, const uint8_t* text, const uint64_t* rec_offsets,
                     size_t n_records, const uint64_t* group_offsets, size_t n_groups, const uint32_t* pairs, size_t n_pairs,
                     const uint8_t* codes, unsigned threads, uint32_t* hits, size_t capacity, uint64_t* total);
/* Start and alignment of confirmed pairs on the host (host/edit_distance.hpp): the semantics and the layout of
 * txq_edit_align_device (include/txq.h: the walk back by three rules, 2 max_errors + 3 u32 words a pair — start, n_runs, runs as
 * (length << 2) | op —, "none" and the refusal marker passed on) with NO limit on the pattern length or the distance.  The CPU
 * twin of that kernel: it answers the pairs the device declines and the kernel is compared with it.  results: the 3 u32 a
 * search call wrote per pair.  A pair with d > max_errors, or whose triple is not a cell of its matrix (a record outside the
 * group, an end beyond the record, d > m, D[m][j] != d), gets start = 0xFFFFFFFE and nothing else written.  Buffers, threads and
 * the return value as txh_edit_search; max_errors is at most 2^24. */
int txh_edit_align(const uint8_t* patterns, const uint64_t* pat_offsets, size_t n_patterns, const uint8_t* text, const uint64_t* rec_offsets,
                   size_t n_records, const uint64_t* group_offsets, size_t n_groups, const uint32_t* pairs, size_t n_pairs, const uint32_t* results,
                   const uint8_t* codes, uint32_t max_errors, unsigned threads, uint32_t* align);

/* ---- .ibf index files (include/index_base.h:160-202 layout; see host/index_file.hpp) ---- */
typedef struct txh_index txh_index;
int txh_index_parse(const void* bytes, size_t n, txh_index** out);
/* the same from a file, the way `tetrex query` loads it: the file is mapped and the bit matrices stay in the mapping */
int txh_index_load(const char* path, txh_index** out);
/* a flat IBF index image from raw words; paths = '\n'-separated bin paths (one per bin) */
int txh_index_from_ibf(unsigned k, int dna, unsigned reduction, unsigned hash_count, uint64_t bins, uint64_t bin_size,
                       const uint64_t* words, const char* paths, txh_index** out);
/* JSON summary: k, molecule, is_hibf, reduction, hash_count, bins, format, per-IBF shapes, paths */
int txh_index_describe(const txh_index* ix, char* json, size_t cap);
/* words of IBF `ibf_id` (0 for a flat IBF); returns the word count (nothing written past cap) */
int64_t txh_index_words(const txh_index* ix, uint64_t ibf_id, uint64_t* out, size_t cap);
/* HIBF maps of IBF `ibf_id`: next_ibf_id and tb_to_user_bin, `bins` entries each; returns bins */
int64_t txh_index_maps(const txh_index* ix, uint64_t ibf_id, uint64_t* next_ibf_id, uint64_t* tb_to_user, size_t cap);
/* serialised file image; valid until the next call on this handle or txh_index_free */
const void* txh_index_serialise(txh_index* ix, size_t* bytes);
void txh_index_free(txh_index* ix);

/* ---- size-aware HIBF layout (host/layout.hpp; `tetrex index --layout sized`) ----
 * A pure function: counts[user_bins] = each user bin's k-mer count estimate (by user bin id); unions[user_bins x window] =
 * union estimates over runs of the bins in layout order (estimate descending, ties by id): unions[s * window + L - 1] for
 * the bins at sorted positions s .. s+L-1, window = min(B, 4 * ceil(B / t_max)).  params NULL: the defaults below. */
typedef struct {
    uint64_t tmax;       /* technical bins per IBF at most, a multiple of 64; 0: 64 * ceil(ceil(sqrt(B)) / 64) */
    float fpr;           /* of the user bins (0.05) */
    float relaxed_fpr;   /* of merged bins (0.3) */
    unsigned hash_count; /* 3 */
    double alpha;        /* weight of lower levels' bits (1.2) */
} txh_layout_params;
typedef struct txh_layout txh_layout;
int txh_hibf_layout(const double* counts, uint64_t user_bins, const double* unions, uint64_t window, const txh_layout_params* params,
                    txh_layout** out);
int64_t txh_layout_ibf_count(const txh_layout* l);
/* IBF `ibf` of the layout (0 = root, then depth-first pre-order): its bin_size and maps (as txh_index_maps); returns its
 * technical bins (nothing written past cap) */
int64_t txh_layout_ibf(const txh_layout* l, uint64_t ibf, uint64_t* bin_size, uint64_t* next_ibf_id, uint64_t* tb_to_user, size_t cap);
/* the layout order (user bin at each sorted position); returns B */
int64_t txh_layout_order(const txh_layout* l, uint64_t* order, size_t cap);
void txh_layout_free(txh_layout* l);
/* The same over a given order: order[user_bins] must be a permutation of 0 .. B-1 (anything else is refused), and
 * unions[s * window + L - 1] is the union of the bins order[s .. s+L-1].  With the layout order of counts this is
 * txh_hibf_layout, field for field.  txh_layout_order returns the order given. */
int txh_hibf_layout_ordered(const double* counts, uint64_t user_bins, const uint64_t* order, const double* unions, uint64_t window,
                            const txh_layout_params* params, txh_layout** out);

/* ---- similarity rearrangement of the user bins before the layout (host/layout.hpp; `tetrex index --layout sized --rearrange`) ----
 * Intervals of the layout order: an interval starts at sorted position s and takes the following positions e while
 * counts[order[e]] >= ratio * counts[order[s]] (ratio in (0, 1]) and while it is shorter than max_len (1 .. 4096; 0: 4096).
 * starts receives the first sorted position of every interval, ascending; returns their number (nothing written past cap). */
#define TXH_REARRANGE_MAX_LEN 4096
int64_t txh_rearrange_intervals(const double* counts, uint64_t user_bins, double ratio, uint64_t max_len, uint64_t* starts, size_t cap);
/* The chain inside one interval of n bins: counts[n] by position in the interval, unions[n x n] their pairwise union
 * estimates.  Position 0 stays; then the bin not yet placed with the largest J = (c_last + c_j - u[last][j]) / u[last][j]
 * (in double, in this order; u == 0: J = 0; ties: the smaller position) follows the bin placed last.  n <= 2: the identity.
 * chain[n] receives the positions in their new order. */
int txh_rearrange_chain(const double* counts, const double* unions, uint64_t n, uint64_t* chain);

/* The whole `tetrex index` build (FASTA files -> index image, bits set on the GPU), without the CLI.  Exported by
 * libtetrex_query.so (it needs libtxq.so); errors via txe_last_error().  The handle is an ordinary txh_index
 * (txh_index_describe / _words / _maps / _serialise / _free of libtetrex_host.so).  options NULL: the CLI's defaults. */
typedef struct {
    unsigned k;          /* 6 */
    int dna;             /* -n */
    unsigned reduction;  /* 0 none, 1 murphy, 2 li (-r) */
    unsigned hash_count; /* 3 (-c) */
    float fpr;           /* 0.05 (-p) */
    int flavour;         /* 0 HIBF, uniform layout (default); 1 HIBF, sized layout (--layout sized); 2 flat IBF (-i) */
    uint64_t tmax;       /* --tmax (sized only; 0: the default) */
    int device;          /* -D */
    double rearrange_ratio; /* --rearrange [--rearrange-ratio R] (sized only): 0 off (the default), else the ratio in (0, 1] */
} txh_build_options;
int txh_index_build(const char* const* paths, size_t n, const txh_build_options* options, txh_index** out);

#ifdef __cplusplus
}
#endif
#endif
