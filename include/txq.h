/* txq.h — C-ABI of the MI355X (gfx950) TetRex query engine (libtxq.so).
 *
 * This is the drop-in boundary for the (H)IBF probe hot path of remyschwab/TetRex.  Every
 * entry point replaces one seam of the reference (paths relative to the reference root):
 *
 *   txq_index_upload        <- TetrexIndex::spawn_agent()            include/index_base.h:145
 *                              IBFIndex::spawn_agent / HIBFIndex::spawn_agent
 *                                                                     include/index_ibf.h:141-144, index_hibf.h:149-152
 *                              (the agent's raw pointer into the bit matrix becomes an HBM-resident copy)
 *   txq_probe / _device     <- TetrexIndex::query(uint64_t) -> bitvector  include/index_base.h:104-107
 *                              IBFIndex::query  -> bulk_contains      include/index_ibf.h:146-150
 *                              HIBFIndex::query -> membership_for(.,1) + populate_bitvector
 *                                                                     include/index_hibf.h:132-147
 *                              (batched: one call probes n k-mers; call sites include/otf_collector.h:262,273)
 *   txq_run_programs        <- OTFCollector::collect()               include/otf_collector.h:341-393
 *                              (the mask algebra of the collector — path_ &= hits, absorb |=, Match |= —
 *                               compiled by the host into mask-DAG programs, see txq_program.h)
 *   txq_emplace_device      <- interleaved_bloom_filter::emplace     include/index_ibf.h:94-98 (index build, "next")
 *   txq_count / _device     <- seqan::hibf membership_for(values, threshold) / counting_agent::bulk_count, the general form of
 *                              the one-value, threshold-1 call at include/index_hibf.h:142-147 (`tetrex search`)
 *   txq_edit_search / _device  (no counterpart: `tetrex search --verify` confirms candidate bins by edit distance)
 *   txq_edit_search_long / _device  (the same for patterns of up to 4096 bytes, the pattern spread over the lanes of a wave)
 *   txq_edit_align / _device  (no counterpart: start and CIGAR of the pairs a search call confirmed, `--verify --align`)
 *   txq_edit_windows / _device  (no counterpart: txq_edit_search for windows into one letter buffer, `--window --verify-windows`)
 *   txq_edit_align_windows / _device  (no counterpart: txq_edit_align for windows against a table of text views, `--align-windows`)
 *   txq_edit_window_targets / _device  (no counterpart: txq_edit_targets for windows against a table of text views, `--window-targets`)
 *   txq_frame_window_letters / _device  (no counterpart: the letters, stops and thresholds of translated windows, `--verify-frame-windows`)
 *
 * Conventions: plain C, no exceptions cross the boundary.  Every function returns 0 on success or a
 * negative txq_status; txq_last_error() gives the message for the calling thread.  Host buffers are
 * owned by the caller; device memory is owned by the library unless the function name ends in
 * _device (then pointers are HIP device pointers owned by the caller and `stream` is a hipStream_t,
 * NULL = default stream, and the call is asynchronous on that stream).  One txq_index may be used
 * from one host thread at a time; distinct indexes are independent.
 *
 * Bit layout (identical to seqan::hibf::bit_vector as used by the reference): mask word w, bit b
 * (LSB first) <-> bin 64*w + b.  Bits >= bins in the last word are zero.
 */
#ifndef TXQ_H
#define TXQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TXQ_VERSION 1

/* Environment variables.  Every one selects between code paths that give the SAME results (A/B measurements, tests that
 * run one input through every path); none is needed in production.  They are read at txq_init, txq_index_upload,
 * txq_session_begin, txq_run_programs*, txq_probe* and txq_edit_search* — never while a stage runs — and a session keeps the values it began with.
 *   TXQ_TRACE, TXQ_TRACE_STAGES, TXQ_TRACE_SYNC      timers and per-stage notes on stderr
 *   TXQ_DENSE_TREE=0|1|2                              dense steps on a regular HIBF: generic descent | TreeRows | TreeRowsByLane
 *   TXQ_DENSE_UNROLL, TXQ_DENSE_SLICES, TXQ_DENSE_TILE_ROUNDS, TXQ_DENSE_NT   shape of a dense step's tiles, cache policy of its destination accesses
 *   TXQ_FUSE_UNITS=0, TXQ_ONE_STREAM                  one launch per kind and level; no second stream
 *   TXQ_FINAL_PINNED=0                                a session's final masks gathered on the device and copied, not written straight into pinned host memory
 *   TXQ_SPARSE_STEPS=0, TXQ_SPARSE_UNROLL=2|3, TXQ_SPARSE_UNITS=<n>
 *                                                     pushed steps of tracked blocks on narrow masks: rounds of entries instead of units; units in
 *                                                     flight per lane group; units per chunk (default 512)
 *   TXQ_KMER_TABLE_MB=<n>, TXQ_KMER_TABLE_MIN=<n>     most an index's table of all k-mers' masks may take (default 512; 0: none);
 *                                                     the session of fewest programs that builds it (default 16)
 *   TXQ_HIBF_INTERLEAVE=0, TXQ_HIBF_INTERLEAVE_PROBE=0, TXQ_HIBF_LEVELS=1, TXQ_HIBF_STATIONARY=0, TXQ_HIBF_SMALL=0,
 *   TXQ_HIBF_LAYOUT_ORDER=0, TXQ_HIBF_LAYOUT_FUSED=0, TXQ_HIBF_LANE_HASH, TXQ_HIBF_STEPS_PER_GROUP, TXQ_HIBF_TILE, TXQ_HIBF_UNROLL, TXQ_HIBF_STORE_KIND, TXQ_HIBF_WAVES, TXQ_HIBF_STACK_LDS, TXQ_HIBF_LAYOUT_DIRECT=0
 *                                                     which HIBF descent kernel runs, and its tiling
 *   TXQ_PROBE_BLOCKS_PER_CU, TXQ_PROBE_UNROLL, TXQ_PROBE_NT   grid and variant of the flat probe kernel
 *   TXQ_EDIT_CHUNK=<bytes>                            bytes of text per lane of the edit-distance kernel (txq_edit_search, below)
 *   TXQ_EDIT_LONG_SPAN=<bytes>                        bytes of text per lane group of the long-pattern edit-distance kernel (txq_edit_search_long, below)
 *   TXQ_EDIT_WINDOWS_BUNDLE=1|2|4                     the most (window, bin) pairs that walk a bin's text together (txq_edit_windows, below)
 *   TXQ_COUNT_WINDOWS_UNIT=<n>, TXQ_COUNT_WINDOWS_WAVES=1|4   windows per workgroup of the sliding count and its waves (txq_count_windows, below)
 *   TXQ_COUNT_WINDOWS_TREE=0|1                        on an HIBF: every (window, IBF) pair counted in full | the count slides down the tree
 *                                                     (txq_count_windows, below)
 *   TXQ_PROBE_TABLE=0|1                               a flat probe's table of its batch's k-mer domain: never | whenever it fits
 *                                                     (unset: where the batch repeats its values often enough to pay for it)
 *   TXQ_PROBE_TABLE_KEEP=0                            that table is built from its first row on every call, not kept with the
 *                                                     index and extended (the rows never outlive txq_emplace_device either way)
 *   TXQ_PROBE_TABLE_FUSED=0                           a call on kept rows runs three launches (sample, build, answer) like a first
 *                                                     call, not the one launch that answers, counts and extends the table
 *   TXQ_PROBE_TABLE_TILE=0                            no table-only tile body: a full tile whose 64 k-mers all have a table row
 *                                                     takes the general body like every other tile (A/B and cross-checks)
 *   TXQ_PROBE_SORT=0|1                                a large one-launch call on kept rows, without d_alive, on rows of 16 or 32 whole
 *                                                     words: never | answered from its batch in value-bucket order (three small
 *                                                     launches partition it), so that an XCD's L2 holds the table rows it reads.
 *                                                     Scratch kept with the index, grow-only: 8 bytes per k-mer of the largest such
 *                                                     batch and up to 4 MB of counters, at most TXQ_KMER_TABLE_MB MiB (a larger
 *                                                     batch is answered in batch order)
 *   TXQ_PROBE_SORT_MIN=<n>                            the smallest such batch (default 8388608)
 *   TXQ_PROBE_SORT_BUCKET_KB=<n>                      table rows per value bucket, in KiB (default 1024; at most 256 buckets)
 * (tests/test_gpu_knobs.py runs a workload under each of them against the oracle.) */

typedef enum {
    TXQ_OK = 0,
    TXQ_ERR_ARG = -1,      /* invalid argument / inconsistent descriptor            */
    TXQ_ERR_HIP = -2,      /* a HIP runtime call failed (message has the HIP error)  */
    TXQ_ERR_NOMEM = -3,    /* host or device allocation failed                       */
    TXQ_ERR_STATE = -4,    /* txq_init not called / no GPU present                   */
    TXQ_ERR_OVERFLOW = -5, /* an internal work queue overflowed (HIBF frontier)      */
    TXQ_ERR_PROGRAM = -6   /* malformed mask-DAG program                             */
} txq_status;

typedef struct txq_index txq_index; /* opaque; owns device memory */

/* Host view of one interleaved Bloom filter, exactly the six scalars + the word array that
 * seqan::hibf::interleaved_bloom_filter serialises (SURVEY.md §8c ".ibf layout"):
 * words[r * bin_words + w] holds technical bins 64w..64w+63 of row r. */
typedef struct {
    uint64_t bins;       /* number of (technical) bins in use, B                  */
    uint64_t tech_bins;  /* 64 * ceil(B / 64)                                     */
    uint64_t bin_size;   /* rows m                                                */
    uint64_t hash_shift; /* countl_zero(bin_size)                                 */
    uint64_t bin_words;  /* tech_bins / 64                                        */
    uint64_t hash_funs;  /* h, 1..5                                               */
    const uint64_t* words;
} txq_ibf_desc;

#define TXQ_MERGED_BIN UINT64_MAX

/* Host view of a whole index.  n_ibf == 1 and NULL maps: a flat IBF (IBFIndex).  Otherwise an
 * HIBF: ibf[0] is the root, next_ibf_id[i][b] is the child IBF of merged technical bin b of
 * IBF i, tb_to_user_bin[i][b] its user bin or TXQ_MERGED_BIN; each map has ibf[i].bins entries. */
typedef struct {
    uint64_t n_ibf;
    const txq_ibf_desc* ibf;
    const uint64_t* const* next_ibf_id;
    const uint64_t* const* tb_to_user_bin;
    uint64_t user_bins; /* bits in a result mask (== ibf[0].bins for a flat IBF) */
} txq_index_desc;

typedef struct {
    uint64_t user_bins;    /* bits of a full (unsharded) mask                         */
    uint64_t mask_words;   /* words of a full mask = ceil(user_bins / 64)             */
    uint64_t shard_word0;  /* first mask word owned by this shard                     */
    uint64_t shard_words;  /* mask words owned by this shard (what txq_probe emits)   */
    uint64_t n_ibf;        /* 1 for a flat IBF                                        */
    uint64_t device_bytes; /* HBM held by the index                                   */
    int      is_hibf;
    int      device;       /* HIP device ordinal                                      */
    int      join_or;      /* 0: this shard owns the mask-word columns [shard_word0, shard_word0 + shard_words);
                              1: a SUB-TREE shard (txq_index_upload_subtrees): it emits full-width masks (shard_word0 = 0,
                              shard_words = mask_words) that hold only the user bins of its sub-trees — the shards' masks are ORed */
    int      shard_rank;   /* which shard of ... */
    int      n_shards;     /* ... how many this index was uploaded as                 */
    int      reserved;
} txq_index_info;

/* Bind this process to n_devices GPUs (device_ids == NULL: devices 0 .. n_devices-1).  One process per GPU
 * (n_devices == 1, the torch.distributed / RCCL deployment) and one process driving all GPUs of a node are both
 * supported: shard r of an index (txq_index_upload, txq_index_create_ibf) lives on device_ids[r % n_devices], and
 * every call on an index or session runs on the device that holds it, whichever thread makes it.
 * Fails with TXQ_ERR_STATE when no GPU is present: there is no CPU fallback anywhere in this library. */
int txq_init(int n_devices, const int* device_ids);
int txq_shutdown(void);
const char* txq_last_error(void);
int txq_device_count(void); /* >= 0, or a negative txq_status */

/* Copy an index into HBM (of device_ids[shard_rank % n_devices], see txq_init).  With n_shards > 1 only the
 * mask-word columns of shard `shard_rank` are kept (flat IBF: words [W*r/R, W*(r+1)/R) of every row, re-laid out
 * contiguously; HIBF: the whole tree is kept and only the user-bin mask columns are sharded). */
int txq_index_upload(const txq_index_desc* desc, int shard_rank, int n_shards, txq_index** out);
/* The same for an HIBF, sharded by SUB-TREES where the tree is a general one (as seqan::hibf's layout shapes it: reference
 * include/index_hibf.h:114-129): the root is replicated, its merged bins — the level-1 sub-trees — are dealt over the shards
 * by the row words under them (largest first, to the shard that holds least), the user bins that sit in the root itself go to
 * shard 0, and a shard keeps only its own sub-trees (in its copy of the root the technical bins of the others are cleared, so
 * nothing is ever descended into or reported for them).  Such a shard emits FULL-WIDTH masks (info.join_or = 1) with the user
 * bins of its sub-trees only; a split bin may straddle shards: the join is an OR.  Its sessions work in layout order like an
 * unsharded general tree's.  A regular two-level tree (what `tetrex index` writes) and a flat IBF are sharded by mask
 * columns exactly as txq_index_upload does (info.join_or = 0). */
int txq_index_upload_subtrees(const txq_index_desc* desc, int shard_rank, int n_shards, txq_index** out);
int txq_index_get_info(const txq_index* ix, txq_index_info* info);
int txq_index_free(txq_index* ix);

/* Do sessions on this index execute dense DP steps (include/txq_program.h version 3)?  0: no (flat IBFs with 2^32 rows
 * and more).  1: yes (any HIBF: a step runs as a batch of k-mers through the descent).  2: yes, fused into one kernel
 * (flat IBFs, regular two-level HIBFs) — such sessions also run TRACKED programs (sparse blocks with live lists). */
int txq_index_supports_dense(const txq_index* ix);

/* Device memory as a session on this index will find it: bytes free on the index's device, and bytes of slot storage the
 * index keeps from earlier sessions (the next session reuses them before it allocates).  Host layers size their budgets
 * for slot storage (dense blocks) by the sum instead of by a constant. */
int txq_index_memory(const txq_index* ix, uint64_t* free_bytes, uint64_t* kept_bytes);

/* One 64-bit value a host layer may keep with the index (0 after upload); libtetrex_query stores what its staged
 * expansion has learned about the index there. */
int txq_index_set_tag(txq_index* ix, uint64_t tag);
int txq_index_get_tag(const txq_index* ix, uint64_t* tag);

/* An empty (all-zero) flat IBF living only in HBM, for device-side construction. */
int txq_index_create_ibf(uint64_t bins, uint64_t bin_size, uint64_t hash_funs, int shard_rank, int n_shards,
                         txq_index** out);
/* Copy the shard's bit matrix back, row-major [bin_size][shard_words]. */
int txq_index_download_words(const txq_index* ix, uint64_t* words, size_t n_words);

/* Batched bulk_contains: masks[i * shard_words + w] for k-mer i.  Host buffers; synchronous.
 * Chunks are pipelined (probe of chunk c+1 overlaps the copy-back of chunk c); a `masks` buffer
 * from txq_host_alloc (pinned) receives the device copies directly, any other one goes through a
 * pinned bounce buffer. */
int txq_probe(txq_index* ix, const uint64_t* kmers, size_t n, uint64_t* masks);
/* Same on device-resident buffers, asynchronous on `stream`.  d_alive may be NULL; otherwise it
 * receives ceil(n/64) words, bit i set iff mask i has any bit set in this shard
 * (bitvector::none() of include/otf_collector.h:383, per shard). */
int txq_probe_device(txq_index* ix, const uint64_t* d_kmers, size_t n, uint64_t* d_masks, uint64_t* d_alive,
                     void* stream);
/* A trace of the flat probe's sorted answer (TXQ_PROBE_SORT above), for tests: out[0] = calls that bucketed their batch,
 * out[1] = answers that then ran in bucket order (a batch with a k-mer at or above the table's valid rows is answered in
 * batch order), counted since the table's state was last started over.  Waits for the index's last probe call. */
int txq_index_probe_sorted(txq_index* ix, uint64_t out[2]);

/* Threshold membership of value sets (seqan::hibf membership_for(values, threshold); counting_agent::bulk_count on a
 * flat IBF).  Query q owns d_values[d_offsets[q] .. d_offsets[q+1]) (n_queries + 1 ascending offsets, at most 2^32-1
 * values per call).  d_hits: n_queries x shard_words words.  d_counts: NULL, or n_queries x (64 * shard_words) u32.
 * Flat IBF: counts[q][b] = how many values of q have bit b in bulk_contains, hits[q][b] = counts[q][b] >= thresholds[q].
 * HIBF: every visited IBF counts the values per technical bin; a run of technical bins of one user bin is summed (a split
 * bin's parts add up), a merged bin whose count reaches the threshold is visited, a run whose sum reaches it is a hit;
 * counts[q][u] is the run's sum (the largest, where a user bin's parts form several runs; 0 for a user bin whose IBF is not
 * visited), so hits[q][u] == (counts[q][u] >= thresholds[q]) on every kind of index.  Threshold 0 selects every bin; one value at
 * threshold 1 gives txq_probe's mask.  A column shard answers for its own columns; sub-tree shards are refused (TXQ_ERR_ARG).
 * txq_count checks its host offsets before anything is launched; txq_count_device trusts the device offsets it is given.
 * Neither can check that the offsets stay within the values (no value count is passed): that is the caller's part.
 * Limits: on an HIBF every IBF may have at most 8192 technical bins (a wider one: TXQ_ERR_ARG).  On a flat IBF a long query is
 * spread over many workgroups; on an HIBF each (query, IBF) pair is counted by one wave, so a very long query (10^5 values and
 * more) is slow there, though exact. */
int txq_count_device(txq_index* ix, const uint64_t* d_values, const uint64_t* d_offsets, size_t n_queries,
                     const uint32_t* d_thresholds, uint64_t* d_hits, uint32_t* d_counts, void* stream);
int txq_count(txq_index* ix, const uint64_t* values, const uint64_t* offsets, size_t n_queries,
              const uint32_t* thresholds, uint64_t* hits, uint32_t* counts);  /* host buffers, synchronous */

/* The same of sliding windows over one value array (`tetrex search --window`; not in the reference).  Window j owns
 * d_values[d_win_begin[j] .. d_win_begin[j] + d_win_len[j]).  The windows form a sliding sequence: d_win_begin does not
 * decrease and d_win_begin + d_win_len does not decrease; they may overlap, touch, leave gaps, repeat, or be empty.  The result
 * is DEFINED as what txq_count_device gives when window j is query j — hits, counts, threshold 0 selecting every user bin of the
 * shard, a column shard answering for its own columns, d_counts == NULL — and sub-tree shards are refused (TXQ_ERR_ARG).
 * Flat IBF: a workgroup takes TXQ_COUNT_WINDOWS_UNIT consecutive windows, counts the first in full and every next one from
 * its predecessor: the values that enter are added to the counters, those that leave are subtracted (their rows were read a
 * window ago and come from L2), so a window costs the rows of two steps, not of its whole length.  A window is counted by ONE
 * workgroup: a window of 10^5 values is exact, but slow (txq_count_device spreads such a query over many workgroups).
 * HIBF: the count slides down the tree.  A wave takes a unit of min(TXQ_COUNT_WINDOWS_UNIT, 32) consecutive windows on ONE IBF
 * and slides over those windows of the unit that visit the IBF — a subsequence of a sliding sequence still slides —, then hands
 * every child the windows of the unit that descend into it, as one work item of the next level.  With TXQ_COUNT_WINDOWS_TREE=0
 * the windows run as independent queries, each (window, IBF) pair counted in full by one wave, no sliding.  Every IBF may have
 * at most 8192 technical bins, as for txq_count.
 * txq_count_windows checks before anything is launched that the windows slide, that each ends within n_values and that no
 * pointer it needs is NULL (TXQ_ERR_ARG); txq_count_windows_device trusts the device arrays it is given.  It allocates nothing
 * outside the index's scratch and does not synchronise with the host.
 *   TXQ_COUNT_WINDOWS_UNIT=<n>    windows per workgroup on a flat IBF (default 16, 1 .. 2^20; read at every call)
 *   TXQ_COUNT_WINDOWS_WAVES=1|4   waves of that workgroup (default 1; read at every call)
 *   TXQ_COUNT_WINDOWS_TREE=0|1    on an HIBF: independent queries | sliding in units of min(TXQ_COUNT_WINDOWS_UNIT, 32) windows
 *                                 (default 1: on 2*10^5 windows sliding by 16 values it takes 0.25 to 0.63 of the other route's
 *                                 time; read at every call)
 * The results are the same for every value of each. */
int txq_count_windows_device(txq_index* ix, const uint64_t* d_values, const uint64_t* d_win_begin, const uint32_t* d_win_len,
                             size_t n_windows, const uint32_t* d_thresholds, uint64_t* d_hits, uint32_t* d_counts, void* stream);
int txq_count_windows(txq_index* ix, const uint64_t* values, size_t n_values, const uint64_t* win_begin, const uint32_t* win_len,
                      size_t n_windows, const uint32_t* thresholds, uint64_t* hits, uint32_t* counts);  /* host buffers, synchronous */
/* A trace of the index's last txq_count_windows / txq_count_windows_device call on an HIBF, for tests and measurements:
 * out[0] = (window, IBF) visits, out[1] = values added to counters, out[2] = values subtracted from them, out[3] = work items
 * (one wave each).  With TXQ_COUNT_WINDOWS_TREE=0 that is visits, the summed lengths of the visiting windows, 0 and visits.
 * All zero on a flat IBF, before the first call, and after a call of no windows or one that failed.  Waits for the index's
 * last such call. */
int txq_count_windows_trace(txq_index* ix, uint64_t out[4]);

/* Six-frame translation of nucleotide records into the k-mer values of a peptide index (`tetrex search --translate`; not in
 * the reference).  Record r is the bytes d_seq[d_rec_offsets[r] .. d_rec_offsets[r+1]) (n_records + 1 ascending offsets).
 * Letters A C G T U in either case (U reads as T); any other byte is ambiguous.  Frame f = 0..5 is +1 +2 +3 -1 -2 -3: frames
 * +1..+3 read the record from offset 0, 1, 2, frames -1..-3 its reverse complement from offset 0, 1, 2; trailing bytes that
 * do not fill a codon are dropped.  Codons translate by NCBI table 1, a codon with an ambiguous byte is X, a stop is *.
 * The values of a frame: every window of k residues without a stop, in ascending position, folded as the index's encoder
 * does it: value = sum of d_codes[residue j] << 5 (k - 1 - j), d_codes the encoder's 256-byte table (so reduced alphabets
 * work unchanged).  Query 6 r + f owns d_values[d_offsets[6 r + f] .. d_offsets[6 r + f + 1]); d_offsets has 6 n_records + 1
 * entries, d_offsets[0] = 0, and is in the form txq_count_device takes.  d_values must hold txq_translate_bound values:
 * the sum over records and offsets o = 0, 1, 2 of 2 max(0, floor((L_r - o) / 3) - k + 1) (UINT64_MAX: bad arguments).
 * The call is deterministic and does not synchronise with the host; its scratch is the library's, in stream order.
 * txq_translate is the synchronous twin on host buffers (it checks the record offsets).  k outside 1..12 and null
 * pointers: TXQ_ERR_ARG. */
uint64_t txq_translate_bound(const uint64_t* rec_offsets, size_t n_records, unsigned k);
int txq_translate_device(const uint8_t* d_seq, const uint64_t* d_rec_offsets, size_t n_records, unsigned k, const uint8_t* d_codes,
                         uint64_t* d_values, uint64_t* d_offsets, void* stream);
int txq_translate(const uint8_t* seq, const uint64_t* rec_offsets, size_t n_records, unsigned k, const uint8_t* codes,
                  uint64_t* values, uint64_t* offsets);

/* The same translation, and the frames cut into windows (`tetrex search --translate --frame-window`; not in the
 * reference).  Records, frames, genetic code and values are those of txq_translate above: d_values and d_offsets come out
 * exactly as txq_translate_device writes them.  A frame of R = floor((L - o) / 3) residues is cut like a record of R letters
 * under `tetrex search --window`: no window where R < k; one, [0, R), where R <= window; otherwise [a, a + window) at a = 0,
 * step, 2 step, ... while a + window <= R, and one more at R - window where the last of these ends before R.  window and step
 * count residues.  The windows of frame q = 6 r + f are d_win_offsets[q] .. d_win_offsets[q + 1] (6 n_records + 1 entries, the
 * first 0).  Window [a, a + l) owns the frame's stop-free k-mers at residue positions a .. a + l - k, which are consecutive
 * values: d_win_begin[j] is the index of the first of them in d_values (where there is none: the index of the frame's first
 * value behind position a, d_offsets[q + 1] at the latest) and d_win_len[j] their number, which may be 0.
 * Sliding order: over the whole array d_win_begin does not decrease and d_win_begin + d_win_len does not decrease — within a
 * frame because the windows ascend, from frame to frame because the frames' values follow each other — so d_values,
 * d_win_begin and d_win_len are what txq_count_windows_device takes, unchanged, for any range of windows.
 * txq_translate_windows_bound is the exact number of windows (no GPU needed; UINT64_MAX: bad arguments): d_win_begin and
 * d_win_len must hold that many entries.  k outside 1..12, window < k, step outside 1..window and null pointers: TXQ_ERR_ARG,
 * and nothing is written.  A call may produce at most 2^32 - 2 windows: txq_translate_windows refuses more (TXQ_ERR_ARG);
 * txq_translate_windows_device cannot see the record lengths, so its caller asks txq_translate_windows_bound.  The device
 * call is deterministic, allocates nothing outside the library's stream-ordered scratch, reads nothing back and does not
 * synchronise with the host.  Thresholds are the caller's: they follow from d_win_len.  txq_translate_windows is the
 * synchronous twin on host buffers (it checks the record offsets). */
uint64_t txq_translate_windows_bound(const uint64_t* rec_offsets, size_t n_records, unsigned k, uint32_t window, uint32_t step);
int txq_translate_windows_device(const uint8_t* d_seq, const uint64_t* d_rec_offsets, size_t n_records, unsigned k, const uint8_t* d_codes,
                                 uint32_t window, uint32_t step, uint64_t* d_values, uint64_t* d_offsets, uint64_t* d_win_offsets,
                                 uint64_t* d_win_begin, uint32_t* d_win_len, void* stream);
int txq_translate_windows(const uint8_t* seq, const uint64_t* rec_offsets, size_t n_records, unsigned k, const uint8_t* codes, uint32_t window,
                          uint32_t step, uint64_t* values, uint64_t* offsets, uint64_t* win_offsets, uint64_t* win_begin, uint32_t* win_len);

/* The six frames of nucleotide records as residue letters (`tetrex search --translate --verify-frames`; not in
 * the reference).  Records, letters, frames and the genetic code are those of txq_translate above; a frame with offset o over
 * L bytes has floor((L - o) / 3) residues (none where L < o), upper-case letters of NCBI table 1, '*' for a stop, 'X' for a
 * codon with an ambiguous byte.  Frame 6 r + f is d_frames[d_frame_offsets[6 r + f] .. d_frame_offsets[6 r + f + 1]): 6 n_records
 * + 1 offsets, the first 0, the frames back to back — the form txq_edit_search*_device take as d_patterns / d_pat_offsets.
 * txq_translate_frames_bound is the exact size in bytes: the sum over records and o = 0, 1, 2 of 2 floor((L_r - o) / 3)
 * (UINT64_MAX: bad arguments).  d_frames may have any alignment; no byte at or behind frames_bytes is written (the offsets are
 * complete all the same), no byte outside the frames is written, and nothing of d_frames is read.  The call is deterministic,
 * allocates nothing, reads nothing back and does not synchronise with the host.  txq_translate_frames is the synchronous twin
 * on host buffers (it checks the record offsets; a buffer below the bound: TXQ_ERR_ARG).  Null pointers: TXQ_ERR_ARG (d_seq
 * may be null where the records have no bytes, d_frames where frames_bytes is 0). */
uint64_t txq_translate_frames_bound(const uint64_t* rec_offsets, size_t n_records);
int txq_translate_frames_device(const uint8_t* d_seq, const uint64_t* d_rec_offsets, size_t n_records, uint8_t* d_frames, size_t frames_bytes,
                                uint64_t* d_frame_offsets, void* stream);
int txq_translate_frames(const uint8_t* seq, const uint64_t* rec_offsets, size_t n_records, uint8_t* frames, size_t frames_bytes,
                         uint64_t* frame_offsets);  /* host buffers, synchronous */

/* Where the letters of every frame window lie, how many stops they hold and the threshold that follows
 * (`tetrex search --translate --frame-window --verify-frame-windows`; not in the reference).  The step between
 * the two calls above and txq_count_windows_device / txq_edit_windows_device.  d_rec_offsets, k, window and step are those of
 * the txq_translate_windows_device call that left d_win_offsets and d_win_len (n_windows entries: the windows' stop-free
 * k-mers w); d_frames, frames_bytes and d_frame_offsets are as txq_translate_frames_device left them for the same records.
 * For window j, window j - d_win_offsets[q] of its frame q with residues [a, a + l):
 *   d_let_begin[j]   d_frame_offsets[q] + a, the index of its first residue letter in d_frames
 *   d_let_len[j]     l
 *   d_stops[j]       s, the number of '*' among those letters
 *   d_thresholds[j]  0xFFFFFFFF ("not searched", what txq_count_windows_device takes for it) where s > edits or
 *                    w <= k (edits - s), else w - k (edits - s)
 * The threshold loses nothing: within `edits` edits of anything every stop is an edited column of its own, the edits - s
 * that remain touch at most k of the w stop-free k-mers each, and the k-mers only stops touch are not among the w.
 * d_let_begin and d_let_len are the window arrays txq_edit_windows_device takes (letters_bytes = frames_bytes), d_thresholds
 * what txq_count_windows_device takes: nothing goes to the host between translation and count.  A j at or behind
 * d_win_offsets[6 n_records] and a window its frame does not have get begin 0 and length 0, a window whose letters leave
 * frames_bytes keeps its begin and length; all of them get 0 stops and "not searched".  No byte at or behind frames_bytes is read whatever the arrays say, and
 * d_frames may have any alignment.  The call is deterministic, allocates nothing, reads nothing back and does not
 * synchronise with the host.  Null pointers, k outside 1..12, window < k and step outside 1..window: TXQ_ERR_ARG, nothing
 * written; at most 2^32 - 2 windows.  txq_frame_window_letters is the synchronous twin on host buffers: it checks that the
 * three offset arrays ascend, that the frame and window offsets begin at 0 and that n_windows covers the window offsets. */
int txq_frame_window_letters_device(const uint64_t* d_rec_offsets, size_t n_records, unsigned k, uint32_t window, uint32_t step,
                                    const uint8_t* d_frames, size_t frames_bytes, const uint64_t* d_frame_offsets,
                                    const uint64_t* d_win_offsets, const uint32_t* d_win_len, size_t n_windows, uint32_t edits,
                                    uint64_t* d_let_begin, uint32_t* d_let_len, uint32_t* d_stops, uint32_t* d_thresholds, void* stream);
int txq_frame_window_letters(const uint64_t* rec_offsets, size_t n_records, unsigned k, uint32_t window, uint32_t step, const uint8_t* frames,
                             size_t frames_bytes, const uint64_t* frame_offsets, const uint64_t* win_offsets, const uint32_t* win_len,
                             size_t n_windows, uint32_t edits, uint64_t* let_begin, uint32_t* let_len, uint32_t* stops, uint32_t* thresholds);

/* Approximate matching of (pattern, bin) pairs by edit distance (`tetrex search --verify`; not in the reference).
 * Classes: d_codes[256] maps a byte to a class 0..30; any other value (255 by convention) is "matches nothing, not even
 * itself".  Two bytes match when their classes are equal and below 31.
 * Distance of a pattern P of m >= 1 bytes to a text record R of n >= 0 bytes, by Sellers' recurrence:
 *     D[i][0] = i, D[0][j] = 0, D[i][j] = min(D[i-1][j-1] + [P[i-1] and R[j-1] do not match], D[i-1][j] + 1, D[i][j-1] + 1),
 *     d(P, R) = min over j = 0..n of D[m][j]     (the fewest edits that turn P into a substring of R; never across two records).
 * Pattern p is d_patterns[d_pat_offsets[p] .. d_pat_offsets[p+1]), record r is d_text[d_rec_offsets[r] .. d_rec_offsets[r+1])
 * (records back to back: n + 1 ascending offsets each), group g — one bin — is records d_group_offsets[g] ..
 * d_group_offsets[g+1] - 1.  Pair i is d_pairs[3 i .. 3 i + 2] = (pattern, group, cap e).  With d* the least d(P, R) over the
 * group's records, d_out[3 i .. 3 i + 2] = (d*, r, j) where d* <= e: r the lowest record index (into d_rec_offsets) that reaches
 * d*, j the lowest end position in r that reaches it — the number of bytes of r before the match's end, 0 for an empty
 * match; otherwise (a distance above the cap, a group of no records) all three are 0xFFFFFFFF.  Distances above the cap are
 * never reported.
 * Patterns of 1 .. TXQ_EDIT_MAX_PATTERN bytes run here (up to TXQ_EDIT_LONG_MAX_PATTERN: txq_edit_search_long below; longer
 * ones: txh_edit_search of include/txh.h, the same semantics on the host).  txq_edit_search checks its host buffers first: m = 0, m > TXQ_EDIT_MAX_PATTERN, a pair that names a
 * pattern or group out of range, offsets that do not ascend or leave their array, null pointers: TXQ_ERR_ARG, nothing
 * launched.  txq_edit_search_device cannot read its device buffers without waiting for them, so it returns TXQ_ERR_ARG only
 * for what it can see (null pointers, the size limits below) and the kernels check the rest: such a pair gets
 * (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFE) — a caller that cannot vouch for its buffers looks for 0xFFFFFFFE in the second field —, and with pattern_bytes / text_bytes (the sizes of d_patterns /
 * d_text) no load leaves a buffer whatever the offsets say.  At most 2^31 pairs, text_bytes + n_records < 2^48.
 * d_workspace: TXQ_EDIT_WORKSPACE(n_pairs) bytes of device memory, 8-byte aligned, the caller's like every other buffer of
 * a _device call (it holds a 64-bit key and a unit count per pair while the call runs; its contents mean nothing afterwards).
 * The call allocates nothing and does not synchronise with the host.
 *   TXQ_EDIT_CHUNK=<bytes>   the bytes of text one lane owns (default 512, a multiple of 16 in 16 .. 2^20; read at every call).
 *                            A lane re-reads m + min(e, m) bytes in front of its chunk, 64 chunks are one wave's unit of
 *                            work; the results do not depend on it (tests use 64 to cut small texts into many units). */
#define TXQ_EDIT_MAX_PATTERN 512
#define TXQ_EDIT_WORKSPACE(n_pairs) (16 * (size_t)(n_pairs) + 8)
int txq_edit_search_device(const uint8_t* d_patterns, const uint64_t* d_pat_offsets, size_t n_patterns, size_t pattern_bytes,
                           const uint8_t* d_text, const uint64_t* d_rec_offsets, size_t n_records, size_t text_bytes,
                           const uint64_t* d_group_offsets, size_t n_groups, const uint32_t* d_pairs, size_t n_pairs,
                           const uint8_t* d_codes, uint32_t* d_out, void* d_workspace, void* stream);
int txq_edit_search(const uint8_t* patterns, const uint64_t* pat_offsets, size_t n_patterns, const uint8_t* text, const uint64_t* rec_offsets,
                    size_t n_records, const uint64_t* group_offsets, size_t n_groups, const uint32_t* pairs, size_t n_pairs,
                    const uint8_t* codes, uint32_t* out);  /* host buffers, synchronous */

/* The same for patterns of 1 .. TXQ_EDIT_LONG_MAX_PATTERN bytes (`tetrex search --verify` sends records of 513 .. 4096 letters
 * here; DESIGN.md §12 "Long patterns").  Arguments, semantics, results, the refusal marker (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFE),
 * the size limits and the promises of the _device call — nothing allocated, nothing read back, nothing waited for, no load
 * outside a buffer — are those of txq_edit_search / txq_edit_search_device above, word for word; only the limit on m differs:
 * txq_edit_search_long returns TXQ_ERR_ARG for m = 0, m > TXQ_EDIT_LONG_MAX_PATTERN or a pair that names a missing pattern or
 * group, the _device call marks such a pair in its result and answers the others.  Short patterns are accepted too (slower than
 * above: a pattern of any length up to 1024 bytes occupies 16 lanes), so the two kernels can be checked against each other.
 * The pattern's 64-bit words lie over the lanes of a wave, one word per lane, which is where the limit of 64 x 64 bytes comes
 * from; longer patterns: txh_edit_search of include/txh.h.
 * d_workspace: TXQ_EDIT_LONG_WORKSPACE(n_pairs) bytes of device memory, 8-byte aligned.
 *   TXQ_EDIT_LONG_SPAN=<bytes>   the bytes of text one lane group walks (default 4096, a multiple of 16 in 16 .. 2^20; read at
 *                                every call).  A group re-reads m + min(e, m) bytes in front of its span, 64 / G spans are one
 *                                wave's unit of work (G = 16, 32 or 64 lanes by the pattern's length); the results do not
 *                                depend on it (tests use 64 and 16 to cut small texts into many units). */
#define TXQ_EDIT_LONG_MAX_PATTERN 4096
#define TXQ_EDIT_LONG_WORKSPACE(n_pairs) (16 * (size_t)(n_pairs) + 8)
int txq_edit_search_long_device(const uint8_t* d_patterns, const uint64_t* d_pat_offsets, size_t n_patterns, size_t pattern_bytes,
                                const uint8_t* d_text, const uint64_t* d_rec_offsets, size_t n_records, size_t text_bytes,
                                const uint64_t* d_group_offsets, size_t n_groups, const uint32_t* d_pairs, size_t n_pairs,
                                const uint8_t* d_codes, uint32_t* d_out, void* d_workspace, void* stream);
int txq_edit_search_long(const uint8_t* patterns, const uint64_t* pat_offsets, size_t n_patterns, const uint8_t* text, const uint64_t* rec_offsets,
                         size_t n_records, const uint64_t* group_offsets, size_t n_groups, const uint32_t* pairs, size_t n_pairs,
                         const uint8_t* codes, uint32_t* out);  /* host buffers, synchronous */

/* The same for patterns that are WINDOWS into one letter buffer (`tetrex search --window --verify-windows`; not
 * in the reference).  Window p is d_letters[d_win_begin[p] .. d_win_begin[p] + d_win_len[p]) — the array types of
 * txq_count_windows_device —, n_windows of them in a buffer of letters_bytes bytes.  Windows may overlap, repeat, touch or
 * leave gaps, in any order: the windows of a record are never written out.  Text, records, groups, the class table, the pairs
 * (window, group, cap e), d_out = (d*, r, j), the refusal marker (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFE), the size limits and the
 * promises of the _device call — nothing allocated, nothing read back, nothing waited for, no load outside a buffer whatever
 * the arrays say — are those of txq_edit_search / txq_edit_search_device above.  THE RESULT IS DEFINED AS what txq_edit_search
 * answers with window p written out as pattern p.
 * Windows of 1 .. TXQ_EDIT_MAX_PATTERN bytes run here.  txq_edit_windows_device marks a pair whose window has no letters, more
 * than that, leaves letters_bytes, or whose window or group index is out of range, and answers the others; txq_edit_windows
 * checks its host buffers first as txq_edit_search does (TXQ_ERR_ARG, nothing launched).
 * Consecutive pairs of one group whose windows have the same number of 64-bit words (1, 2, 4 or 8: up to 64, 128, 256, 512
 * letters) walk the group's text TOGETHER, up to 4 of them (2 at 4 words, 1 at 8): a lane loads and classifies each byte once
 * and steps every pair's state.  A caller gains that by putting the windows of a record that go to one group side by side;
 * the arrangement of the pairs changes speed, never results.
 * d_workspace: TXQ_EDIT_WINDOWS_WORKSPACE(n_pairs) bytes of device memory, 8-byte aligned (a key and a unit count per pair).
 *   TXQ_EDIT_CHUNK=<bytes>             as for txq_edit_search above; the lead-in is the largest of the pairs that walk together.
 *   TXQ_EDIT_WINDOWS_BUNDLE=1|2|4      the most pairs that walk together (read at every call; 1: every pair walks alone, as
 *                                      in txq_edit_search_device).  Unset: 4, the fastest measured, in a call of at least 8192
 *                                      pairs, and 1 in a smaller one, where every pair has a wave of its own and walking
 *                                      together only makes a wave's path longer.  The results do not depend on it. */
#define TXQ_EDIT_WINDOWS_WORKSPACE(n_pairs) (16 * (size_t)(n_pairs) + 8)
int txq_edit_windows_device(const uint8_t* d_letters, size_t letters_bytes, const uint64_t* d_win_begin, const uint32_t* d_win_len, size_t n_windows,
                            const uint8_t* d_text, const uint64_t* d_rec_offsets, size_t n_records, size_t text_bytes,
                            const uint64_t* d_group_offsets, size_t n_groups, const uint32_t* d_pairs, size_t n_pairs,
                            const uint8_t* d_codes, uint32_t* d_out, void* d_workspace, void* stream);
int txq_edit_windows(const uint8_t* letters, size_t letters_bytes, const uint64_t* win_begin, const uint32_t* win_len, size_t n_windows,
                     const uint8_t* text, const uint64_t* rec_offsets, size_t n_records, const uint64_t* group_offsets, size_t n_groups,
                     const uint32_t* pairs, size_t n_pairs, const uint8_t* codes, uint32_t* out);  /* host buffers, synchronous */

/* Every record of a group that a pattern matches within its cap (`tetrex search --verify --all-targets`; not in
 * the reference).  Classes, Sellers' D, patterns, records, groups, pairs (pattern, group, cap e) and the refusal rules are
 * those of txq_edit_search above, word for word.  A HIT of pair i is a record r of its group, empty ones included, with
 * d(P, r) = min_j D[m][j] <= e: the quadruple (i, d, r, j), j the lowest end position in r that reaches d, 0 for an empty
 * match — so m <= e makes every record of the group a hit of distance at most m, and an empty record the hit (m, r, 0).
 * The hits are listed by pair, then by record index; no atomic append, the order does not depend on scheduling (the rule of
 * txq_hit_list_device below).  The least (d, r, j) of a pair's hits, d first, then r, is exactly what txq_edit_search* answers
 * for the pair, and a pair of no hit is the pair that gets "none" there.
 * In place of d_out the calls take
 *   d_hits, capacity   room for `capacity` quadruples of u32 (pair, d, r, j);
 *   d_total            one u64: the number of hits whatever the capacity.  At most `capacity` are written, the first ones in
 *                      order; the caller retries with a larger list;
 *   d_status           one u32 per pair: 0 where the pair was answered, 0xFFFFFFFE where it was refused — an index or an
 *                      offset outside its array, m = 0 or above the limit, or slots that do not fit (next).  A refused pair
 *                      contributes no hit;
 *   n_slots            a slot is one 64-bit key per (pair, record of its group) and lives in the workspace.  The pairs'
 *                      slots lie one behind the other in pair order; a pair whose slots would end beyond n_slots is refused
 *                      — and so is every pair behind it, one whose group has no records included: its (empty) slots
 *                      lie beyond n_slots as well.  The caller knows the sum over its pairs of the
 *                      records of their groups from the group offsets it already has;
 *   d_workspace        TXQ_EDIT_TARGETS_WORKSPACE(n_pairs, n_slots) bytes of device memory, 8-byte aligned.
 * txq_edit_targets_device takes patterns of 1 .. TXQ_EDIT_MAX_PATTERN bytes, txq_edit_targets_long_device of 1 ..
 * TXQ_EDIT_LONG_MAX_PATTERN (longer ones: txh_edit_targets of include/txh.h, the same semantics on the host).  The promises of
 * the sibling _device calls hold: nothing allocated, nothing read back, nothing waited for, and no load or store outside a
 * buffer whatever offsets and pairs say; TXQ_ERR_ARG only for what the call can see (null pointers, the size limits: those of
 * txq_edit_search_device, and at most 2^38 slots and rows).  txq_edit_targets and txq_edit_targets_long are the synchronous
 * twins on host buffers; they check them first as txq_edit_search does (TXQ_ERR_ARG, nothing launched) and copy back the
 * total, the status words and the rows written.  TXQ_EDIT_CHUNK and TXQ_EDIT_LONG_SPAN cut the text as they do for the search
 * calls; the results do not depend on them. */
#define TXQ_EDIT_TARGETS_WORKSPACE(n_pairs, n_slots) (8 * (2 * (size_t)(n_pairs) + (size_t)(n_slots) + (size_t)(n_slots) / 256 + 4))
int txq_edit_targets_device(const uint8_t* d_patterns, const uint64_t* d_pat_offsets, size_t n_patterns, size_t pattern_bytes,
                            const uint8_t* d_text, const uint64_t* d_rec_offsets, size_t n_records, size_t text_bytes,
                            const uint64_t* d_group_offsets, size_t n_groups, const uint32_t* d_pairs, size_t n_pairs,
                            const uint8_t* d_codes, uint32_t* d_hits, size_t capacity, uint64_t* d_total, uint32_t* d_status, size_t n_slots,
                            void* d_workspace, void* stream);
int txq_edit_targets_long_device(const uint8_t* d_patterns, const uint64_t* d_pat_offsets, size_t n_patterns, size_t pattern_bytes,
                                 const uint8_t* d_text, const uint64_t* d_rec_offsets, size_t n_records, size_t text_bytes,
                                 const uint64_t* d_group_offsets, size_t n_groups, const uint32_t* d_pairs, size_t n_pairs,
                                 const uint8_t* d_codes, uint32_t* d_hits, size_t capacity, uint64_t* d_total, uint32_t* d_status, size_t n_slots,
                                 void* d_workspace, void* stream);
int txq_edit_targets(const uint8_t* patterns, const uint64_t* pat_offsets, size_t n_patterns, const uint8_t* text, const uint64_t* rec_offsets,
                     size_t n_records, const uint64_t* group_offsets, size_t n_groups, const uint32_t* pairs, size_t n_pairs, const uint8_t* codes,
                     uint32_t* hits, size_t capacity, uint64_t* total, uint32_t* status, size_t n_slots);  /* host buffers, synchronous */
int txq_edit_targets_long(const uint8_t* patterns, const uint64_t* pat_offsets, size_t n_patterns, const uint8_t* text, const uint64_t* rec_offsets,
                          size_t n_records, const uint64_t* group_offsets, size_t n_groups, const uint32_t* pairs, size_t n_pairs, const uint8_t* codes,
                          uint32_t* hits, size_t capacity, uint64_t* total, uint32_t* status, size_t n_slots);  /* host buffers, synchronous */

/* Where a confirmed match begins, and its alignment (`tetrex search --verify --align`; not in the reference).
 * Take a pair (pattern P of m bytes, group, cap) of txq_edit_search* above, its result (d, r, j) with d != 0xFFFFFFFF, R = record
 * r, the class table and Sellers' D as defined there (D[0][.] = 0, D[.][0] = i).  The alignment of the pair is the path found
 * by walking back from (i, j') = (m, j) until i = 0, at each cell taking the FIRST rule that holds:
 *   1. diagonal: j' > 0 and D[i-1][j'-1] + c = D[i][j'], c = 0 if P[i-1] and R[j'-1] match, else 1: operation '=' where c = 0,
 *      'X' where c = 1; then i--, j'--;
 *   2. up: D[i-1][j'] + 1 = D[i][j']: operation 'I', a pattern letter with no target letter; then i--;
 *   3. left: operation 'D', a target letter skipped; then j'--.
 * `start` is the j' at which i reaches 0 — the bytes of R in front of the match, which is R[start .. j) — and the operations,
 * read from the pattern's first letter to its last, are run-length encoded.  There are at most 2 d + 1 runs; the '=', 'X' and
 * 'D' lengths sum to j - start, the '=', 'X' and 'I' lengths to m, the 'X', 'I' and 'D' lengths to d.  A byte of no class
 * matches nothing, itself included, so it gives 'X'.
 * Arguments: the pattern, text and group buffers and the d_pairs of the search call, the d_out it wrote (read on the device:
 * queue this call behind the search call on the same stream; no host round trip is needed in between), the class table, and
 * max_errors, which sizes the answers: pair i owns d_align[i * TXQ_EDIT_ALIGN_STRIDE(max_errors) ..), u32 words
 *     start, n_runs, then n_runs runs as (length << 2) | op with op 0 '=', 1 'X', 2 'I', 3 'D'; the other run words are zero.
 * A pair whose result is "none" gets start = 0xFFFFFFFF, n_runs = 0 and zero run words; a pair that carries the search calls'
 * refusal marker, or that this call's own checks refuse (a pattern or group out of range, an empty pattern, offsets that leave
 * their array), gets start = 0xFFFFFFFF, n_runs = 0xFFFFFFFE and zero run words.  A pair the device does not align gets start =
 * 0xFFFFFFFE and NOTHING else of its words is written: d > TXQ_EDIT_ALIGN_MAX_DISTANCE (the 2 d + 1 diagonals of the walk are
 * the lanes of one wave), d > max_errors, m > TXQ_EDIT_LONG_MAX_PATTERN — the caller takes these to txh_edit_align of
 * include/txh.h, the same semantics on the host with no limit on m or d —, and a triple that is not a cell of the pair's matrix
 * (the triples are device data: a record outside the group, an end beyond the record, d > m, D[m][j] != d).  Whatever the
 * offsets and the triples say, no load or store leaves a buffer.  The result is deterministic; the call allocates nothing,
 * reads nothing back and does not synchronise with the host.  max_errors is at most TXQ_EDIT_ALIGN_MAX_ERRORS (TXQ_ERR_ARG).
 * d_workspace: TXQ_EDIT_ALIGN_WORKSPACE(n_pairs) bytes — none: a wave keeps the direction bits of its pair in LDS (16 bytes a
 * pattern letter), so the argument may be null and nothing of it is touched; it is there for the shape the sibling calls have.
 * txq_edit_align is the synchronous twin on host buffers; it checks them first as txq_edit_search does (any m >= 1 passes: a
 * long pattern is declined, not refused).  A declined pair's words behind the marker keep what `align` held. */
#define TXQ_EDIT_ALIGN_MAX_DISTANCE 31
#define TXQ_EDIT_ALIGN_MAX_ERRORS (1u << 24)
#define TXQ_EDIT_ALIGN_STRIDE(max_errors) (2 * (size_t)(max_errors) + 3)
#define TXQ_EDIT_ALIGN_WORKSPACE(n_pairs) ((size_t)0)
int txq_edit_align_device(const uint8_t* d_patterns, const uint64_t* d_pat_offsets, size_t n_patterns, size_t pattern_bytes,
                          const uint8_t* d_text, const uint64_t* d_rec_offsets, size_t n_records, size_t text_bytes,
                          const uint64_t* d_group_offsets, size_t n_groups, const uint32_t* d_pairs, size_t n_pairs, const uint32_t* d_out,
                          const uint8_t* d_codes, uint32_t max_errors, uint32_t* d_align, void* d_workspace, void* stream);
int txq_edit_align(const uint8_t* patterns, const uint64_t* pat_offsets, size_t n_patterns, const uint8_t* text, const uint64_t* rec_offsets,
                   size_t n_records, const uint64_t* group_offsets, size_t n_groups, const uint32_t* pairs, size_t n_pairs, const uint32_t* results,
                   const uint8_t* codes, uint32_t max_errors, uint32_t* align);  /* host buffers, synchronous */

/* The same for patterns that are WINDOWS into one letter buffer and texts behind a TABLE OF VIEWS (`tetrex search --window
 * --verify-windows --align-windows` and its frame-window sibling; not in the reference).  Window p is
 * d_letters[d_win_begin[p] .. d_win_begin[p] + d_win_len[p]), as txq_edit_windows_device takes them: in any order, overlapping,
 * repeated.  View g is d_views[g]: the records of one bin, wherever the caller keeps them, so ONE call aligns pairs of any number
 * of bins.  Pair i is d_pairs[3 i ..] = (window, view, cap); the view is ONE group, all its records.  d_results[3 i ..] is the
 * triple (d, r, j) a search call answered for that window against that view, r an index into the view's offsets; "none" and the
 * refusal marker pass through as in txq_edit_align_device.  The answers, their stride, the markers and max_errors are
 * txq_edit_align_device's, word for word.  THE RESULT IS DEFINED AS what txq_edit_align answers with the window written out as
 * the pattern and the view's records as the one group of a text of its own.
 * Windows of 1 .. TXQ_EDIT_MAX_PATTERN letters run here; a longer one is declined (start = 0xFFFFFFFE, nothing else written):
 * the caller takes it to txh_edit_align.  A pair is refused (start = 0xFFFFFFFF, n_runs = 0xFFFFFFFE, zero run words) when its
 * window index is >= n_windows, its view index >= n_views, its window empty or leaving letters_bytes.  A triple that is not a
 * cell of the pair's matrix is declined as there: r >= the view's n_records, offsets that leave text_bytes or do not ascend, j
 * beyond the record, d > m, d > TXQ_EDIT_ALIGN_MAX_DISTANCE, d > max_errors, D[m][j] != d.
 * The view table's CONTENTS (pointers and sizes) are the caller's word, like any pointer argument; everything read THROUGH them
 * is device data: no load or store leaves [d_text, d_text + text_bytes), the view's n_records + 1 offsets, letters_bytes or the
 * pair's own answer words, whatever arrays and triples say.  TXQ_ERR_ARG only for what the call can see: null pointers, more
 * than 2^31 - 1 pairs, max_errors above TXQ_EDIT_ALIGN_MAX_ERRORS.  One launch, one wave per pair; the call allocates nothing,
 * reads nothing back and waits for nothing.  d_workspace: TXQ_EDIT_ALIGN_WINDOWS_WORKSPACE(n_pairs) bytes — none, the direction
 * bits stay in LDS; the argument may be null.
 * txq_edit_align_windows is the synchronous twin: `views` is a host array of views that hold HOST pointers.  It checks its
 * buffers first as txq_edit_windows does (TXQ_ERR_ARG, nothing launched; a view's offsets ascend and end within text_bytes; a
 * window above TXQ_EDIT_MAX_PATTERN passes: it is declined, not refused), stages all texts into one allocation, builds the device
 * table and copies the answers back.  A declined pair's words behind the marker keep what `align` held. */
typedef struct txq_text_view {      /* the records of one bin */
    const uint8_t*  d_text;         /* records back to back */
    const uint64_t* d_rec_offsets;  /* n_records + 1 ascending offsets into d_text */
    uint64_t n_records, text_bytes;
} txq_text_view;
#define TXQ_EDIT_ALIGN_WINDOWS_WORKSPACE(n_pairs) ((size_t)0)
int txq_edit_align_windows_device(const uint8_t* d_letters, size_t letters_bytes, const uint64_t* d_win_begin, const uint32_t* d_win_len, size_t n_windows,
                                  const txq_text_view* d_views, size_t n_views, const uint32_t* d_pairs, size_t n_pairs, const uint32_t* d_results,
                                  const uint8_t* d_codes, uint32_t max_errors, uint32_t* d_align, void* d_workspace, void* stream);
int txq_edit_align_windows(const uint8_t* letters, size_t letters_bytes, const uint64_t* win_begin, const uint32_t* win_len, size_t n_windows,
                           const txq_text_view* views, size_t n_views, const uint32_t* pairs, size_t n_pairs, const uint32_t* results,
                           const uint8_t* codes, uint32_t max_errors, uint32_t* align);  /* host views, synchronous */

/* Every record of a view that a WINDOW matches within its cap, for pairs of any number of bins in ONE call (`tetrex search
 * --window --verify-windows --window-targets` and its frame-window sibling; not in the reference).  Windows are
 * taken as txq_edit_windows_device takes them: window p is d_letters[d_win_begin[p] .. d_win_begin[p] + d_win_len[p]), in any
 * order, overlapping, repeated.  Texts are taken as txq_edit_align_windows_device takes them: view g is d_views[g], the records of
 * one bin wherever the caller keeps them; pair i is d_pairs[3 i ..] = (window, view, cap e), the view being ONE group of all its
 * records.  The answers are those of txq_edit_targets_device above, word for word: the hit list (pair, d, r, j) by pair, then by
 * record — r an index into the view's offsets —, d_total, d_status, and slots in pair order — a pair needs one per record of
 * its view — with the same rule: a pair whose slots would end beyond n_slots is refused, and so is every pair behind it.
 * THE RESULT IS DEFINED AS what txq_edit_targets answers with the window written out as the pattern and the view's records as
 * the one group of a text of its own.
 * Windows of 1 .. TXQ_EDIT_MAX_PATTERN letters run here.  A pair is refused (status 0xFFFFFFFE, no hit) when its window index is
 * >= n_windows, its view index >= n_views, its window empty, longer than that or leaving letters_bytes, or when the view's
 * offsets leave text_bytes or its ends do not ascend (d_rec_offsets[0] <= d_rec_offsets[n_records] <= text_bytes is what is
 * checked; offsets in between that do not ascend give hits that mean nothing, and no access outside a buffer).  A view of no
 * records is answered: no slots, no hits.
 * The promises of the sibling _device calls hold word for word: nothing allocated, nothing read back, nothing waited for, no
 * atomic append — the order of the rows does not depend on scheduling.  The view table's CONTENTS (pointers and sizes) are the
 * caller's word, like any pointer argument; everything read THROUGH them is device data: no load or store leaves [d_text,
 * d_text + text_bytes), the view's n_records + 1 offsets, letters_bytes, the slots or the hit list, whatever arrays and pairs
 * say.  TXQ_ERR_ARG only for what the call can see: null pointers, a workspace that is not 8-byte aligned, more than 2^31 - 1
 * pairs, 2^38 slots or rows and more.  d_workspace: TXQ_EDIT_WINDOW_TARGETS_WORKSPACE(n_pairs, n_slots) bytes of device
 * memory, 8-byte aligned.  Every pair walks its view's text alone (no bundles as in txq_edit_windows_device).
 * txq_edit_window_targets is the synchronous twin: `views` is a host array of views that hold HOST pointers.  It checks its
 * buffers first (TXQ_ERR_ARG, nothing launched: every pair's window and view in range, windows of 1 .. TXQ_EDIT_MAX_PATTERN
 * letters inside letters_bytes, every view's offsets ascending within text_bytes), stages all texts into one allocation, builds
 * the device table and copies back the total, the status words and the rows written.
 *   TXQ_EDIT_CHUNK=<bytes>   cuts the text as for txq_edit_search above; the results do not depend on it. */
#define TXQ_EDIT_WINDOW_TARGETS_WORKSPACE(n_pairs, n_slots) (8 * (2 * (size_t)(n_pairs) + (size_t)(n_slots) + (size_t)(n_slots) / 256 + 4))
int txq_edit_window_targets_device(const uint8_t* d_letters, size_t letters_bytes, const uint64_t* d_win_begin, const uint32_t* d_win_len, size_t n_windows,
                                   const txq_text_view* d_views, size_t n_views, const uint32_t* d_pairs, size_t n_pairs, const uint8_t* d_codes,
                                   uint32_t* d_hits, size_t capacity, uint64_t* d_total, uint32_t* d_status, size_t n_slots, void* d_workspace,
                                   void* stream);
int txq_edit_window_targets(const uint8_t* letters, size_t letters_bytes, const uint64_t* win_begin, const uint32_t* win_len, size_t n_windows,
                            const txq_text_view* views, size_t n_views, const uint32_t* pairs, size_t n_pairs, const uint8_t* codes, uint32_t* hits,
                            size_t capacity, uint64_t* total, uint32_t* status, size_t n_slots);  /* host views, synchronous */

/* Which records of a bin does a regular expression match?  (`tetrex query --gpu-verify`; not in the reference.)
 * An automaton is a blob of include/txq_regex.h, where its layout and the meaning of "matches" are stated (as code: the
 * kernel, the host twin txh_regex_filter of include/txh.h and the tests run the same inline interpreter).  Automaton p is
 * d_automata[d_auto_offsets[p] .. d_auto_offsets[p+1]) — n + 1 ascending offsets, each a multiple of 16, d_automata itself
 * 16-byte aligned —, record r is d_text[d_rec_offsets[r] .. d_rec_offsets[r+1]) (records back to back), group g — one bin — is
 * records d_group_offsets[g] .. d_group_offsets[g+1] - 1.  Pair i is d_pairs[2 i .. 2 i + 1] = (automaton, group).  Its answer
 * is a bitmap of ceil(records of the group / 32) u32 words at d_out[d_out_offsets[i]]: bit j of word w is set iff the
 * automaton matches record d_group_offsets[g] + 32 w + j.  The call zeroes d_out[0 .. out_words) itself (bitmaps may not
 * overlap), and d_status[i] = 0 where pair i was answered, TXQ_REGEX_REFUSED where it was not: an automaton or a group out
 * of range, offsets that leave their arrays (automata_bytes / text_bytes / n_records / out_words are the sizes), an automaton
 * that is not 16-byte aligned or whose header is malformed.  A refused pair sets no bit; whatever the buffers hold, no load
 * leaves them (a class or a transition outside an automaton's tables reads as the dead state).
 * An automaton whose lmax is TXQ_REGEX_UNBOUNDED is run over a record by ONE lane, so a record of more than
 * TXQ_REGEX_MAX_SERIAL bytes is flagged without being looked at: a set bit then means "matches, or too long to tell", which
 * is what a caller that confirms flagged records on the host needs.  Bounded automata are exact at any record length.
 * txq_regex_filter checks its host buffers first (offsets that do not ascend, pairs out of range, malformed automata, every
 * table entry, bitmaps outside the output, null pointers: TXQ_ERR_ARG, nothing launched).  txq_regex_filter_device returns
 * TXQ_ERR_ARG only for what it can see (null pointers, alignment, more than 2^31 pairs or 2^32 - 2 records) and the kernels check
 * the rest.  d_workspace: TXQ_REGEX_WORKSPACE(n_pairs) bytes of device memory, 8-byte aligned, the caller's (a unit count per
 * pair while the call runs).  The call allocates nothing and does not synchronise with the host.
 *   TXQ_REGEX_CHUNK=<bytes>       the bytes of text one lane owns (default 256, a multiple of 16 in 16 .. 2^20; read at every
 *                                 call).  256 chunks are one workgroup's unit of work, for which it loads the automaton into
 *                                 LDS once; a lane re-reads lmax - 1 bytes in front of its chunk.  The results do not depend
 *                                 on it (tests use 16).
 *   TXQ_REGEX_MAX_SERIAL=<bytes>  the longest record an unbounded automaton is run over (default 65536; read at every call). */
#define TXQ_REGEX_REFUSED 0xFFFFFFFEu
#define TXQ_REGEX_WORKSPACE(n_pairs) (8 * (size_t)(n_pairs) + 8)
int txq_regex_filter_device(const uint8_t* d_automata, const uint64_t* d_auto_offsets, size_t n_automata, size_t automata_bytes,
                            const uint8_t* d_text, const uint64_t* d_rec_offsets, size_t n_records, size_t text_bytes,
                            const uint64_t* d_group_offsets, size_t n_groups, const uint32_t* d_pairs, size_t n_pairs,
                            const uint64_t* d_out_offsets, uint32_t* d_out, size_t out_words, uint32_t* d_status, void* d_workspace,
                            void* stream);
int txq_regex_filter(const uint8_t* automata, const uint64_t* auto_offsets, size_t n_automata, const uint8_t* text, const uint64_t* rec_offsets,
                     size_t n_records, const uint64_t* group_offsets, size_t n_groups, const uint32_t* pairs, size_t n_pairs,
                     const uint64_t* out_offsets, uint32_t* out, size_t out_words, uint32_t* status);  /* host buffers, synchronous */

/* The set bits of a hit matrix (n_queries x words words, as txq_count_device writes it) as a list of (query, bin, count)
 * u32 triples in (query, bin) order: bin = 64 * word + bit — on a column shard the column within the shard —, count =
 * d_counts[query * 64 * words + bin], or 0 where d_counts is NULL.  *d_total receives the number of set bits whatever
 * the capacity; at most `capacity` triples are written (the caller retries with a larger list).  No atomic append: the
 * order does not depend on scheduling.  Asynchronous on `stream`. */
int txq_hit_list_device(const uint64_t* d_hits, const uint32_t* d_counts, size_t n_queries, size_t words, uint32_t* d_list,
                        size_t capacity, uint64_t* d_total, void* stream);

/* Device-side emplace: value i is inserted into bin bins_of[i] (flat IBF only; bins outside this
 * shard's columns are skipped). */
int txq_emplace_device(txq_index* ix, const uint64_t* d_values, const uint32_t* d_bins_of, size_t n, void* stream);

/* Index construction of a size-aware HIBF (`tetrex index --layout sized`, tetrex_amd/csrc/host/layout.hpp).  The input is
 * the k-mer values of every user bin as one CSR array on the device: bin b holds d_values[d_offsets[b] .. d_offsets[b+1]),
 * offsets ascending, n_bins + 1 of them; n_values bounds every index.  A library too large for the device is streamed as
 * chunks (each chunk with offsets of its own over all n_bins bins): both the sketch and the insertion combine with what
 * earlier chunks left (max / OR), so the result does not depend on the chunking.
 *
 * HyperLogLog sketches, TXQ_HLL_REGISTERS u8 registers per bin (d_registers: n_bins x 4096, zeroed by the caller before
 * the first chunk).  With x the splitmix64 finaliser of a value
 *     x ^= x >> 30; x *= 0xbf58476d1ce4e5b9; x ^= x >> 27; x *= 0x94d049bb133111eb; x ^= x >> 31
 * the value sets register x >> 52 to at least min(clz(x << 12), 52) + 1.  The result is the same whatever the scheduling. */
#define TXQ_HLL_BITS 12
#define TXQ_HLL_REGISTERS 4096
int txq_sketch_device(const uint64_t* d_values, size_t n_values, const uint64_t* d_offsets, uint64_t n_bins, uint8_t* d_registers,
                      void* stream);
/* Union estimates over runs of the bins in the order d_order (n_bins bin ids): d_estimates[s * window + L - 1] = the
 * estimate of the union of bins d_order[s .. s+L-1] for L = 1 .. window (0.0 where s + L > n_bins).  The estimate of
 * registers M[0..m), m = 4096: E = alpha_m * m^2 / Z, alpha_m = 0.7213 / (1 + 1.079 / m), Z = sum 2^-M[r] (computed as the
 * exact integer sum of 2^(53 - M[r]), rounded once to a double and scaled by 2^-53); where E <= 2.5 m and V > 0 registers
 * are zero, linear counting m * ln(m / V) replaces it (ln of the host's libm).  window = 1 with the identity order gives
 * each bin's own estimate. */
int txq_union_estimates_device(const uint8_t* d_registers, const uint32_t* d_order, uint64_t n_bins, uint64_t window,
                               double* d_estimates, void* stream);
/* Pairwise union estimates (`tetrex index --layout sized --rearrange`, host/layout.hpp): d_estimates[i * n + j] = the
 * estimate of the union of bins d_ids[i] and d_ids[j] (bin ids into d_registers; they may repeat), by the estimator above, so
 * the diagonal holds each bin's own estimate and the matrix is symmetric.  n = 0 is a no-op; null pointers and n > 4096
 * (one table: 4096^2 doubles at most) are TXQ_ERR_ARG. */
int txq_pair_unions_device(const uint8_t* d_registers, const uint32_t* d_ids, uint64_t n, double* d_estimates, void* stream);
/* Insertion into every IBF of a tree.  d_ibfs[n_ibf]: the IBFs' shapes, each .words a DEVICE pointer to its zeroed
 * [bin_size][bin_words] matrix.  User bin b's path from the root is d_path[3 * e .. 3 * e + 2] = (ibf, first technical bin,
 * parts) for e in [d_path_offsets[b], d_path_offsets[b+1]); only the leaf entry may have parts > 1.  Each value sets, in each
 * IBF on its bin's path, the hash_funs bits of technical bin first + (parts > 1 ? mulhi64(fmix(v ^ 0x9e3779b97f4a7c15), parts)
 * : 0) (fmix: the finaliser above), so a value always lands in the same part.  Entries outside an IBF's bins are skipped. */
int txq_tree_insert_device(const uint64_t* d_values, size_t n_values, const uint64_t* d_offsets, uint64_t n_bins,
                           const uint64_t* d_path_offsets, const uint64_t* d_path, const txq_ibf_desc* d_ibfs, uint64_t n_ibf,
                           void* stream);

/* Mask-DAG programs (format: include/txq_program.h).  Runs n_programs programs found in
 * `blob`; final_masks receives n_programs x shard_words words (host buffer, synchronous). */
int txq_run_programs(txq_index* ix, const void* blob, size_t blob_bytes, size_t n_programs, uint64_t* final_masks);
int txq_run_programs_device(txq_index* ix, const void* blob, size_t blob_bytes, size_t n_programs,
                            uint64_t* d_final_masks, void* stream);

/* Staged execution: the host expands the frontier of a batch of queries piecewise and streams
 * each piece (a blob with the NEW ops of every program; slot contents persist in HBM between
 * stages).  After a stage the library answers n_queries feedback questions "has slot
 * query_slot[i] of program query_program[i] any bit set?" (bitvector::none() of
 * include/otf_collector.h:383) into alive[i]: 0 = none, otherwise 1 + floor(log2(number of bits set in this
 * shard's columns)) — alive or not is all the collector needs; how FULL the surviving masks are tells the host whether
 * state lists saturate on this index (dense DP steps pay) or thin out (pruning pays), so the host can prune dead
 * states before expanding them.  Every stage's blob must hold exactly n_programs programs (possibly with no
 * ops) and their current n_slots.  txq_session_end copies the RESULT slot of every program to
 * final_masks (n_programs x shard_words, host) and destroys the session; a NULL final_masks
 * just destroys it. */
typedef struct txq_session txq_session;
int txq_session_begin(txq_index* ix, size_t n_programs, txq_session** out);
/* Attach the d-gram index of `tetrex query -g` (reference include/otf_collector.h:235,
 * include/dGramIndex.h:279-283): a flat IBF over the same bins, uploaded with the same shard.  The
 * last n_aux_kmers entries of a stage's k-mer table (txq_program.h) are then probed on it. */
int txq_session_set_aux_index(txq_session* s, txq_index* aux);
int txq_session_stage(txq_session* s, const void* blob, size_t blob_bytes, const uint32_t* query_program,
                      const uint32_t* query_slot, size_t n_queries, uint8_t* alive);
int txq_session_end(txq_session* s, uint64_t* final_masks);

/* Plain device-memory helpers so that a host program needs no HIP headers. */
int txq_malloc(void** dptr, size_t bytes);
int txq_free(void* dptr);
int txq_memcpy_h2d(void* dst, const void* src, size_t bytes);
int txq_memcpy_d2h(void* dst, const void* src, size_t bytes);
int txq_synchronize(void);
/* Page-locked host memory (hipHostMalloc): fastest source/destination of the host-buffer entry points. */
int txq_host_alloc(void** ptr, size_t bytes);
int txq_host_free(void* ptr);

#ifdef __cplusplus
}
#endif
#endif /* TXQ_H */
