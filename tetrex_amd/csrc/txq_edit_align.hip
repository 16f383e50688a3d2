// Start and CIGAR of the pairs an edit-distance search confirmed, on gfx950 (txq_edit_align / txq_edit_align_device;
// `tetrex search --verify --align`).  The reference has no counterpart.  The semantics are in include/txq.h,
// the step logic — band, row update, direction bits, walk — in txq_edit_align_plan.hpp, which a CPU test runs as well.
//
// Mapping to the machine:
//   * one wave per pair, block i of the grid being pair i.  The wave reads the pair's triple (d, r, j) from the search call's
//     d_out — device data: align_kind() admits only triples whose every derived index stays inside the record — and a pair
//     with nothing to align writes its marker and returns;
//   * lane k owns diagonal k - d of Sellers' matrix (2 d + 1 <= 63 lanes work), one pattern letter is one step.  Rows come in
//     blocks of 64: each lane fetches one pattern byte and two record bytes (coalesced byte loads, none outside R[0 .. j)) and
//     turns them into classes; inside the block a row's pattern class is read from a uniform lane, the 128 text classes move down
//     by one lane per row, the value from above and the dependency inside the row — at most six steps — are DPP moves, so a
//     row touches the LDS pipeline only to store its direction bits;
//   * a cell's operation is two bits, a row's operations are two ballots, which lane 0 stores in LDS: 16 bytes a row, 64 KiB
//     for m = 4096.  Two instances, one launch each — 512 rows (8 KiB, four blocks and more per CU) and 4096 rows (64 KiB, two
//     per CU) —, a pair runs in the smaller one that holds its pattern; the first instance also writes every marker;
//   * the walk back reads one row per step (all lanes the same address: a broadcast) and is the same in every lane; the run
//     that closes as number q stays in lane q, and at the end lane q stores it to its place, the last-closed run first.
// Nothing is allocated, nothing read back, and the workspace argument is not touched: the direction bits never leave the CU.
//
// txq_edit_align_windows / _device (`tetrex search --verify-windows --align-windows`) is the same kernel behind
// another admit(): the pattern is a window into one letter buffer, the text a view of a table — one per resident bin —, so one
// launch aligns pairs of any number of bins.  Windows of up to 512 letters run: the 8 KiB instance only.
#include <cstddef>

#include "txq_edit_align_plan.hpp"
#include "txq_edit_common.hpp"

namespace txq {
namespace {

constexpr uint32_t kSmallRows = TXQ_EDIT_MAX_PATTERN, kLargeRows = TXQ_EDIT_LONG_MAX_PATTERN;
static_assert(kLargeRows == kAlignMaxPattern && TXQ_EDIT_ALIGN_MAX_DISTANCE == kAlignMaxDistance, "include/txq.h and the plan header agree");
constexpr uint32_t kMaxErrors = TXQ_EDIT_ALIGN_MAX_ERRORS;

struct AlArgs {
    EdArgs e;             // patterns, text, pairs (out, keys, pref unused)
    const uint32_t* res;  // the search call's d_out
    uint32_t* align;
    uint32_t max_errors;
};

// Cross-lane moves as DPP modifiers of a VALU move: no trip through the LDS pipeline, which a shuffle takes and which would
// make every row wait for several of them in turn.
template <int kCtrl, int kRowMask>
__device__ __forceinline__ uint32_t dpp_move(uint32_t x, uint32_t otherwise) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)otherwise, (int)x, kCtrl, kRowMask, 0xF, false);  // a lane without a source keeps `otherwise`
}
// x of lane k + 1; in the wave's last lane `otherwise` (wave_shl:1)
__device__ __forceinline__ uint32_t lane_above(uint32_t x, uint32_t otherwise) { return dpp_move<0x130, 0xF>(x, otherwise); }
// The minimum of x over lanes 0 .. k, for a band of 2 d + 1 lanes: the doubling steps of align_scan_step inside rows of 16 lanes
// (row_shr:1, 2, 4, 8), then the rows joined by lane 15 of each row going to the row behind it (row_bcast:15, rows 1 and 3) and
// lane 31 to the upper half (row_bcast:31).  A step that no lane of the band needs is left out (d is uniform).
__device__ __forceinline__ uint32_t band_prefix_min(uint32_t x, uint32_t d) {
    if (d >= 1) {
        x = align_scan_step(x, dpp_move<0x111, 0xF>(x, kAlignInf));
        x = align_scan_step(x, dpp_move<0x112, 0xF>(x, kAlignInf));
    }
    if (d >= 2) x = align_scan_step(x, dpp_move<0x114, 0xF>(x, kAlignInf));
    if (d >= 4) x = align_scan_step(x, dpp_move<0x118, 0xF>(x, kAlignInf));
    if (d >= 8) x = align_scan_step(x, dpp_move<0x142, 0xA>(x, kAlignInf));
    if (d >= 16) x = align_scan_step(x, dpp_move<0x143, 0xC>(x, kAlignInf));
    return x;
}

// The kernel's one seam: how a pair finds its pattern bytes, its record and the bounds its triple is checked against.
// admit() answers what the triple asks for and, for a pair that runs, m, the pattern's m bytes and the record's first byte.
struct AlignPair {
    AlignKind kind;
    uint32_t m;
    const uint8_t* ptext;  // the pattern: m bytes
    const uint8_t* rtext;  // the record: bytes [0, j) of it are read
};

// a pattern of an offset table against a group of the text (txq_edit_align_device)
__device__ __forceinline__ AlignPair admit(const AlArgs& a, uint64_t pair, uint32_t d, uint32_t r, uint32_t j) {
    const PairView v = view_pair<0xFFFFFFFFu>(a.e, pair);
    const AlignKind kind = !v.ok ? AlignKind::Refused : align_kind(d, r, j, v.m, a.max_errors, a.e.t.rec, v.r0, v.r1, v.gs, v.ge);
    if (kind != AlignKind::Run) return {kind, 0, nullptr, nullptr};
    return {kind, v.m, a.e.pat + v.p0, a.e.t.text + a.e.t.rec[r]};
}
__device__ __forceinline__ const uint8_t* class_table(const AlArgs& a) { return a.e.codes; }

// a window of one letter buffer against a view of a table (txq_edit_align_windows_device): views[g] is read once, uniformly
struct AwArgs {
    const uint8_t* letters;
    uint64_t letters_bytes;
    const uint64_t* win_begin;
    const uint32_t* win_len;
    uint64_t n_win;
    const AlignTextView* views;
    uint64_t n_views;
    const uint32_t* pairs;
    const uint8_t* codes;
    const uint32_t* res;  // one triple per pair, as a search call answered it for the window against the view
    uint32_t* align;
    uint32_t max_errors;
};
static_assert(sizeof(AlignTextView) == sizeof(txq_text_view) && offsetof(AlignTextView, text) == offsetof(txq_text_view, d_text) &&
                  offsetof(AlignTextView, rec) == offsetof(txq_text_view, d_rec_offsets) && offsetof(AlignTextView, n_rec) == offsetof(txq_text_view, n_records) &&
                  offsetof(AlignTextView, text_bytes) == offsetof(txq_text_view, text_bytes),
              "include/txq.h and the plan header agree on a view");

__device__ __forceinline__ AlignPair admit(const AwArgs& a, uint64_t pair, uint32_t d, uint32_t r, uint32_t j) {
    const uint32_t p = a.pairs[3 * pair], g = a.pairs[3 * pair + 1];
    if (!align_window_ok(p, g, a.n_win, a.n_views, a.win_begin, a.win_len, a.letters_bytes)) return {AlignKind::Refused, 0, nullptr, nullptr};
    const AlignTextView v = a.views[g];
    const uint32_t m = a.win_len[p];
    const AlignKind kind = align_window_kind(d, r, j, m, a.max_errors, v);
    if (kind != AlignKind::Run) return {kind, 0, nullptr, nullptr};
    return {kind, m, a.letters + a.win_begin[p], v.text + v.rec[r]};
}
__device__ __forceinline__ const uint8_t* class_table(const AwArgs& a) { return a.codes; }

template <uint32_t kRows, class Args>
__global__ __launch_bounds__(64) void edit_align_kernel(Args a) {
    __shared__ uint64_t dir[2 * kRows];  // row i: dir[2 (i - 1)] the low bits of its operations, dir[2 (i - 1) + 1] the high bits
    constexpr bool kFirst = kRows == kSmallRows;
    const uint32_t lane = threadIdx.x;
    const uint64_t pair = blockIdx.x;
    const uint32_t run_words = 2 * a.max_errors + 1;
    uint32_t* const out = a.align + pair * (uint64_t)(run_words + 2);
    const uint32_t d = a.res[3 * pair], r = a.res[3 * pair + 1], j = a.res[3 * pair + 2];
    const AlignPair v = admit(a, pair, d, r, j);
    const AlignKind kind = v.kind;
    if (kind != AlignKind::Run) {
        if (!kFirst) return;
        if (kind == AlignKind::Declined) {
            if (lane == 0) out[0] = kAlignDeclined;
            return;
        }
        if (lane == 0) out[0] = kAlignNone, out[1] = kind == AlignKind::Refused ? kAlignDeclined : 0u;
        for (uint32_t x = lane; x < run_words; x += 64) out[2 + x] = 0;
        return;
    }
    const uint32_t m = v.m;
    if ((m <= kSmallRows) != kFirst) return;  // (uniform over the wave)

    const AlignBand b{m, d, j};
    const uint8_t* const rtext = v.rtext;
    const uint8_t* const ptext = v.ptext;
    const uint8_t* const codes = class_table(a);
    const uint32_t k = lane;
    uint32_t prev = align_row0(b, k);
    for (uint32_t i0 = 0; i0 < m; i0 += 64) {
        uint32_t pc = 31, ta = 31, tb = 31;
        if (i0 + lane < m) pc = codes[ptext[i0 + lane]];
        const int64_t xa = align_text_index(b, i0, lane), xb = xa + 64;
        if (xa >= 0 && xa < (int64_t)j) ta = codes[rtext[xa]];
        if (xb >= 0 && xb < (int64_t)j) tb = codes[rtext[xb]];
        const uint32_t rows = m - i0 < 64 ? m - i0 : 64;
        for (uint32_t ii = 0; ii < rows; ++ii) {
            const uint32_t i = i0 + ii + 1;
            const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)pc, (int)ii);
            const bool match = p < 31 && p == ta;  // (ta: byte number ii + k of the block's 128, see below)
            const uint32_t above = lane_above(prev, kAlignInf);
            const uint32_t up = k < 2 * d ? above : kAlignInf;
            const int64_t col = align_column(b, i, k);
            const bool in_band = align_in_band(b, k, col);
            const uint32_t x = band_prefix_min(align_scan_bias(align_cell(in_band, col, i, up, prev, match), k), d);
            const uint32_t val = align_scan_value(in_band, x, k);
            const uint32_t op = align_op(col, val, up, prev, match);
            const uint64_t lo = __ballot(op & 1), hi = __ballot(op >> 1);
            if (lane == 0) dir[2 * (i - 1)] = lo, dir[2 * (i - 1) + 1] = hi;
            prev = val;
            // the 128 bytes move down by one lane: lane k now holds byte number ii + 1 + k
            ta = lane_above(ta, (uint32_t)__builtin_amdgcn_readfirstlane((int)tb));
            tb = lane_above(tb, 31u);
        }
    }
    __syncthreads();
    // (m, j) of the band holds d exactly where the triple is a cell of the matrix; anything else is declined
    bool lost = __shfl(prev, d) != d;
    AlignWalk w = align_walk_begin(b);
    uint32_t mine = 0;
    while (!lost && w.i > 0) {
        const uint32_t closed = align_walk_step(w, dir[2 * (w.i - 1)], dir[2 * (w.i - 1) + 1]);
        if (closed && lane == w.n_runs - 1) mine = closed;
        lost = align_walk_lost(w, b) || w.n_runs > 2 * d;  // (a run more is still to close)
    }
    const int64_t start = align_column(b, 0, w.k);
    if (lost || start < 0) {
        if (lane == 0) out[0] = kAlignDeclined;
        return;
    }
    const uint32_t last = align_walk_end(w);
    if (lane == w.n_runs - 1) mine = last;
    if (lane == 0) out[0] = (uint32_t)start, out[1] = w.n_runs;
    if (lane < w.n_runs) out[2 + align_run_slot(w.n_runs, lane)] = mine;
    for (uint32_t x = w.n_runs + lane; x < run_words; x += 64) out[2 + x] = 0;
}

int align_device_args(const uint8_t* d_patterns, const uint64_t* d_pat_offsets, size_t pattern_bytes, const uint8_t* d_text,
                      const uint64_t* d_rec_offsets, size_t n_records, size_t text_bytes, const uint64_t* d_group_offsets, const uint32_t* d_pairs,
                      size_t n_pairs, const uint32_t* d_out, const uint8_t* d_codes, uint32_t max_errors, const uint32_t* d_align) {
    if (max_errors > kMaxErrors) return fail(TXQ_ERR_ARG, "max_errors is at most %u", kMaxErrors);
    if (int rc = edit_args(d_pat_offsets, d_rec_offsets, d_group_offsets, d_pairs, n_pairs, n_records, text_bytes, d_codes, d_out)) return rc;
    if (n_pairs && !d_align) return fail(TXQ_ERR_ARG, "null argument");
    if ((pattern_bytes && !d_patterns) || (text_bytes && !d_text)) return fail(TXQ_ERR_ARG, "null argument");
    return require_init();
}

}  // namespace
}  // namespace txq

using namespace txq;

extern "C" {

int txq_edit_align_device(const uint8_t* d_patterns, const uint64_t* d_pat_offsets, size_t n_patterns, size_t pattern_bytes,
                          const uint8_t* d_text, const uint64_t* d_rec_offsets, size_t n_records, size_t text_bytes,
                          const uint64_t* d_group_offsets, size_t n_groups, const uint32_t* d_pairs, size_t n_pairs, const uint32_t* d_out,
                          const uint8_t* d_codes, uint32_t max_errors, uint32_t* d_align, void* d_workspace, void* stream) {
    (void)d_workspace;  // TXQ_EDIT_ALIGN_WORKSPACE is 0: the direction bits live in LDS
    if (int rc = align_device_args(d_patterns, d_pat_offsets, pattern_bytes, d_text, d_rec_offsets, n_records, text_bytes, d_group_offsets, d_pairs,
                                   n_pairs, d_out, d_codes, max_errors, d_align))
        return rc;
    if (n_pairs == 0) return TXQ_OK;
    hipStream_t st = (hipStream_t)stream;
    const AlArgs a{{d_patterns, d_pat_offsets, n_patterns, pattern_bytes, {d_text, d_rec_offsets, n_records, text_bytes, d_group_offsets, n_groups},
                    d_pairs, n_pairs, d_codes, nullptr, nullptr, nullptr, 0},
                   d_out, d_align, max_errors};
    edit_align_kernel<kSmallRows, AlArgs><<<(unsigned)n_pairs, 64, 0, st>>>(a);
    edit_align_kernel<kLargeRows, AlArgs><<<(unsigned)n_pairs, 64, 0, st>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "edit align kernel launch");
    return TXQ_OK;
}

int txq_edit_align(const uint8_t* patterns, const uint64_t* pat_offsets, size_t n_patterns, const uint8_t* text, const uint64_t* rec_offsets,
                   size_t n_records, const uint64_t* group_offsets, size_t n_groups, const uint32_t* pairs, size_t n_pairs, const uint32_t* results,
                   const uint8_t* codes, uint32_t max_errors, uint32_t* align) {
    if (!pat_offsets || !rec_offsets || !group_offsets) return fail(TXQ_ERR_ARG, "null argument");
    if (max_errors > kMaxErrors) return fail(TXQ_ERR_ARG, "max_errors is at most %u", kMaxErrors);
    if (int rc = check_ascending(pat_offsets, n_patterns, "pattern")) return rc;
    if (int rc = check_ascending(rec_offsets, n_records, "record")) return rc;
    if (int rc = check_ascending(group_offsets, n_groups, "group", "records", n_records)) return rc;
    const uint64_t pat0 = pat_offsets[0], pat_bytes = pat_offsets[n_patterns] - pat0;
    const uint64_t text0 = rec_offsets[0], text_bytes = rec_offsets[n_records] - text0;
    if (int rc = edit_args(pat_offsets, rec_offsets, group_offsets, pairs, n_pairs, n_records, text_bytes, codes, results)) return rc;
    if ((n_pairs && !align) || (pat_bytes && !patterns) || (text_bytes && !text)) return fail(TXQ_ERR_ARG, "null argument");
    for (size_t i = 0; i < n_pairs; ++i) {
        const uint32_t p = pairs[3 * i], g = pairs[3 * i + 1];
        if (p >= n_patterns || g >= n_groups) return fail(TXQ_ERR_ARG, "pair %zu names pattern %u of %zu, group %u of %zu", i, p, n_patterns, g, n_groups);
        if (pat_offsets[p + 1] == pat_offsets[p]) return fail(TXQ_ERR_ARG, "pair %zu: an empty pattern", i);
    }
    if (int rc = require_init()) return rc;
    if (n_pairs == 0) return TXQ_OK;
    const size_t stride = TXQ_EDIT_ALIGN_STRIDE(max_errors);
    DeviceStage d;
    const size_t s_pat = d.add(pat_bytes + 16), s_po = d.add((n_patterns + 1) * 8), s_text = d.add(text_bytes + 16), s_rec = d.add((n_records + 1) * 8),
                 s_grp = d.add((n_groups + 1) * 8), s_pairs = d.add(n_pairs * 12), s_codes = d.add(256), s_res = d.add(n_pairs * 12),
                 s_align = d.add(n_pairs * stride * 4);
    if (const hipError_t e = d.alloc(); e != hipSuccess) return fail_hip(e, "hipMalloc");
    const std::vector<uint64_t> po = rebased(pat_offsets, n_patterns), ro = rebased(rec_offsets, n_records);
    d.upload(s_pat, patterns + pat0, pat_bytes);
    d.upload(s_po, po.data(), po.size() * 8);
    d.upload(s_text, text + text0, text_bytes);
    d.upload(s_rec, ro.data(), ro.size() * 8);
    d.upload(s_grp, group_offsets, (n_groups + 1) * 8);
    d.upload(s_pairs, pairs, n_pairs * 12);
    d.upload(s_codes, codes, 256);
    d.upload(s_res, results, n_pairs * 12);
    d.upload(s_align, align, n_pairs * stride * 4);  // (a declined pair keeps what the caller had behind its marker)
    int rc = TXQ_OK;
    if (d.error() == hipSuccess)
        rc = txq_edit_align_device(d.at<uint8_t>(s_pat), d.at<uint64_t>(s_po), n_patterns, pat_bytes, d.at<uint8_t>(s_text), d.at<uint64_t>(s_rec), n_records,
                                   text_bytes, d.at<uint64_t>(s_grp), n_groups, d.at<uint32_t>(s_pairs), n_pairs, d.at<uint32_t>(s_res), d.at<uint8_t>(s_codes),
                                   max_errors, d.at<uint32_t>(s_align), nullptr, nullptr);
    if (rc == TXQ_OK) d.download(align, s_align, n_pairs * stride * 4);  // (waits for the kernels)
    if (d.error() != hipSuccess) return fail_hip(d.error(), "txq_edit_align copies");
    return rc;
}

int txq_edit_align_windows_device(const uint8_t* d_letters, size_t letters_bytes, const uint64_t* d_win_begin, const uint32_t* d_win_len, size_t n_windows,
                                  const txq_text_view* d_views, size_t n_views, const uint32_t* d_pairs, size_t n_pairs, const uint32_t* d_results,
                                  const uint8_t* d_codes, uint32_t max_errors, uint32_t* d_align, void* d_workspace, void* stream) {
    (void)d_workspace;  // TXQ_EDIT_ALIGN_WINDOWS_WORKSPACE is 0: the direction bits live in LDS
    if (max_errors > kMaxErrors) return fail(TXQ_ERR_ARG, "max_errors is at most %u", kMaxErrors);
    if (n_pairs > 0x7FFFFFFFull) return fail(TXQ_ERR_ARG, "at most 2^31 - 1 pairs per call");
    if (!d_codes || (n_pairs && (!d_pairs || !d_results || !d_align)) || (n_windows && (!d_win_begin || !d_win_len)) || (n_views && !d_views) ||
        (letters_bytes && !d_letters))
        return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = require_init()) return rc;
    if (n_pairs == 0) return TXQ_OK;
    const AwArgs a{d_letters, letters_bytes, d_win_begin, d_win_len, n_windows, reinterpret_cast<const AlignTextView*>(d_views), n_views, d_pairs, d_codes,
                   d_results, d_align, max_errors};
    edit_align_kernel<kSmallRows, AwArgs><<<(unsigned)n_pairs, 64, 0, (hipStream_t)stream>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "edit align windows kernel launch");
    return TXQ_OK;
}

int txq_edit_align_windows(const uint8_t* letters, size_t letters_bytes, const uint64_t* win_begin, const uint32_t* win_len, size_t n_windows,
                           const txq_text_view* views, size_t n_views, const uint32_t* pairs, size_t n_pairs, const uint32_t* results, const uint8_t* codes,
                           uint32_t max_errors, uint32_t* align) {
    if (max_errors > kMaxErrors) return fail(TXQ_ERR_ARG, "max_errors is at most %u", kMaxErrors);
    if (n_pairs > 0x7FFFFFFFull) return fail(TXQ_ERR_ARG, "at most 2^31 - 1 pairs per call");
    if (!codes || (n_pairs && (!pairs || !results || !align)) || (n_windows && (!win_begin || !win_len)) || (n_views && !views) || (letters_bytes && !letters))
        return fail(TXQ_ERR_ARG, "null argument");
    // every text at a 16-byte boundary of one slice, every view's offsets behind those of the view before
    std::vector<uint64_t> text_at(n_views), rec_at(n_views);
    uint64_t texts_bytes = 0, n_offsets = 0;
    for (size_t g = 0; g < n_views; ++g) {
        const txq_text_view& v = views[g];
        if (!v.d_rec_offsets || (v.text_bytes && !v.d_text)) return fail(TXQ_ERR_ARG, "null argument");
        if (v.n_records >= 0xFFFFFFFEull) return fail(TXQ_ERR_ARG, "at most 2^32 - 2 records per view");
        if (int rc = check_ascending(v.d_rec_offsets, v.n_records, "record", "text", v.text_bytes)) return rc;
        text_at[g] = texts_bytes, rec_at[g] = n_offsets;
        texts_bytes += (v.text_bytes + 15) & ~(uint64_t)15;
        n_offsets += v.n_records + 1;
    }
    for (size_t i = 0; i < n_pairs; ++i) {
        const uint32_t p = pairs[3 * i], g = pairs[3 * i + 1];
        if (p >= n_windows || g >= n_views) return fail(TXQ_ERR_ARG, "pair %zu names window %u of %zu, view %u of %zu", i, p, n_windows, g, n_views);
        const uint64_t m = win_len[p], b = win_begin[p];
        if (m < 1) return fail(TXQ_ERR_ARG, "pair %zu: an empty window", i);
        if (b > letters_bytes || m > letters_bytes - b) return fail(TXQ_ERR_ARG, "pair %zu: window %u leaves the %zu letters", i, p, letters_bytes);
    }
    if (int rc = require_init()) return rc;
    if (n_pairs == 0) return TXQ_OK;
    const size_t stride = TXQ_EDIT_ALIGN_STRIDE(max_errors);
    DeviceStage d;
    const size_t s_let = d.add(letters_bytes + 16), s_wb = d.add(n_windows * 8 + 8), s_wl = d.add(n_windows * 4 + 4), s_text = d.add(texts_bytes + 16),
                 s_rec = d.add(n_offsets * 8 + 8), s_views = d.add(n_views * sizeof(txq_text_view) + 8), s_pairs = d.add(n_pairs * 12), s_codes = d.add(256),
                 s_res = d.add(n_pairs * 12), s_align = d.add(n_pairs * stride * 4);
    if (const hipError_t e = d.alloc(); e != hipSuccess) return fail_hip(e, "hipMalloc");
    std::vector<txq_text_view> table(n_views);
    for (size_t g = 0; g < n_views; ++g) {
        const txq_text_view& v = views[g];
        d.upload(s_text + text_at[g], v.d_text, v.text_bytes);
        d.upload(s_rec + 8 * rec_at[g], v.d_rec_offsets, (v.n_records + 1) * 8);
        table[g] = {d.at<uint8_t>(s_text) + text_at[g], d.at<uint64_t>(s_rec) + rec_at[g], v.n_records, v.text_bytes};
    }
    d.upload(s_let, letters, letters_bytes);
    d.upload(s_wb, win_begin, n_windows * 8);
    d.upload(s_wl, win_len, n_windows * 4);
    d.upload(s_views, table.data(), n_views * sizeof(txq_text_view));
    d.upload(s_pairs, pairs, n_pairs * 12);
    d.upload(s_codes, codes, 256);
    d.upload(s_res, results, n_pairs * 12);
    d.upload(s_align, align, n_pairs * stride * 4);  // (a declined pair keeps what the caller had behind its marker)
    int rc = TXQ_OK;
    if (d.error() == hipSuccess)
        rc = txq_edit_align_windows_device(d.at<uint8_t>(s_let), letters_bytes, d.at<uint64_t>(s_wb), d.at<uint32_t>(s_wl), n_windows,
                                           d.at<txq_text_view>(s_views), n_views, d.at<uint32_t>(s_pairs), n_pairs, d.at<uint32_t>(s_res), d.at<uint8_t>(s_codes),
                                           max_errors, d.at<uint32_t>(s_align), nullptr, nullptr);
    if (rc == TXQ_OK) d.download(align, s_align, n_pairs * stride * 4);  // (waits for the kernel)
    if (d.error() != hipSuccess) return fail_hip(d.error(), "txq_edit_align_windows copies");
    return rc;
}

}  // extern "C"
