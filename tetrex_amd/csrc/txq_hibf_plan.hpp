// What an HIBF upload sends to the device, worked out on the host: plain C++ on the tree's shape (no HIP, no Index, never
// an IBF's words), so that every array can be checked without a GPU (tests/native/hibf_plan_dump.cpp).  txq_hibf.hip
// hibf_upload calls these in order and uploads what they return; DESIGN.md "HIBF upload" says what each array is for.
//   read_tree           the ONE walk of the tree: validation, flattened maps, levels, parents, BFS order
//   plan_maps           merged / descend masks, identity leaves, the fused descent's node records
//   plan_regular        regular two-level trees: ChildRec table, root record, shape of the interleaved copy
//   plan_layout_order   any other tree: the layout-order row (chunks, gates, paths, leaves, split user bins)
//   plan_subtree_shard  txq_index_upload_subtrees: which IBFs a shard keeps, renumbered, and its maps
// Where a record holds a device address the caller passes the IBFs' descriptors (std::vector<IbfDev>, words included).
#pragma once
#include "txq_records.hpp"
#include "../../include/txq.h"
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <deque>
#include <optional>
#include <string>
#include <utility>

namespace txq {

// (PlanError: txq_records.hpp) a refused tree: TXQ_ERR_ARG, which fault, and the IBF it is about
inline PlanError plan_error(PlanError::Kind kind, uint64_t ibf, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return PlanError{TXQ_ERR_ARG, buf, kind, ibf};
}

// shard r of R owns mask words [lo, hi): as even as possible, earlier shards get the remainder
inline void shard_range(uint64_t words, int r, int R, uint64_t* lo, uint64_t* hi) {
    uint64_t base = words / R, rem = words % R;
    *lo = base * r + (r < (int)rem ? r : rem);
    *hi = *lo + base + (r < (int)rem ? 1 : 0);
}

// rows of `shard_words` words in HBM: an even number of words (16-byte lane accesses) unless there is only one
inline uint32_t row_stride(uint32_t shard_words) { return shard_words <= 1 ? 1u : ((shard_words + 1u) & ~1u); }

// the descriptor of column slice [w0, w1) of an IBF, before it has memory (txq_api.hip alloc_ibf)
inline IbfDev ibf_shape(const txq_ibf_desc& d, uint64_t w0, uint64_t w1) {
    IbfDev f{};
    f.bin_size = d.bin_size;
    f.hash_shift = (uint32_t)d.hash_shift;
    f.hash_funs = (uint32_t)d.hash_funs;
    f.bins = (uint32_t)d.bins;
    f.word0 = (uint32_t)w0;
    f.ident_word = kNoIdent;
    f.reserved = 0;
    f.shard_words = (uint32_t)(w1 - w0);
    f.stride = row_stride(f.shard_words);
    f.words = nullptr;
    return f;
}
inline uint64_t ibf_bytes(const IbfDev& f) { return f.bin_size * (uint64_t)f.stride * 8; }

// ---- the tree ---------------------------------------------------------------------------------------------------------
struct HibfTree {
    uint64_t n = 0;
    std::vector<uint64_t> off;        // [n + 1] IBF i's technical bins in the flattened maps
    std::vector<uint64_t> next, tbu;  // flattened next_ibf_id (0 where the bin is not merged) and tb_to_user_bin
    std::vector<int> level;           // [n] 0: the root
    std::vector<uint64_t> parent, parent_tb;  // [n] the IBF and its merged bin that lead here (root: UINT64_MAX)
    std::vector<uint64_t> order;      // breadth first: parents before children
    uint32_t depth = 1;               // levels
    uint64_t max_level_width = 1;     // most IBFs on one level
    uint32_t hash_max = 1;            // most hash functions of any IBF
    uint64_t total_tbs() const { return off[n]; }
    bool merged(uint64_t i, uint64_t b) const { return tbu[off[i] + b] == TXQ_MERGED_BIN; }
    bool user(uint64_t i, uint64_t b) const { return !merged(i, b) && tbu[off[i] + b] != kClearedBin; }  // (a cleared root bin is no user bin)
    uint64_t child(uint64_t i, uint64_t b) const { return next[off[i] + b]; }
};

// Validates the tree before anything reaches the GPU and reads everything later steps ask about its shape.
// cleared_ok: the root may hold kClearedBin (a sub-tree shard).  check_user_bins = false: user-bin numbers are taken as they
// are (plan_subtree_shard: a shard's upload checks the IBFs that shard keeps).
inline PlanError read_tree(const txq_index_desc& desc, bool cleared_ok, HibfTree* out, bool check_user_bins = true) {
    HibfTree& t = *out;
    const uint64_t n = desc.n_ibf;
    typedef unsigned long long ull;
    if (n >> 31) return plan_error(PlanError::kOther, 0, "too many IBFs");
    t = HibfTree{};
    t.n = n;
    t.off.assign(n + 1, 0);
    for (uint64_t i = 0; i < n; ++i) {
        if (!desc.next_ibf_id[i] || !desc.tb_to_user_bin[i]) return plan_error(PlanError::kOther, i, "HIBF map %llu is null", (ull)i);
        t.off[i + 1] = t.off[i] + desc.ibf[i].bins;
    }
    t.next.assign(t.off[n], 0);
    t.tbu.assign(t.off[n], 0);
    t.level.assign(n, -1);
    t.parent.assign(n, UINT64_MAX);
    t.parent_tb.assign(n, 0);
    t.order.reserve(n);
    std::deque<uint64_t> q{0};
    t.level[0] = 0;
    std::vector<uint64_t> width(1, 1);
    while (!q.empty()) {
        const uint64_t i = q.front();
        q.pop_front();
        t.order.push_back(i);
        for (uint64_t b = 0; b < desc.ibf[i].bins; ++b) {
            const uint64_t ub = desc.tb_to_user_bin[i][b];
            uint64_t nx = desc.next_ibf_id[i][b];
            if (ub == TXQ_MERGED_BIN) {
                if (nx >= n || nx == i) return plan_error(PlanError::kBadChild, nx, "IBF %llu bin %llu: bad child %llu", (ull)i, (ull)b, (ull)nx);
                if (t.level[nx] >= 0) return plan_error(PlanError::kTwoParents, nx, "IBF %llu has two parents: not a tree", (ull)nx);
                t.level[nx] = t.level[i] + 1;
                t.parent[nx] = i;
                t.parent_tb[nx] = b;
                if ((size_t)t.level[nx] >= width.size()) width.push_back(0);
                ++width[t.level[nx]];
                q.push_back(nx);
            } else {  // (a sub-tree shard's cleared root bins carry kClearedBin)
                if (check_user_bins && ub >= desc.user_bins && !(ub == kClearedBin && cleared_ok && i == 0))
                    return plan_error(PlanError::kOther, i, "IBF %llu bin %llu: user bin %llu out of range", (ull)i, (ull)b, (ull)ub);
                nx = 0;
            }
            t.next[t.off[i] + b] = nx;
            t.tbu[t.off[i] + b] = ub;
        }
    }
    for (uint64_t i = 0; i < n; ++i)
        if (t.level[i] < 0) return plan_error(PlanError::kOther, i, "IBF %llu is unreachable from the root", (ull)i);
    t.depth = (uint32_t)width.size();
    for (uint64_t w : width) t.max_level_width = std::max(t.max_level_width, w);
    for (uint64_t i = 0; i < n; ++i) t.hash_max = std::max(t.hash_max, (uint32_t)desc.ibf[i].hash_funs);
    return PlanError{};
}

// ---- maps of the descent kernels ----------------------------------------------------------------------------------------
struct MapsPlan {
    std::vector<uint64_t> moff;     // [n + 1] IBF i's words in merged / descend (4 per IBF at least: the fused kernel reads two 16-byte pieces)
    std::vector<uint64_t> merged;   // bit b of IBF i's word w: technical bin 64 w + b is a merged bin
    std::vector<uint64_t> descend;  // the merged bins whose sub-tree holds a user bin of this shard's mask columns
    bool compact = false;           // the tree fits the 32-byte node records
    std::vector<HibfNode> nodes;    // compact: [technical bin] the child behind a merged bin, [total technical bins] the root
};

// Also sets ibf[i].ident_word of identity-mapped leaves (technical bin b is user bin 64 * ident_word + b).
inline MapsPlan plan_maps(const HibfTree& t, const txq_index_desc& desc, std::vector<IbfDev>& ibf, uint64_t shard_word0, uint64_t shard_words) {
    const uint64_t n = t.n;
    MapsPlan m;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t base = t.tbu[t.off[i]];
        bool ident = base != TXQ_MERGED_BIN && base % 64 == 0 && (base >> 6) + desc.ibf[i].bin_words < kNoIdent;
        for (uint64_t b = 0; ident && b < desc.ibf[i].bins; ++b) ident = t.tbu[t.off[i] + b] == base + b;
        if (ident) ibf[i].ident_word = (uint32_t)(base >> 6);
    }
    m.moff.assign(n + 1, 0);
    for (uint64_t i = 0; i < n; ++i) m.moff[i + 1] = m.moff[i] + ((desc.ibf[i].bin_words + 3) & ~(uint64_t)3);
    m.merged.assign(m.moff[n], 0);
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t b = 0; b < desc.ibf[i].bins; ++b)
            if (t.merged(i, b)) m.merged[m.moff[i] + (b >> 6)] |= 1ULL << (b & 63);
    // Sub-tree pruning for column shards: a merged bin is only descended into when its sub-tree
    // holds a user bin whose mask word belongs to this shard (span[i] = mask-word range under IBF i).
    std::vector<std::pair<uint64_t, uint64_t>> span(n, {UINT64_MAX, 0});
    for (size_t at = t.order.size(); at-- > 0;) {  // children before parents
        const uint64_t i = t.order[at];
        for (uint64_t b = 0; b < desc.ibf[i].bins; ++b) {
            const uint64_t ub = t.tbu[t.off[i] + b];
            if (ub == kClearedBin) continue;
            std::pair<uint64_t, uint64_t> r = ub == TXQ_MERGED_BIN ? span[t.child(i, b)] : std::make_pair(ub >> 6, ub >> 6);
            if (r.first < span[i].first) span[i].first = r.first;
            if (r.first != UINT64_MAX && r.second > span[i].second) span[i].second = r.second;
        }
    }
    m.descend.assign(m.moff[n], 0);
    const uint64_t shard_lo = shard_word0, shard_hi = shard_word0 + shard_words;  // [lo, hi)
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t b = 0; b < desc.ibf[i].bins; ++b) {
            if (!t.merged(i, b)) continue;
            const auto& r = span[t.child(i, b)];
            if (r.first != UINT64_MAX && r.first < shard_hi && r.second >= shard_lo) m.descend[m.moff[i] + (b >> 6)] |= 1ULL << (b & 63);
        }
    // node records by technical bin for the fused kernel (skipped for trees too large for it)
    const uint64_t total = t.total_tbs();
    m.compact = total < kRootEntry && m.moff[n] < 0xFFFFFFFFull && total <= ((size_t)256 << 20) / sizeof(HibfNode);
    for (const IbfDev& f : ibf) m.compact = m.compact && !(f.bin_size >> 32) && f.stride < (1u << 20) && f.hash_shift < 64 && f.hash_funs < 8;
    if (m.compact) {
        m.nodes.assign(total + 1, HibfNode{});
        auto node_of = [&](uint64_t i) {
            const IbfDev& f = ibf[i];
            bool has_merged = false;
            for (uint64_t w = m.moff[i]; w < m.moff[i + 1]; ++w) has_merged = has_merged || m.merged[w] != 0;
            HibfNode nd{};
            nd.words = (uint64_t)(uintptr_t)f.words;
            nd.bin_size = (uint32_t)f.bin_size;
            nd.packed = pack_ibf_params(f) | ((uint32_t)has_merged << 29);
            nd.off = (uint32_t)t.off[i];
            nd.moff = (uint32_t)m.moff[i];
            nd.ident_word = f.ident_word;
            nd.bins = f.bins;
            return nd;
        };
        for (uint64_t i = 0; i < n; ++i)
            for (uint64_t b = 0; b < desc.ibf[i].bins; ++b)
                if (t.merged(i, b)) m.nodes[t.off[i] + b] = node_of(t.child(i, b));
        m.nodes[total] = node_of(0);
    }
    return m;
}

// ---- regular two-level trees --------------------------------------------------------------------------------------------
// Is the tree a regular two-level one: a root of merged bins only over leaf IBFs that each map an aligned run of user bins, all
// of one power-of-two row width, tiling the mask?  Those shard by mask columns (txq_index_upload_subtrees) and get a ChildRec
// table (plan_regular).  by_column[c]: the IBF that owns mask words [c * wpr, (c + 1) * wpr); root_tb[i]: the root's bin of IBF i.
inline bool regular_two_level(const txq_index_desc& d, std::vector<uint64_t>* by_column = nullptr, std::vector<uint64_t>* root_tb = nullptr) {
    const uint64_t n = d.n_ibf;
    if (n < 2 || d.ibf[0].bins != n - 1) return false;
    const uint64_t wpr = d.ibf[1].bin_words;
    if (wpr < 1 || (wpr & (wpr - 1)) || wpr > 128 || (d.user_bins + 63) / 64 != wpr * (n - 1)) return false;
    std::vector<uint64_t> column(n - 1, UINT64_MAX), tb(n, UINT64_MAX);
    for (uint64_t b = 0; b < d.ibf[0].bins; ++b) {
        if (d.tb_to_user_bin[0][b] != TXQ_MERGED_BIN) return false;
        const uint64_t c = d.next_ibf_id[0][b];
        if (c == 0 || c >= n || tb[c] != UINT64_MAX) return false;
        tb[c] = b;
    }
    for (uint64_t i = 1; i < n; ++i) {
        if (d.ibf[i].bin_words != wpr) return false;
        const uint64_t base = d.tb_to_user_bin[i][0];
        if (base == TXQ_MERGED_BIN || base % (wpr * 64)) return false;
        for (uint64_t b = 0; b < d.ibf[i].bins; ++b)
            if (d.tb_to_user_bin[i][b] != base + b) return false;
        const uint64_t col = base / (wpr * 64);
        if (col >= n - 1 || column[col] != UINT64_MAX) return false;
        column[col] = i;
    }
    if (by_column) by_column->swap(column);
    if (root_tb) root_tb->swap(tb);
    return true;
}

struct RegularPlan {
    std::vector<ChildRec> children;   // this shard's children in mask-column order
    std::vector<uint64_t> by_column;  // every column's IBF
    bool children_uniform = true;     // same rows / hash shift / hash count in every child
    uint32_t child_row_words = 0;
    uint64_t children_bytes = 0;      // their matrices
    HibfNode root{};                  // the root as the kernels take it
    bool interleave = false;          // small tree of uniform children: worth a copy with row r of all children side by side ...
    IbfDev interleaved{};             // ... of this shape (words: null)
};

// The ChildRec table of a regular two-level tree whose shard's column range starts and ends on child boundaries; nothing for
// any other tree (or one the 32-byte node records do not fit: `compact`).
inline std::optional<RegularPlan> plan_regular(const HibfTree& t, const txq_index_desc& desc, const std::vector<IbfDev>& ibf, bool compact,
                                               uint64_t shard_word0, uint64_t shard_words) {
    RegularPlan r;
    std::vector<uint64_t> root_tb;
    if (!compact || desc.ibf[0].bins >= (1u << 20) || t.depth != 2 || !regular_two_level(desc, &r.by_column, &root_tb)) return std::nullopt;
    const uint32_t wpr = (uint32_t)desc.ibf[1].bin_words;
    if (shard_word0 % wpr || shard_words % wpr || !shard_words) return std::nullopt;
    for (uint64_t c = shard_word0 / wpr; c < (shard_word0 + shard_words) / wpr; ++c) {
        const IbfDev& f = ibf[r.by_column[c]];
        r.children.push_back(ChildRec{(uint64_t)(uintptr_t)f.words, (uint32_t)f.bin_size, f.hash_shift | (f.hash_funs << 8) | ((uint32_t)root_tb[r.by_column[c]] << 12)});
        r.children_bytes += ibf_bytes(f);
    }
    for (const ChildRec& c : r.children)
        r.children_uniform = r.children_uniform && c.bin_size == r.children[0].bin_size && (c.packed & 0xFFFu) == (r.children[0].packed & 0xFFFu);
    r.child_row_words = wpr;
    const IbfDev& root = ibf[0];
    r.root.words = (uint64_t)(uintptr_t)root.words;
    r.root.bin_size = (uint32_t)root.bin_size;
    r.root.packed = pack_ibf_params(root);
    r.root.bins = root.bins;
    r.interleave = r.children_uniform && root.bins <= 64 && shard_words <= 32;
    if (r.interleave) {  // [rows][stride] like a flat IBF over the children's hash parameters
        const IbfDev& c0 = ibf[r.by_column[shard_word0 / wpr]];
        IbfDev& f = r.interleaved;
        f.bin_size = c0.bin_size;
        f.hash_shift = c0.hash_shift;
        f.hash_funs = c0.hash_funs;
        f.shard_words = (uint32_t)shard_words;
        f.stride = row_stride(f.shard_words);
        f.bins = (uint32_t)shard_words * 64u;
        f.ident_word = kNoIdent;
    }
    return r;
}

// ---- layout order -------------------------------------------------------------------------------------------------------
// Layout order for a tree that is not regular (txq_records.hpp VChunk): the rows of all IBFs, levels ascending, each IBF padded
// to whole chunks; per chunk its record, per IBF its ancestors, which bits are user bins, and the user bin behind every bit.
struct SplitPlan {                      // split user bins (txq_records.hpp VSplit); empty vectors when the tree has none
    bool any = false;
    std::vector<uint64_t> nonrep;       // [words] bits of the parts that are not their bin's representative
    std::vector<uint32_t> rep_pos;      // [words * 64] for such a bit: the representative's bit position in the row
    std::vector<VSplitRange> ranges;    // [chunks]; `side` is a WORD OFFSET into the side buffer (the uploader adds its address)
    std::vector<VSplit> flat;           // the chunks' entries, every IBF's consecutive
    std::vector<uint32_t> side_pos;     // per entry: its bit in its IBF's side row (word * 64 + bit)
    std::vector<uint64_t> side_off;     // [n + 1] per IBF: first word of its side matrix in the side buffer
    std::vector<uint32_t> side_stride;  // [n] words per side row (0: the IBF has no split bins)
};
struct LayoutPlan {
    uint64_t cwords = 2;                // words per chunk: 2 (16-byte lanes), or 1 for trees of narrow IBFs
    uint64_t words = 0;                 // of a row, the padding word included
    std::vector<uint64_t> seg;          // [n] an IBF's first word in the row
    std::vector<uint64_t> padded;       // [n] an IBF's words in the row: whole chunks
    std::vector<uint32_t> chunk0;       // [n] an IBF's first chunk
    std::vector<VChunk> chunks;
    std::vector<VPath> paths;           // [n]
    std::vector<uint64_t> leaf;         // [words] bits that are user bins (split bins: the representative only)
    std::vector<uint32_t> vuser;        // [words * 64] the user bin of a bit (kNoGate: none)
    std::vector<VLevel> levels;         // group_first = {offset into `groups`, number of groups}
    std::vector<uint32_t> groups;       // per level: first chunk of each group, then the level's end
    std::vector<HibfNode> vnodes;       // MapsPlan::nodes with every IBF's first row word as ident_word (empty: not compact)
    uint32_t v_inner_words = 0;         // of a row: the words of IBFs with merged bins (what the next level reads as gates)
    SplitPlan split;
};

// Per IBF the technical bins by user bin; the lowest part represents the bin.  Marks the chunks that hold representatives
// (VChunk::packed bit 30) and takes the other parts out of `leaf`.
inline void plan_split_bins(const HibfTree& t, const txq_index_desc& desc, const std::vector<IbfDev>& ibf, LayoutPlan& p) {
    const uint64_t n = t.n, cwords = p.cwords;
    SplitPlan& s = p.split;
    std::vector<uint64_t> nonrep(p.words, 0);
    std::vector<std::vector<VSplit>> per_chunk(p.chunks.size());
    std::vector<std::pair<uint64_t, uint64_t>> bins_of;  // (user bin, technical bin) of one IBF
    for (uint64_t i = 0; i < n; ++i) {
        bins_of.clear();
        for (uint64_t b = 0; b < desc.ibf[i].bins; ++b)
            if (t.user(i, b)) bins_of.emplace_back(t.tbu[t.off[i] + b], b);
        std::sort(bins_of.begin(), bins_of.end());
        for (size_t at = 0; at < bins_of.size();) {
            size_t end = at + 1;
            while (end < bins_of.size() && bins_of[end].first == bins_of[at].first) ++end;
            if (end - at > 1) {
                if (!s.any) { s.any = true; s.rep_pos.assign(p.words * 64, kNoGate); }
                const uint64_t rep = bins_of[at].second;  // (sorted: the lowest technical bin)
                const uint32_t chunk = p.chunk0[i] + (uint32_t)((rep >> 6) / cwords);
                const uint16_t rep_bit = (uint16_t)(rep - (uint64_t)((rep >> 6) / cwords) * cwords * 64);
                for (size_t j = at + 1; j < end; ++j) {
                    const uint64_t part = bins_of[j].second;
                    nonrep[p.seg[i] + (part >> 6)] |= 1ULL << (part & 63);
                    s.rep_pos[(p.seg[i] + (part >> 6)) * 64 + (part & 63)] = (uint32_t)((p.seg[i] + (rep >> 6)) * 64 + (rep & 63));
                    per_chunk[chunk].push_back(VSplit{(uint32_t)(part >> 6), rep_bit, (uint16_t)(part & 63)});
                }
            }
            at = end;
        }
    }
    if (!s.any) return;
    s.nonrep.swap(nonrep);
    s.ranges.resize(p.chunks.size());
    s.side_off.assign(n + 1, 0);
    s.side_stride.assign(n, 0);
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t word = 0, used = 0, last_word = 0;
        bool has = false;
        const uint32_t c_end = p.chunk0[i] + (uint32_t)(p.padded[i] / cwords);
        for (uint32_t c = p.chunk0[i]; c < c_end; ++c) {
            std::stable_sort(per_chunk[c].begin(), per_chunk[c].end(), [](const VSplit& x, const VSplit& y) { return x.rep_bit < y.rep_bit; });
            const uint32_t cnt = (uint32_t)per_chunk[c].size();
            s.ranges[c] = VSplitRange{(uint32_t)s.flat.size(), cnt, {0, 0, 0, 0}, 0, 0, 0};
            if (!cnt) continue;
            has = true;
            // a chunk's parts are consecutive side bits from bit0 of one word on, into as many further words as they need (no
            // bound: one user bin split 200 ways gives its representative's chunk 199 parts); a chunk that does not fit after
            // `used` starts a fresh word, so only chunks of more than 64 parts span words, and those start at bit 0
            if (used && used + cnt > 64) { ++word; used = 0; }
            s.ranges[c].bit0 = used;
            s.ranges[c].side = word;  // (within the IBF's matrix for now)
            for (uint32_t e = 0; e < cnt; ++e) {
                s.ranges[c].reps[per_chunk[c][e].rep_bit >> 5] |= 1u << (per_chunk[c][e].rep_bit & 31);
                s.side_pos.push_back(word * 64 + used + e);
            }
            used += cnt;
            last_word = word + (used - 1) / 64;
            while (used >= 64) { used -= 64; ++word; }
            s.flat.insert(s.flat.end(), per_chunk[c].begin(), per_chunk[c].end());
        }
        s.side_stride[i] = has ? last_word + 1 : 0;
        s.side_off[i + 1] = s.side_off[i] + (uint64_t)s.side_stride[i] * ibf[i].bin_size;
        for (uint32_t c = p.chunk0[i]; c < c_end; ++c) {
            s.ranges[c].side_stride = s.side_stride[i];
            s.ranges[c].side += s.side_off[i];
        }
    }
    // a chunk that holds representatives says so in its record: the others never look at their range
    for (size_t c = 0; c < p.chunks.size(); ++c)
        if (s.ranges[c].count) p.chunks[c].packed |= 1u << 30;
    // the ONES of a layout-order session: a split bin is its representative
    for (size_t w = 0; w < p.leaf.size(); ++w) p.leaf[w] &= ~s.nonrep[w];
}

// Nothing where sessions cannot work in layout order: a column shard (it does not cut the layout-order row in one piece), more
// levels than a fused dense step follows, numbers that do not fit the records.  nodes: MapsPlan::nodes, or null.
inline std::optional<LayoutPlan> plan_layout_order(const HibfTree& t, const txq_index_desc& desc, const std::vector<IbfDev>& ibf, uint64_t mask_words,
                                                   uint64_t shard_word0, uint64_t shard_words, const std::vector<HibfNode>* nodes) {
    const uint64_t n = t.n;
    if (shard_words != mask_words || shard_word0 != 0 || t.depth > kMaxVDepth + 1 || desc.user_bins >= kNoGate) return std::nullopt;
    for (const IbfDev& f : ibf)
        if ((f.bin_size >> 32) || f.stride >= (1u << 20) || f.hash_funs > 5) return std::nullopt;
    LayoutPlan p;
    // 16-byte chunks (every IBF padded to an even number of words) unless that widens the row by more than 30 % — trees of
    // many one-word IBFs —: then 8-byte chunks
    uint64_t exact = 0, padded2 = 0;
    for (uint64_t i = 0; i < n; ++i) { exact += desc.ibf[i].bin_words; padded2 += (desc.ibf[i].bin_words + 1) & ~(uint64_t)1; }
    const uint64_t cwords = p.cwords = padded2 * 10 > exact * 13 ? 1 : 2;
    p.padded.resize(n);
    for (uint64_t i = 0; i < n; ++i) p.padded[i] = (desc.ibf[i].bin_words + cwords - 1) / cwords * cwords;
    // IBFs by level (ascending ids within a level), their segments in the row
    std::vector<std::vector<uint64_t>> by_level(t.depth);
    for (uint64_t i = 0; i < n; ++i) by_level[t.level[i]].push_back(i);
    p.seg.assign(n, 0);
    uint64_t words = 0;
    for (auto& lv : by_level)
        for (uint64_t i : lv) { p.seg[i] = words; words += p.padded[i]; }
    const bool pad_word = (words & 1) != 0;  // (slot masks of an even number of words: one word that belongs to no IBF)
    if (pad_word) ++words;
    if (words >= (1u << 26)) return std::nullopt;
    p.words = words;
    p.chunk0.assign(n, 0);
    p.paths.assign(n, VPath{});
    p.leaf.assign(words, 0);
    p.vuser.assign(words * 64, kNoGate);
    auto packed_of = [](const IbfDev& f) { return pack_ibf_params(f) | ((uint32_t)(f.stride == 1) << 29); };
    for (auto& lv : by_level) {
        VLevel L;
        L.first_chunk = (uint32_t)p.chunks.size();
        uint64_t group_bytes = 0;
        for (uint64_t i : lv) {
            const IbfDev& f = ibf[i];
            const uint64_t bytes = ibf_bytes(f);
            if (L.group_first.empty() || group_bytes + bytes > ((uint64_t)2 << 20)) { L.group_first.push_back((uint32_t)p.chunks.size()); group_bytes = 0; }
            group_bytes += bytes;
            p.chunk0[i] = (uint32_t)p.chunks.size();
            const bool root = t.parent[i] == UINT64_MAX;
            for (uint64_t c = 0; c < p.padded[i]; c += cwords) {
                VChunk r{};
                r.words = (uint64_t)(uintptr_t)f.words;
                r.bin_size = (uint32_t)f.bin_size;
                r.packed = packed_of(f);
                r.col = (uint32_t)c;
                r.gate_word = root ? kNoGate : (uint32_t)(p.seg[t.parent[i]] + (t.parent_tb[i] >> 6));
                r.gate_bit = (uint32_t)(t.parent_tb[i] & 63);
                r.ibf = (uint32_t)i;
                p.chunks.push_back(r);
            }
            for (uint64_t b = 0; b < desc.ibf[i].bins; ++b)
                if (t.user(i, b)) {
                    p.leaf[p.seg[i] + (b >> 6)] |= 1ULL << (b & 63);
                    p.vuser[(p.seg[i] + (b >> 6)) * 64 + (b & 63)] = (uint32_t)t.tbu[t.off[i] + b];
                }
            VPath& path = p.paths[i];
            std::vector<uint64_t> chain;  // i's ancestors, nearest first
            for (uint64_t a = i; t.parent[a] != UINT64_MAX; a = t.parent[a]) chain.push_back(a);
            for (size_t at = chain.size(); at-- > 0;) {  // root first
                const uint64_t child = chain[at];
                const IbfDev& fa = ibf[t.parent[child]];
                auto& slot = path.anc[path.depth++];
                slot.words = (uint64_t)(uintptr_t)fa.words;
                slot.bin_size = (uint32_t)fa.bin_size;
                slot.packed = packed_of(fa);
                slot.word = (uint32_t)(t.parent_tb[child] >> 6);
                slot.bit = (uint32_t)(t.parent_tb[child] & 63);
            }
        }
        if (pad_word && &lv == &by_level.back()) {  // the padding word: a chunk without hash functions — always zero
            VChunk r{};
            r.words = (uint64_t)(uintptr_t)ibf[0].words;
            r.bin_size = 1;
            r.packed = 1;  // stride 1, no hash function
            r.gate_word = kNoGate;
            p.chunks.push_back(r);
        }
        L.n_chunks = (uint32_t)p.chunks.size() - L.first_chunk;
        L.group_first.push_back((uint32_t)p.chunks.size());
        p.levels.push_back(L);
    }
    for (VLevel& L : p.levels) {  // the groups of all levels in one device array; group_first becomes offsets into it
        const uint32_t at = (uint32_t)p.groups.size();
        p.groups.insert(p.groups.end(), L.group_first.begin(), L.group_first.end());
        const uint32_t ng = (uint32_t)L.group_first.size() - 1;
        L.group_first.assign({at, ng});
    }
    if (nodes) {  // the fused kernel's node records with every IBF's place in the layout-order row (hibf_fused_kernel<G, LAYOUT>)
        p.vnodes = *nodes;
        for (uint64_t i = 1; i < n; ++i) p.vnodes[t.off[t.parent[i]] + t.parent_tb[i]].ident_word = (uint32_t)p.seg[i];
        p.vnodes[t.total_tbs()].ident_word = (uint32_t)p.seg[0];
    }
    for (uint64_t i = 0; i < n; ++i) {
        bool inner = false;
        for (uint64_t b = 0; b < desc.ibf[i].bins && !inner; ++b) inner = t.merged(i, b);
        if (inner) p.v_inner_words += (uint32_t)p.padded[i];
    }
    plan_split_bins(t, desc, ibf, p);
    return p;
}

// ---- sub-tree shards ----------------------------------------------------------------------------------------------------
// A general tree in `n_shards` sub-tree shards: the sub-trees under the root's merged bins are dealt out, largest (by row words)
// first, each to the shard that holds least (ties: the lower shard) — the same deal on every rank.  A shard's tree is the root
// and its own sub-trees, renumbered in the original order; in its copy of the root the columns of everybody else's technical
// bins are cleared (keep_mask) and those bins become kClearedBin: no user bin, never firing.
struct SubtreeShard {
    std::vector<uint64_t> kept;       // the shard's IBFs: ids in the whole tree, ascending
    std::vector<uint64_t> new_id;     // [n] an IBF's id in the shard's tree (UINT64_MAX: not kept)
    std::vector<uint64_t> keep_mask;  // [root row words] the root's technical bins that are this shard's
    std::vector<std::vector<uint64_t>> next, user;  // [kept] the shard's maps
};
inline SubtreeShard plan_subtree_shard(const HibfTree& t, const txq_index_desc& desc, int rank, int n_shards) {
    const uint64_t n = t.n, root_bins = desc.ibf[0].bins;
    std::vector<uint64_t> owner(n, UINT64_MAX), weight(root_bins, 0);  // which root bin's sub-tree an IBF belongs to (the root: none)
    for (uint64_t i : t.order) {
        if (i == 0) continue;
        owner[i] = t.parent[i] == 0 ? t.parent_tb[i] : owner[t.parent[i]];
        weight[owner[i]] += desc.ibf[i].bin_words;
    }
    std::vector<uint64_t> order;
    for (uint64_t b = 0; b < root_bins; ++b)
        if (t.merged(0, b)) order.push_back(b);
    std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return weight[a] > weight[b]; });
    std::vector<uint64_t> load(n_shards, 0);
    std::vector<int> shard_of_bin(root_bins, 0);  // (the root's own user bins: shard 0)
    for (uint64_t b : order) {
        int best = 0;
        for (int r = 1; r < n_shards; ++r)
            if (load[r] < load[best]) best = r;
        shard_of_bin[b] = best;
        load[best] += weight[b];
    }
    SubtreeShard s;
    s.new_id.assign(n, UINT64_MAX);
    for (uint64_t i = 0; i < n; ++i)
        if (i == 0 || shard_of_bin[owner[i]] == rank) { s.new_id[i] = s.kept.size(); s.kept.push_back(i); }
    s.keep_mask.assign(desc.ibf[0].bin_words, 0);
    for (uint64_t b = 0; b < root_bins; ++b)
        if (shard_of_bin[b] == rank) s.keep_mask[b >> 6] |= 1ULL << (b & 63);
    s.next.resize(s.kept.size());
    s.user.resize(s.kept.size());
    for (size_t j = 0; j < s.kept.size(); ++j) {
        const uint64_t i = s.kept[j];
        s.next[j].assign(desc.ibf[i].bins, 0);
        s.user[j].assign(desc.ibf[i].bins, 0);
        for (uint64_t b = 0; b < desc.ibf[i].bins; ++b) {
            if (i == 0 && shard_of_bin[b] != rank) { s.user[j][b] = kClearedBin; continue; }  // (cleared column: no user bin, never reported)
            s.user[j][b] = t.tbu[t.off[i] + b];
            if (t.merged(i, b)) s.next[j][b] = s.new_id[t.child(i, b)];
        }
    }
    return s;
}

}  // namespace txq
