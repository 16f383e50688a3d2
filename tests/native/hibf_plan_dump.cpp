// Everything an HIBF upload plans on the host (tetrex_amd/csrc/txq_hibf_plan.hpp), printed by name: one case of
// tests/golden/hibf_plan_trees.json comes in on stdin as a stream of numbers, every planned array and scalar goes out as
// "name value" (arrays: byte count and hex), tests/test_hibf_plan.py compares them with tests/golden/hibf_plan_expected.json.
// No GPU: IBF i "lives" at address (i + 1) << 32, which is what the records that hold device addresses then contain.
//   input: mode (0 txq_index_upload, 1 txq_index_upload_subtrees)  rank  n_shards  user_bins  n_ibf
//          per IBF: bins  bin_size  hash_funs  has_maps (0: null maps)  [bins x next_ibf_id]  [bins x tb_to_user_bin]
#include "../../tetrex_amd/csrc/txq_hibf_plan.hpp"

#include <cinttypes>
#include <cstdio>

using namespace txq;

static void scalar(const char* name, uint64_t v) { printf("%s %" PRIu64 "\n", name, v); }
static void bytes(const char* name, const void* p, size_t n) {
    printf("%s %zu ", name, n);
    for (size_t i = 0; i < n; ++i) printf("%02x", ((const unsigned char*)p)[i]);
    printf("\n");
}
template <class T>
static void array(const char* name, const std::vector<T>& v, size_t count = SIZE_MAX) {
    bytes(name, v.data(), std::min(count, v.size()) * sizeof(T));
}
static uint64_t number() {
    unsigned long long v = 0;
    if (scanf("%llu", &v) != 1) { fprintf(stderr, "hibf_plan_dump: short input\n"); exit(2); }
    return v;
}
static int refused(const PlanError& e) {
    printf("rc %d\n", e.code);
    printf("error %s\n", e.text.c_str());
    return 0;
}

// what hibf_upload does with a tree, the device left out; device_bytes as its device_array / device_alloc calls count it
static int upload(const txq_index_desc& desc, uint64_t shard_word0, uint64_t shard_words, bool cleared_ok) {
    const uint64_t mask_words = (desc.user_bins + 63) / 64;
    HibfTree tree;
    if (PlanError e = read_tree(desc, cleared_ok, &tree)) return refused(e);
    const uint64_t n = tree.n;
    std::vector<IbfDev> ibf;
    uint64_t device_bytes = 0, max_stride = 1;
    for (uint64_t i = 0; i < n; ++i) {
        IbfDev f = ibf_shape(desc.ibf[i], 0, desc.ibf[i].bin_words);
        f.words = (uint64_t*)(uintptr_t)((i + 1) << 32);
        device_bytes += ibf_bytes(f);
        max_stride = std::max<uint64_t>(max_stride, f.stride);
        ibf.push_back(f);
    }
    const MapsPlan maps = plan_maps(tree, desc, ibf, shard_word0, shard_words);
    device_bytes += n * sizeof(IbfDev) + tree.total_tbs() * 16 + n * 8 + maps.nodes.size() * sizeof(HibfNode);  // (merged, descend, merged_off: not counted)
    const auto regular = plan_regular(tree, desc, ibf, maps.compact, shard_word0, shard_words);
    std::optional<LayoutPlan> layout;
    if (!regular) layout = plan_layout_order(tree, desc, ibf, mask_words, shard_word0, shard_words, maps.compact ? &maps.nodes : nullptr);
    if (regular) device_bytes += regular->children.size() * sizeof(ChildRec) + (regular->interleave ? ibf_bytes(regular->interleaved) : 0);
    if (layout) {  // (groups: not counted)
        const LayoutPlan& p = *layout;
        device_bytes += p.vnodes.size() * sizeof(HibfNode) + p.chunks.size() * sizeof(VChunk) + p.paths.size() * sizeof(VPath) + p.leaf.size() * 8 + p.vuser.size() * 4;
        if (p.split.any)
            device_bytes += p.split.side_off[n] * 8 + p.split.nonrep.size() * 8 + p.split.rep_pos.size() * 4 + p.split.ranges.size() * sizeof(VSplitRange) +
                            p.split.flat.size() * sizeof(VSplit);
    }
    scalar("rc", 0);
    scalar("n_ibf", n);
    scalar("shard_word0", shard_word0);
    scalar("shard_words", shard_words);
    scalar("depth", tree.depth);
    scalar("total_tbs", tree.total_tbs());
    scalar("max_level_width", tree.max_level_width);
    scalar("max_stride", max_stride);
    scalar("device_bytes", device_bytes);
    array("ibf", ibf);
    array("next", tree.next);
    array("tb_user", tree.tbu);
    array("map_off", tree.off, n);
    array("merged", maps.merged);
    array("descend", maps.descend);
    array("merged_off", maps.moff, n);
    scalar("compact", maps.compact);
    array("nodes", maps.nodes);
    scalar("regular", regular.has_value());
    if (regular) {
        const RegularPlan& r = *regular;
        scalar("tree_hash_max", tree.hash_max);
        array("by_column", r.by_column);
        array("children", r.children);
        scalar("children_uniform", r.children_uniform);
        scalar("child_row_words", r.child_row_words);
        scalar("children_bytes", r.children_bytes);
        bytes("root_node", &r.root, sizeof r.root);
        scalar("interleave", r.interleave);
        if (r.interleave) bytes("interleaved", &r.interleaved, sizeof r.interleaved);
    }
    scalar("layout_order", layout.has_value());
    if (layout) {
        const LayoutPlan& p = *layout;
        scalar("tree_hash_max", tree.hash_max);
        scalar("v_chunk_words", p.cwords);
        scalar("v_words", p.words);
        scalar("v_inner_words", p.v_inner_words);
        scalar("n_vchunks", p.chunks.size());
        scalar("v_depth", tree.depth - 1);
        array("seg", p.seg);
        array("chunk0", p.chunk0);
        array("vchunks", p.chunks);
        array("vpaths", p.paths);
        array("vleaf", p.leaf);
        array("vuser", p.vuser);
        array("vgroups", p.groups);
        std::vector<uint32_t> levels;
        for (const VLevel& L : p.levels) levels.insert(levels.end(), {L.first_chunk, L.n_chunks, L.group_first[0], L.group_first[1]});
        array("vlevels", levels);
        array("vnodes", p.vnodes);
        scalar("split_bins", p.split.any);
        if (p.split.any) {
            array("vnonrep", p.split.nonrep);
            array("vrep", p.split.rep_pos);
            array("vsplit_range", p.split.ranges);
            array("vsplits", p.split.flat);
            array("side_pos", p.split.side_pos);
            array("side_off", p.split.side_off);
            array("side_stride", p.split.side_stride);
        }
    }
    return 0;
}

int main() {
    const int mode = (int)number(), rank = (int)number(), n_shards = (int)number();
    const uint64_t user_bins = number(), n = number();
    std::vector<txq_ibf_desc> ibfs(n);
    std::vector<std::vector<uint64_t>> next(n), user(n);
    std::vector<const uint64_t*> next_p(n, nullptr), user_p(n, nullptr);
    for (uint64_t i = 0; i < n; ++i) {
        txq_ibf_desc& d = ibfs[i];
        d.bins = number();
        d.bin_size = number();
        d.hash_funs = number();
        d.bin_words = (d.bins + 63) / 64;
        d.tech_bins = d.bin_words * 64;
        d.hash_shift = (uint64_t)__builtin_clzll(d.bin_size);
        d.words = nullptr;
        if (!number()) continue;
        for (uint64_t b = 0; b < d.bins; ++b) next[i].push_back(number());
        for (uint64_t b = 0; b < d.bins; ++b) user[i].push_back(number());
        next_p[i] = next[i].data();
        user_p[i] = user[i].data();
    }
    const txq_index_desc desc{n, ibfs.data(), next_p.data(), user_p.data(), user_bins};
    uint64_t lo, hi;
    shard_range((user_bins + 63) / 64, rank, n_shards, &lo, &hi);
    if (mode == 0 || n_shards == 1) return upload(desc, lo, hi - lo, false);
    // txq_index_upload_subtrees: regular two-level trees shard by mask columns, any other tree by sub-trees
    for (uint64_t i = 0; i < n; ++i)
        if (!next_p[i] || !user_p[i]) return refused(plan_error(PlanError::kOther, i, "HIBF map %llu is null", (unsigned long long)i));
    if (regular_two_level(desc)) return upload(desc, lo, hi - lo, false);
    HibfTree tree;
    if (PlanError e = read_tree(desc, false, &tree, false)) {
        if (e.kind == PlanError::kBadChild || e.kind == PlanError::kTwoParents)
            e = plan_error(e.kind, e.ibf, "HIBF: bad child %llu (out of range or reached twice)", (unsigned long long)e.ibf);
        return refused(e);
    }
    const SubtreeShard shard = plan_subtree_shard(tree, desc, rank, n_shards);
    array("shard.kept", shard.kept);
    array("shard.new_id", shard.new_id);
    array("shard.keep_mask", shard.keep_mask);
    std::vector<txq_ibf_desc> kept_ibfs;
    std::vector<const uint64_t*> kept_next, kept_user;
    for (size_t j = 0; j < shard.kept.size(); ++j) {
        kept_ibfs.push_back(ibfs[shard.kept[j]]);
        kept_next.push_back(shard.next[j].data());
        kept_user.push_back(shard.user[j].data());
    }
    const txq_index_desc pruned{shard.kept.size(), kept_ibfs.data(), kept_next.data(), kept_user.data(), user_bins};
    return upload(pruned, 0, (user_bins + 63) / 64, true);
}
