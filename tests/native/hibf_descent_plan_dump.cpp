// The path choice and launch arithmetic of the HIBF descent (tetrex_amd/csrc/txq_hibf_descent_plan.hpp) without a GPU: commands
// come in on stdin, one per line, each answered by one line of numbers on stdout; tests/test_hibf_descent_plan.py holds the cases,
// tests/hibf_descent_ref.py the same arithmetic in Python (its DESCENT_FIELDS / LAYOUT_FIELDS name the numbers of a line).
//   descent  shard_words n_ibf total_tbs max_stride max_level_width depth has_nodes n_children child_row_words children_bytes
//            children_uniform root_stride probes_interleaved  levels stationary small lane_hash steps_per_group tile unroll waves
//            stack_lds  n
//     -> path | fused: ok stack_lds wave_bytes waves_per_block grid G w_iters | stationary: ok lanes_per_child n_steps
//        steps_per_group n_groups groups_per_phase phases tile n_tiles grid root_blocks unroll uniform | small: applies blocks |
//        levels: G w_iters chunk cap blocks_level0 blocks_last_chunk_level0 blocks_deeper alive_blocks
//   layout   v_words n_ibf max_stride has_vnodes has_split v_inner_words n_groups  layout_fused layout_direct waves stack_lds  n
//     -> fused: ok stack_lds row_lds_words wave_bytes waves_per_block grid G w_iters | level kernel: n_tiles phases grid piece
#include "../../tetrex_amd/csrc/txq_hibf_descent_plan.hpp"

#include <cstdio>
#include <cstring>

using namespace txq;

int main() {
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        long long a[23];
        const int want = !strcmp(cmd, "descent") ? 23 : !strcmp(cmd, "layout") ? 12 : -1;
        if (want < 0) { fprintf(stderr, "hibf_descent_plan_dump: unknown command %s\n", cmd); return 2; }
        for (int i = 0; i < want; ++i)
            if (scanf("%lld", &a[i]) != 1) { fprintf(stderr, "hibf_descent_plan_dump: short input\n"); return 2; }
        if (!strcmp(cmd, "descent")) {
            DescentShape sh;
            sh.shard_words = (uint32_t)a[0];
            sh.n_ibf = (uint64_t)a[1];
            sh.total_tbs = (uint64_t)a[2];
            sh.max_stride = (uint32_t)a[3];
            sh.max_level_width = (uint64_t)a[4];
            sh.depth = (uint32_t)a[5];
            sh.has_nodes = a[6] != 0;
            sh.n_children = (uint32_t)a[7];
            sh.child_row_words = (uint32_t)a[8];
            sh.children_bytes = (uint64_t)a[9];
            sh.children_uniform = a[10] != 0;
            sh.root_stride = (uint32_t)a[11];
            sh.probes_interleaved = a[12] != 0;
            DescentKnobs kn;
            kn.levels = a[13] != 0;
            kn.stationary = a[14] != 0;
            kn.small = a[15] != 0;
            kn.lane_hash = a[16] != 0;
            kn.steps_per_group = (int)a[17];
            kn.tile = (int)a[18];
            kn.unroll = (int)a[19];
            kn.waves = a[20];
            kn.stack_lds = a[21];
            const size_t n = (size_t)a[22];
            const FusedPlan f = plan_fused(sh, kn, n);
            const StationaryPlan c = plan_stationary(sh, kn, n);
            const LevelsPlan l = plan_levels(sh, n);
            const size_t last = n % l.chunk ? n % l.chunk : l.chunk;
            printf("%d  %d %u %zu %u %u %d %u  %d %u %u %u %u %u %u %u %zu %u %u %d %d  %d %u  %d %u %zu %zu %u %u %u %u\n", (int)descent_path(sh, kn, n),
                   (int)f.ok, f.stack_lds, f.wave_bytes, f.waves_per_block, f.grid, f.G, f.w_iters,
                   (int)c.ok, c.lanes_per_child, c.n_steps, c.steps_per_group, c.n_groups, c.groups_per_phase, c.phases, c.tile, c.n_tiles, c.grid, c.root_blocks, c.unroll, (int)c.uniform,
                   (int)small_applies(sh, kn), small_blocks(n),
                   l.G, l.w_iters, l.chunk, l.cap, level_blocks(l.G, 0, l.chunk), level_blocks(l.G, 0, last), l.blocks_deeper, l.alive_blocks);
        } else {
            DescentKnobs kn;
            kn.layout_fused = a[7] != 0;
            kn.layout_direct = a[8] != 0;
            kn.waves = a[9];
            kn.stack_lds = a[10];
            const size_t n = (size_t)a[11];
            const FusedPlan f = plan_fused_layout((uint32_t)a[0], (uint64_t)a[1], (uint32_t)a[2], a[3] != 0, a[4] != 0, kn, n);
            const uint32_t n_tiles = layout_level_tiles(n);
            printf("%d %u %u %zu %u %u %d %u  %u %u %u %zu\n", (int)f.ok, f.stack_lds, f.row_lds_words, f.wave_bytes, f.waves_per_block, f.grid, f.G, f.w_iters,
                   n_tiles, layout_level_phases((uint32_t)a[6]), layout_level_grid((uint32_t)a[6], n_tiles), layout_level_piece((uint32_t)a[5]));
        }
    }
    return 0;
}
