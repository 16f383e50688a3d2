// The plan of the flat probe's sorted answer (tetrex_amd/csrc/txq_probe_plan.hpp plan_probe_sort, sort_tile) without a GPU:
// commands come in on stdin, one per line, each answered by one line on stdout; tests/test_probe_sort_plan.py holds the cases.
//   plan   kept_fused has_alive has_root lpk stride shard_words n cap_rows sort sort_min bucket_kb scratch_mb
//            -> "on shift buckets chunks n_tiles tiles_per_xcd blocks"
//   remap  n  (plain plan of a 1024-bin index)
//            -> "n_tiles covered duplicates out_of_range other_xcd": how often the tiles [0, n_tiles) are taken by the plan's workgroups,
//               and how many taken tiles lie outside the eighth of the workgroup's XCD (b % 8)
#include "../../tetrex_amd/csrc/txq_probe_plan.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace txq;

int main() {
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        long long a[12] = {0};
        const int want = !strcmp(cmd, "plan") ? 12 : !strcmp(cmd, "remap") ? 1 : -1;
        if (want < 0) { fprintf(stderr, "probe_sort_plan_dump: unknown command %s\n", cmd); return 2; }
        for (int i = 0; i < want; ++i)
            if (scanf("%lld", &a[i]) != 1) { fprintf(stderr, "probe_sort_plan_dump: short input\n"); return 2; }
        if (!strcmp(cmd, "plan")) {
            const ProbeSort p = plan_probe_sort(a[0] != 0, a[1] != 0, a[2] != 0, (uint32_t)a[3], (uint32_t)a[4], (uint32_t)a[5], (uint64_t)a[6], (size_t)a[7],
                                                a[8] != 0, a[9], a[10], a[11]);
            printf("%d %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", (int)p.on, p.shift, p.buckets, p.chunks, p.n_tiles,
                   p.tiles_per_xcd, p.blocks);
        } else {
            const ProbeSort p = plan_probe_sort(true, false, false, 8, 16, 16, (uint64_t)a[0], 1 << 20, true, 1, 1024, 512);
            if (!p.on) { fprintf(stderr, "probe_sort_plan_dump: no plan\n"); return 2; }
            std::vector<uint8_t> taken(p.n_tiles, 0);
            uint64_t covered = 0, duplicates = 0, out_of_range = 0, other_xcd = 0;
            for (uint64_t b = 0; b < p.blocks; ++b)
                for (uint32_t w = 0; w < 4; ++w) {
                    const uint64_t t = sort_tile(p, b, w);
                    if (t / p.tiles_per_xcd != b % kSortXcds) ++other_xcd;
                    if (t >= p.n_tiles) { ++out_of_range; continue; }
                    if (taken[t]++) ++duplicates;
                    else ++covered;
                }
            printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", p.n_tiles, covered, duplicates, out_of_range, other_xcd);
        }
    }
    return 0;
}
