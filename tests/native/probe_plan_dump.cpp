// The host's half of the flat probe's domain table (tetrex_amd/csrc/txq_probe_plan.hpp) without a GPU: commands come in on
// stdin, one per line, each answered by one line on stdout; tests/test_probe_plan.py holds the cases and what they must give.
//   cap   probe_table table_mb bin_size stride hash_funs n         -> table_capacity
//   rows  fresh built top count ratio sample cap_rows              -> "lo rows" of table_rows (what both kernels compute)
//   call  index_generation reallocated keep                        -> "fresh zero_state parity" of plan_probe_call, on ONE table
//   fail                                                           -> a call's launches failed (probe_flat leaves valid = false)
#include "../../tetrex_amd/csrc/txq_probe_plan.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstring>

using namespace txq;

int main() {
    ProbeKeep keep;
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        long long a[7] = {0, 0, 0, 0, 0, 0, 0};
        const int want = !strcmp(cmd, "cap") ? 6 : !strcmp(cmd, "rows") ? 7 : !strcmp(cmd, "call") ? 3 : !strcmp(cmd, "fail") ? 0 : -1;
        if (want < 0) { fprintf(stderr, "probe_plan_dump: unknown command %s\n", cmd); return 2; }
        for (int i = 0; i < want; ++i)
            if (scanf("%lld", &a[i]) != 1) { fprintf(stderr, "probe_plan_dump: short input\n"); return 2; }
        if (!strcmp(cmd, "cap")) {
            printf("%zu\n", table_capacity((int)a[0], a[1], (uint64_t)a[2], (uint32_t)a[3], (uint32_t)a[4], (size_t)a[5]));
        } else if (!strcmp(cmd, "rows")) {
            const ProbeRows r = table_rows(a[0] != 0, (uint32_t)a[1], (uint32_t)a[2], (uint32_t)a[3], (uint32_t)a[4], (uint32_t)a[5], (uint32_t)a[6]);
            printf("%" PRIu32 " %" PRIu32 "\n", r.lo, r.rows);
        } else if (!strcmp(cmd, "call")) {
            const ProbeCall c = plan_probe_call(keep, (uint64_t)a[0], a[1] != 0, a[2] != 0);
            printf("%d %d %" PRIu32 "\n", (int)c.fresh, (int)c.zero_state, c.parity);
        } else {
            keep.valid = false;
            printf("failed\n");
        }
    }
    return 0;
}
