// Prints what plan::target_runs of csrc/host/search_plan.hpp makes of the target hits of one record (`tetrex search
// --verify-windows --window-targets`), for tests/test_window_targets_cpu.py, which holds it to the Python
// restatement tests/window_targets_ref.py.  Built with sanitizers by that test:
//   g++ -std=c++20 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/window_targets_dump.cpp -o dump
// stdin: one target hit a line, "window bin target count distance strand" (strand + or -), in any order.
// stdout: one run a line, "bin target strand first last best nearest" (windows), in the order of the rows.
#include "../../tetrex_amd/csrc/host/search_plan.hpp"

#include <cstdio>

int main() {
    struct Item {
        uint32_t query, bin, target, count, distance;
        char strand;
    };
    std::vector<Item> items;
    Item x;
    while (std::scanf("%u %u %u %u %u %c", &x.query, &x.bin, &x.target, &x.count, &x.distance, &x.strand) == 6) items.push_back(x);
    // the order the command gives them: by bin, then target, then strand (+ first), then window
    std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) {
        if (a.bin != b.bin) return a.bin < b.bin;
        if (a.target != b.target) return a.target < b.target;
        return a.strand != b.strand ? a.strand == '+' : a.query < b.query;
    });
    for (const tetrex::plan::WindowRun& r : tetrex::plan::target_runs(items))
        std::printf("%u %u %c %u %u %u %u\n", items[r.first].bin, items[r.first].target, items[r.first].strand, items[r.first].query, items[r.last].query,
                    items[r.best].query, items[r.nearest].query);
    return 0;
}
