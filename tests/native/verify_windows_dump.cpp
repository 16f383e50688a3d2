// Prints what plan::confirmed_runs of csrc/host/search_plan.hpp makes of the confirmed windows of one record
// (`tetrex search --window --verify-windows`), for tests/test_verify_windows_cpu.py, which holds it to the Python
// restatement tests/verify_windows_ref.py.  Built with sanitizers by that test:
//   g++ -std=c++20 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/verify_windows_dump.cpp -o dump
// stdin: one confirmed window a line, "window bin count distance strand" (strand + or -), in any order.
// stdout: one run a line, "bin strand first last best nearest" (windows), in the order of the rows.
#include "../../tetrex_amd/csrc/host/search_plan.hpp"

#include <cstdio>

int main() {
    struct Item {
        uint32_t query, bin, count, distance;
        char strand;
    };
    std::vector<Item> items;
    Item x;
    while (std::scanf("%u %u %u %u %c", &x.query, &x.bin, &x.count, &x.distance, &x.strand) == 5) items.push_back(x);
    // the order the command gives them: by bin, then strand (+ first), then window
    std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) {
        return a.bin != b.bin ? a.bin < b.bin : a.strand != b.strand ? a.strand == '+' : a.query < b.query;
    });
    for (const tetrex::plan::WindowRun& r : tetrex::plan::confirmed_runs(items))
        std::printf("%u %c %u %u %u %u\n", items[r.first].bin, items[r.first].strand, items[r.first].query, items[r.last].query, items[r.best].query,
                    items[r.nearest].query);
    return 0;
}
