// Prints what tetrex_amd/csrc/host/search_plan.hpp computes, for tests/test_search_plan.py to compare with the Python
// restatements (tests/search_window_ref.py, tests/frame_window_ref.py).  A stand-alone program, built with the address and
// undefined-behaviour sanitizers; numbers come in through the arguments and standard input, one answer a line goes out.
//   windows k W S Lmax           for L = 0 .. Lmax: "L a:len a:len ..." — the windows of a record of L letters
//   thresholds k nmax            for E in 0 1 2: "e E n t", for F in 0.01 0.5 1.0: "f F n t", n = 0 .. nmax
//   runs                         stdin "window bin count" a line, sorted by bin and window: "bin first last best count" a run
//   cut_windows maxv maxw        stdin "begin len" a line: "cut c0 c1 ..." and "most values windows"
//   cut_records maxv maxr        stdin: the record offsets on one line, their bounds on the next: "cut ..." and "most values bytes records"
#include "../../tetrex_amd/csrc/host/search_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

using namespace tetrex;

namespace {

struct Hit { uint32_t query, bin, count; };

unsigned long long number(const char* s) { return std::strtoull(s, nullptr, 10); }

std::vector<uint64_t> numbers_of_line() {
    std::vector<uint64_t> out;
    std::string line;
    std::getline(std::cin, line);
    std::istringstream in(line);
    for (uint64_t v; in >> v;) out.push_back(v);
    return out;
}

void print_cuts(const plan::Cuts& c) {
    std::printf("cut");
    for (size_t x : c.cut) std::printf(" %zu", x);
    std::printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "windows" && argc == 6) {
        const uint32_t k = (uint32_t)number(argv[2]), W = (uint32_t)number(argv[3]), S = (uint32_t)number(argv[4]);
        for (uint64_t L = 0; L <= number(argv[5]); ++L) {
            const txq::fw::Frame layout = plan::record_windows(L, k, W, S);
            std::printf("%llu", (unsigned long long)L);
            for (uint64_t j = 0; j < layout.count; ++j) {
                const txq::fw::Window w = txq::fw::window_at(layout, j);
                std::printf(" %llu:%llu", (unsigned long long)w.a, (unsigned long long)w.len);
            }
            std::printf("\n");
        }
        return 0;
    }
    if (mode == "thresholds" && argc == 4) {
        const uint64_t k = number(argv[2]), nmax = number(argv[3]);
        for (uint64_t E = 0; E <= 2; ++E)
            for (uint64_t n = 0; n <= nmax; ++n)
                std::printf("e %llu %llu %llu\n", (unsigned long long)E, (unsigned long long)n, (unsigned long long)plan::Threshold{false, 0, k, E}.of(n));
        for (const char* F : {"0.01", "0.5", "1.0"})
            for (uint64_t n = 0; n <= nmax; ++n)
                std::printf("f %s %llu %llu\n", F, (unsigned long long)n, (unsigned long long)plan::Threshold{true, std::strtod(F, nullptr), k, 0}.of(n));
        return 0;
    }
    if (mode == "runs" && argc == 2) {
        std::vector<Hit> hits;
        for (Hit h; std::cin >> h.query >> h.bin >> h.count;) hits.push_back(h);
        plan::for_each_run(hits, [](const Hit& first, const Hit& last, const Hit& best) {
            std::printf("%u %u %u %u %u\n", first.bin, first.query, last.query, best.query, best.count);
        });
        return 0;
    }
    if (mode == "cut_windows" && argc == 4) {
        std::vector<uint64_t> begins;
        std::vector<uint32_t> lens;
        for (uint64_t b, l; std::cin >> b >> l;) begins.push_back(b), lens.push_back((uint32_t)l);
        const plan::Cuts c = plan::cut_windows(begins, lens, number(argv[2]), number(argv[3]));
        print_cuts(c);
        std::printf("most %llu %zu\n", (unsigned long long)c.most_values, c.most_items);
        return 0;
    }
    if (mode == "cut_records" && argc == 4) {
        const std::vector<uint64_t> offsets = numbers_of_line(), bounds = numbers_of_line();
        if (offsets.size() != bounds.size() + 1) return 2;
        const plan::Cuts c = plan::cut_records(offsets, [&](size_t r) { return bounds[r]; }, number(argv[2]), number(argv[3]));
        print_cuts(c);
        std::printf("most %llu %llu %zu\n", (unsigned long long)c.most_values, (unsigned long long)c.most_bytes, c.most_items);
        return 0;
    }
    std::fprintf(stderr, "usage: search_plan_dump windows|thresholds|runs|cut_windows|cut_records ...\n");
    return 2;
}
