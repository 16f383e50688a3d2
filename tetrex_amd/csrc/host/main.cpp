// `tetrex` command line — product code.  Keeps the reference's surface for the query path:
//   tetrex query [-d] [-v] [-f] [-c] [-a] [-t N] [-o dest] [-g dibf] [--gpu-verify] <index.ibf> <regex|->
//     (include/arg_parse.h:57-71, src/main.cpp:36-59, src/query.cpp:477-498; --gpu-verify is not in the reference: the records of
//      the candidate bins that hold a match at all are found on the device, the matcher runs on those only — same rows)
//   tetrex index [-k K] [-p fpr] [-c hashes] [-t N] [-n] [-i] [-r murphy|li] [--layout uniform|sized [--tmax N] [--rearrange [--rearrange-ratio R]]] <name> <libs...>
//     (include/arg_parse.h:10-38, src/index_base.cpp:73-117)
//   tetrex search [-e E [--verify [--align] [--all-targets]] | --threshold F] [--counts] [--translate [--verify-frames [--align] [--all-targets]]] [-o dest] [-v] [-D device] <index.ibf> <queries.fa[.gz]>
//     (not in the reference: every FASTA record a query, answered by seqan::hibf membership_for(values, threshold);
//      --translate: nucleotide records on a peptide index, every record's six frames a query of their own;
//      --verify: only the bins that hold the record within E edits, confirmed on the bins' own letters;
//      --verify-frames, with --translate -e E: only the bins that hold the frame's residues within E edits, confirmed likewise;
//      --align, with either: where each confirmed match begins in its target, and its alignment as a CIGAR string;
//      --all-targets, with either: one row per record of the bin within E edits, not only the bin's best one)
//   tetrex search --window W [--step S] (-e E | --threshold F) [--counts] [-o dest] [-v] [-D device] <index.ibf> <queries.fa[.gz]>
//     (a local search: every record cut into overlapping windows of W letters, S apart, each answered like a record of its own,
//      slid on the device; the rows say where on the record each bin is hit)
//   tetrex search --translate --frame-window W [--frame-step S] (-e E | --threshold F) [--counts] [-o dest] [-v] [-D device] <index.ibf> <queries.fa[.gz]>
//     (the local search in the six frames of nucleotide records: every frame cut into overlapping windows of W residues, S apart,
//      translated, cut and slid on the device; the rows say in which frame and where on the record, in nucleotides, each bin is hit)
//   tetrex inspect <index.ibf>   (src/inspect_idx.cpp)
// The candidate-bin masks come from the GPU (libtxq.so); there is no CPU probe path.
#include "device_index.hpp"
#include "../txq_frame_windows_plan.hpp"
#include "fasta.hpp"
#include "index_file.hpp"
#include "kgraph.hpp"
#include "regex_front.hpp"
#include "verify.hpp"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <future>
#include <iomanip>
#include <iostream>
#include <sstream>

using namespace tetrex;

namespace {

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Args {
    std::vector<std::string> pos;
    std::vector<std::pair<std::string, std::string>> opts;  // canonical long name -> value ("" for flags)
    bool has(const std::string& n) const {
        for (auto& o : opts) if (o.first == n) return true;
        return false;
    }
    std::string get(const std::string& n, const std::string& dflt) const {
        for (auto& o : opts) if (o.first == n) return o.second;
        return dflt;
    }
};

struct OptSpec { char s; const char* l; bool value; };

Args parse(int argc, char** argv, int from, const std::vector<OptSpec>& spec) {
    Args a;
    bool only_pos = false;
    for (int i = from; i < argc; ++i) {
        std::string t = argv[i];
        if (only_pos || t.size() < 2 || t[0] != '-' || t == "-") { a.pos.push_back(t); continue; }
        if (t == "--") { only_pos = true; continue; }
        const OptSpec* hit = nullptr;
        std::string inline_value;
        bool has_inline = false;
        if (t[1] == '-') {
            std::string name = t.substr(2);
            const size_t eq = name.find('=');
            if (eq != std::string::npos) { inline_value = name.substr(eq + 1); name = name.substr(0, eq); has_inline = true; }
            for (auto& s : spec) if (name == s.l) hit = &s;
        } else {
            for (auto& s : spec) if (t[1] == s.s) hit = &s;
            if (hit && t.size() > 2) {
                if (hit->value) { inline_value = t.substr(2); has_inline = true; }
                else {  // bundled flags: -vf
                    for (size_t j = 1; j < t.size(); ++j) {
                        const OptSpec* f = nullptr;
                        for (auto& s : spec) if (t[j] == s.s && !s.value) f = &s;
                        if (!f) throw std::runtime_error("Unknown option " + t);
                        a.opts.emplace_back(f->l, "");
                    }
                    continue;
                }
            }
        }
        if (!hit) throw std::runtime_error("Unknown option " + t);
        if (!hit->value) { a.opts.emplace_back(hit->l, ""); continue; }
        if (!has_inline) {
            if (i + 1 >= argc) throw std::runtime_error(std::string("Missing value for option --") + hit->l);
            inline_value = argv[++i];
        }
        a.opts.emplace_back(hit->l, inline_value);
    }
    return a;
}

std::vector<std::string> split(const std::string& s, char d) {
    std::vector<std::string> out;
    std::stringstream ss(s);
    for (std::string t; std::getline(ss, t, d);) out.push_back(t);
    return out;
}

size_t popcount_mask(const uint64_t* m, uint64_t words) {
    size_t n = 0;
    for (uint64_t w = 0; w < words; ++w) n += (size_t)__builtin_popcountll(m[w]);
    return n;
}

int cmd_query(int argc, char** argv) {
    const std::vector<OptSpec> spec = {{'d', "draw", false}, {'v', "verbose", false}, {'f', "file", false}, {'c', "conj", false},
                                       {'a', "augment", false}, {'t', "threads", true}, {'o', "output", true}, {'g', "gibf", true},
                                       {'D', "device", true}, {'S', "stats", false}, {'G', "gpus", true}, {'R', "shards", true}, {'M', "max-ops", true},
                                       {'\0', "gpu-verify", false}};
    Args a;
    try {
        a = parse(argc, argv, 2, spec);
        if (a.pos.size() != 2) throw std::runtime_error("expected <index> <regex>");
        if (a.has("gpu-verify") && a.has("conj")) throw std::runtime_error("--gpu-verify does not work with -c");
    } catch (const std::exception& e) {
        std::cerr << "[Error TetRex Query module " << e.what() << "\n";
        return 0;  // the reference returns normally after a parser error (src/main.cpp:42-46)
    }
    const int threads = std::max(1, std::atoi(a.get("threads", "1").c_str()));
    bool verbose = a.has("verbose");
    const bool from_file = a.has("file"), conj = a.has("conj");
    std::string dest = a.get("output", "-");
    std::string input = a.pos[1];
    if (input == "-") std::cin >> input;

    const bool trace = std::getenv("TETREX_TRACE") != nullptr;
    const double t_start = now();
    // -D d[,d..] / --gpus N (not in the reference): the index's bins are cut into column shards, one per device (--shards R:
    // that many shards, dealt round-robin over the devices); one frontier expansion drives all shards, masks are joined on the host
    DeviceIndex dev;
    std::vector<int> devices;
    for (const std::string& d : split(a.get("device", "0"), ',')) devices.push_back(std::atoi(d.c_str()));
    if (a.has("gpus")) {
        devices.clear();
        for (int d = 0; d < std::max(1, std::atoi(a.get("gpus", "1").c_str())); ++d) devices.push_back(d);
    }
    const int n_shards = a.has("shards") ? std::max(1, std::atoi(a.get("shards", "1").c_str())) : (int)devices.size();
    // HIP start-up (~0.5 s) runs beside the mapping and parsing of the index file
    std::future<void> hip_ready = std::async(std::launch::async, [&devices]() { DeviceIndex::warm_up(devices); });
    IndexImage image;
    try {
        image = read_index_file(a.pos[0]);
    } catch (const std::exception& e) {
        try { hip_ready.get(); } catch (...) {}
        std::cerr << "Filepath to (H)IBF Index not valid" << std::endl;
        std::cerr << e.what() << '\n';
        return 0;
    }
    const double t_read = now();
    hip_ready.get();
    const double t_hip = now();
    if (n_shards > 1 || devices.size() > 1) dev.upload_sharded(image, devices, n_shards);
    else dev.upload(image, devices[0]);
    if (trace) std::cerr << "[tetrex] index map+parse " << (t_read - t_start) << " s, waited for HIP " << (t_hip - t_read) << " s, upload " << (now() - t_hip) << " s" << std::endl;
    if (a.has("gibf")) dev.attach_dgram(read_dgram_index_file(a.get("gibf", "")));  // include/query.h:259-264
    StagedOptions sopt;
    sopt.gaps.augment = a.has("augment");
    if (a.has("max-ops")) {  // -M / --max-ops (not in the reference): mask operations one query may expand to before it is given up (default 2^33)
        const long long m = std::atoll(a.get("max-ops", "0").c_str());
        if (m > 0) sopt.limits.max_ops = sopt.limits.max_states = (size_t)m;
    }
    const KmerEncoder enc = dev.encoder();
    const uint64_t bins = dev.bins(), W = dev.result_words();
    const VerifyOptions vopt{threads};
    // --gpu-verify: the record filter in front of verification.  On a sharded index it runs on the first device.
    const bool gpu_verify = a.has("gpu-verify");
    // fills `sel` for the masks; false (and an empty selection: verification as without the flag) where a bin cannot be read
    auto filter_records = [&](const std::vector<const uint64_t*>& mptr, const std::vector<std::string>& rxs, RecordSelection& sel, RecordFilter::Stats& fs) {
        try {
            RecordFilter rf(image.bin_paths, enc, threads);
            rf.run(mptr, bins, rxs, sel);
            fs = rf.stats();
            return true;
        } catch (const std::exception& e) {
            std::cerr << e.what() << '\n';
            sel.pairs.clear();
            return false;
        }
    };
    auto print_filter_stats = [&](const RecordFilter::Stats& fs, double find_all_seconds) {
        if (trace)
            std::cerr << "[tetrex] gpu-verify: export " << fs.export_seconds << " s, read + upload " << fs.upload_seconds << " s, filter " << fs.filter_seconds
                      << " s, copy back " << fs.copy_seconds << " s, find_all + rows " << find_all_seconds << " s" << std::endl;
        if (!a.has("stats")) return;
        std::cerr << "{\"gpu_verify\": {\"pairs_device\": " << fs.pairs_device << ", \"pairs_host\": " << fs.pairs_host << ", \"records_flagged\": "
                  << fs.records_flagged << ", \"records_total\": " << fs.records_total << ", \"automata_lds\": " << fs.automata_lds
                  << ", \"automata_l2\": " << fs.automata_l2 << ", \"automata_host\": " << fs.automata_host << "}}" << std::endl;
    };
    // -S/--stats (not in the reference): one JSON line on stderr about the candidate-mask stage
    auto print_stats = [&](const StagedStats& st, size_t queries, double seconds) {
        if (!a.has("stats")) return;
        std::cerr << "{\"queries\": " << queries << ", \"mask_seconds\": " << seconds << ", \"stages\": " << st.stages
                  << ", \"ops\": " << st.ops << ", \"kmer_probes\": " << st.kmers << ", \"states\": " << st.states
                  << ", \"pruned_states\": " << st.pruned << ", \"dense_ops\": " << st.dense_ops << ", \"expand_seconds\": " << st.expand_seconds
                  << ", \"execute_seconds\": " << st.execute_seconds << ", \"bins\": " << bins << "}" << std::endl;
    };

    auto run_one = [&](const std::string& rx, const uint64_t* mask, const std::string& destination, bool log_file_mode, double t1) {
        const size_t narrowed = popcount_mask(mask, W);
        if (verbose) std::cerr << "Narrowed Search to " << narrowed << " possible bins" << std::endl;
        if (log_file_mode) std::cerr << "Bin Count: " << narrowed << "\t";
        if (narrowed) {
            try {
                const std::vector<uint64_t> hit = set_bins(mask, bins);
                RecordSelection sel;
                RecordFilter::Stats fs;
                const bool filtered = gpu_verify && !log_file_mode && filter_records({mask}, {rx}, sel, fs);
                const RecordSelection* selection = filtered ? &sel : nullptr;
                const double t_find = now();
                if (destination == "-") verify_bins(hit, image.bin_paths, rx, enc, std::cout, std::cout, vopt, selection);
                else {
                    std::ofstream f(destination);
                    if (!f) throw std::runtime_error("Failed to open output file: " + destination);
                    verify_bins(hit, image.bin_paths, rx, enc, f, std::cout, vopt, selection);
                }
                if (filtered) print_filter_stats(fs, now() - t_find);
            } catch (const std::exception& e) {
                std::cerr << e.what() << '\n';
            }
        }
        if (verbose || log_file_mode) std::cerr << "Query Time: " << (now() - t1) << std::endl;
    };

    if (bins <= 1)
        std::cerr << "[WARNING] Index contains only 1 bin. Unable to accelerate search using the TetRex algorithm. Performing Linear Scan" << std::endl;

    if (from_file) {  // TSV: id <tab> motif; results go to <id>.tsv (src/query.cpp:342-363, include/query.h:329-339)
        verbose = false;
        std::ifstream in(input);
        if (!in) throw std::runtime_error("Could not open file: " + input);
        std::vector<std::string> ids, motifs;
        for (std::string line; std::getline(in, line);) {
            if (line.empty()) continue;
            const std::vector<std::string> f = split(line, '\t');
            if (f.size() >= 2) { ids.push_back(f[0]); motifs.push_back(f[1]); }
        }
        const double t0 = now();
        std::vector<int> status;
        std::vector<std::string> why;
        StagedStats st;
        const std::vector<uint64_t> masks = dev.query_masks(motifs, &status, &why, &st, &sopt);
        print_stats(st, motifs.size(), now() - t0);
        const double batch = (now() - t0) / std::max<size_t>(1, motifs.size());
        const double t_verify = now();
        int failed = 0;
        // The batch is verified BIN-MAJOR (verify_batch): every candidate bin is read once and all the motifs that selected it run
        // over its records; the reference — and TETREX_VERIFY_PER_MOTIF=1 here, for comparison — verifies motif by motif
        // (include/query.h:329-346), re-reading a bin once per motif.  Files and rows are the same either way.
        std::vector<std::string> fwd, rev;
        bool bin_major = !std::getenv("TETREX_VERIFY_PER_MOTIF");
        if (bin_major) {
            std::vector<const uint64_t*> mptr(motifs.size(), nullptr);
            for (size_t i = 0; i < motifs.size(); ++i)
                if (!status[i]) mptr[i] = masks.data() + i * W;
            RecordSelection sel;
            RecordFilter::Stats fs;
            const bool filtered = gpu_verify && filter_records(mptr, motifs, sel, fs);
            try {
                const double t_find = now();
                verify_batch(mptr, bins, image.bin_paths, motifs, enc, &fwd, &rev, vopt, filtered ? &sel : nullptr);
                if (filtered) print_filter_stats(fs, now() - t_find);
            } catch (const std::exception& e) {  // (a bin that cannot be read: motif by motif, so that the others still get their results)
                std::cerr << e.what() << '\n';
                bin_major = false;
            }
        }
        const double per_motif = bin_major ? (now() - t_verify) / std::max<size_t>(1, motifs.size()) : 0.0;
        for (size_t i = 0; i < motifs.size(); ++i) {
            std::cerr << ids[i] << "\t";
            if (status[i]) {  // its mask is incomplete: verifying the bins it happens to hold would silently lose matches
                std::cerr << "[Error] query not searchable, no result written: " << why[i] << std::endl;
                ++failed;
                continue;
            }
            if (!bin_major) { run_one(motifs[i], masks.data() + i * W, ids[i] + ".tsv", true, now() - batch); continue; }
            const size_t narrowed = popcount_mask(masks.data() + i * W, W);
            std::cerr << "Bin Count: " << narrowed << "\t";
            if (narrowed) {
                std::ofstream f(ids[i] + ".tsv");
                if (!f) std::cerr << "Failed to open output file: " << ids[i] << ".tsv" << '\n';
                else f << fwd[i];
                std::cout << rev[i];
            }
            std::cerr << "Query Time: " << (batch + per_motif) << std::endl;  // (the batch's time, shared out evenly)
        }
        // -S: the whole batch as the reference times a query — from after the index is loaded to the last output byte
        // (include/query.h:256,287-289): candidate masks + verification of the candidate bins
        if (a.has("stats"))
            std::cerr << "{\"batch_seconds\": " << (now() - t0) << ", \"verify_seconds\": " << (now() - t_verify) << ", \"threads\": " << vopt.threads
                      << ", \"refused\": " << failed << "}" << std::endl;
        return failed ? 1 : 0;
    }
    if (conj) {
        const std::vector<std::string> queries = split(input, ':');
        if (queries.size() == 1) { std::cerr << "Did you use the correct delimiter (:)?" << std::endl; return 0; }
        const double t1 = now();
        StagedStats st;
        std::vector<int> status;
        std::vector<std::string> why;
        const std::vector<uint64_t> masks = dev.query_masks(queries, &status, &why, &st, &sopt);
        print_stats(st, queries.size(), now() - t1);
        for (size_t q = 0; q < queries.size(); ++q)
            if (status[q]) {  // ANDing a partial mask would drop true candidate bins without a word
                std::cerr << "[Error] query not searchable: " << queries[q] << ": " << why[q] << std::endl;
                return 1;
            }
        std::vector<uint64_t> all(masks.begin(), masks.begin() + W);
        for (size_t q = 1; q < queries.size(); ++q)
            for (uint64_t w = 0; w < W; ++w) all[w] &= masks[q * W + w];
        if (verbose) std::cerr << "Narrowed Search to " << popcount_mask(all.data(), W) << " possible bins" << std::endl;
        if (popcount_mask(all.data(), W)) verify_conjunction(set_bins(all.data(), bins), image.bin_paths, queries, std::cout, vopt);
        if (verbose) std::cerr << "Query Time: " << (now() - t1) << std::endl;
        return 0;
    }
    if (a.has("draw")) {  // include/query.h:244: kgraph_visualizer.gv in the working directory
        try {
            KGraph g = build_kgraph(preprocess_query(input, enc), enc.k(), enc.alphabet() != Alphabet::Base);
            if (sopt.gaps.augment) g.augment();
            std::ofstream("kgraph_visualizer.gv") << g.to_graphviz();
        } catch (const std::exception& e) {
            std::cerr << "[WARNING] could not draw the k-graph: " << e.what() << std::endl;
        }
    }
    const double t1 = now();
    std::vector<int> status;
    std::vector<std::string> why;
    StagedStats st;
    const std::vector<uint64_t> masks = dev.query_masks({input}, &status, &why, &st, &sopt);
    print_stats(st, 1, now() - t1);
    if (status[0]) { std::cerr << "[Error] query not searchable: " << why[0] << std::endl; return 1; }
    run_one(input, masks.data(), dest, false, t1);
    return 0;
}

int cmd_index(int argc, char** argv) {
    const std::vector<OptSpec> spec = {{'k', "ksize", true}, {'p', "fpr", true}, {'c', "hash_count", true}, {'t', "threads", true},
                                       {'n', "nucleic_acid", false}, {'i', "ibf", false}, {'r', "reduce", true}, {'D', "device", true},
                                       {'W', "no-wraparound", false}, {'\0', "layout", true}, {'\0', "tmax", true},
                                       {'\0', "rearrange", false}, {'\0', "rearrange-ratio", true}};
    Args a;
    try {
        a = parse(argc, argv, 2, spec);
        if (a.pos.size() < 2) throw std::runtime_error("expected <name> <libraries...>");
    } catch (const std::exception& e) {
        std::cerr << "[Indexing Parser Error] " << e.what() << "\n";
        return 0;
    }
    BuildOptions opt;
    opt.k = (unsigned)std::atoi(a.get("ksize", "6").c_str());
    opt.fpr = std::strtof(a.get("fpr", "0.05").c_str(), nullptr);
    opt.hash_count = (unsigned)std::atoi(a.get("hash_count", "3").c_str());
    opt.dna = a.has("nucleic_acid");
    opt.hibf = !a.has("ibf");
    opt.dna_wraparound = !a.has("no-wraparound");
    opt.device = std::atoi(a.get("device", "0").c_str());
    const std::string red = a.get("reduce", "None");
    if (red == "murphy") opt.reduction = 1;
    else if (red == "li") opt.reduction = 2;
    else if (red != "None") { std::cerr << "[Indexing Parser Error] reduce must be murphy or li\n"; return 0; }
    // --layout uniform|sized [--tmax N] (not in the reference): the HIBF's layout, host/layout.hpp
    const std::string layout = a.get("layout", "uniform");
    if (a.has("layout") && a.has("ibf")) { std::cerr << "[Indexing Parser Error] --layout is an HIBF option: not with -i\n"; return 0; }
    if (layout == "sized") opt.layout = BuildOptions::kSized;
    else if (layout != "uniform") { std::cerr << "[Indexing Parser Error] --layout must be uniform or sized\n"; return 0; }
    if (a.has("tmax")) {
        const std::string t = a.get("tmax", "");
        char* end = nullptr;
        const unsigned long long v = std::strtoull(t.c_str(), &end, 10);
        if (opt.layout != BuildOptions::kSized) { std::cerr << "[Indexing Parser Error] --tmax needs --layout sized\n"; return 0; }
        if (t.empty() || *end || v == 0 || v % 64) { std::cerr << "[Indexing Parser Error] --tmax must be a positive multiple of 64\n"; return 0; }
        opt.tmax = v;
    }
    // --rearrange [--rearrange-ratio R]: similar bins side by side before the sized layout (host/layout.hpp).  The flag takes
    // no value of its own: an optional one would swallow the index name that follows it.
    if (a.has("rearrange") && opt.layout != BuildOptions::kSized) { std::cerr << "[Indexing Parser Error] --rearrange needs --layout sized\n"; return 0; }
    if (a.has("rearrange-ratio") && !a.has("rearrange")) { std::cerr << "[Indexing Parser Error] --rearrange-ratio needs --rearrange\n"; return 0; }
    if (a.has("rearrange")) {
        const std::string t = a.get("rearrange-ratio", "0.5");
        char* end = nullptr;
        const double v = std::strtod(t.c_str(), &end);
        if (t.empty() || *end || !(v > 0 && v <= 1)) { std::cerr << "[Indexing Parser Error] --rearrange-ratio must be a number in (0, 1]\n"; return 0; }
        opt.rearrange_ratio = v;
    }
    if (!opt.dna && opt.k > 12) { std::cerr << "[Indexing Parser Error] Max kmer size for amino acids is 12" << "\n"; return 0; }
    std::vector<std::string> files;
    for (size_t i = 1; i < a.pos.size(); ++i) {
        const std::filesystem::path p = a.pos[i];
        if (p.extension() == ".lst") {
            std::ifstream in(p);
            if (!in) throw std::runtime_error("Could not open file " + p.string() + " for reading.");
            for (std::string line; std::getline(in, line);) files.push_back(line);
        } else files.push_back(std::filesystem::absolute(p).string());
    }
    size_t seqs = 0;
    const IndexImage img = build_index(files, opt, &seqs);
    std::cerr << "Indexed " << seqs << " sequences across " << files.size() << " bins." << std::endl;
    if (files.size() == 1)
        std::cerr << "[WARNING] The indexed reference library was not split into bins. The TetRex runtime will be significantly slower." << std::endl;
    std::cerr << "Writing to disk... ";
    write_index_file(a.pos[0] + ".ibf", img);
    std::cerr << "DONE" << std::endl;
    return 0;
}

// tetrex track [-l lower] [-u upper] [-n] [-i] <name> <libs...>   (include/arg_parse.h:94-122, src/dGramIndex.cpp:22-38)
int cmd_track(int argc, char** argv) {
    const std::vector<OptSpec> spec = {{'l', "lower", true}, {'u', "upper", true}, {'n', "nucleic_acid", false}, {'i', "ibf", false},
                                       {'D', "device", true}};
    Args a;
    try {
        a = parse(argc, argv, 2, spec);
        if (a.pos.size() < 2) throw std::runtime_error("expected <name> <libraries...>");
    } catch (const std::exception& e) {
        std::cerr << "[Error TetRex Dgram Indexing module " << e.what() << "\n";
        return 0;
    }
    std::vector<std::string> files;
    for (size_t i = 1; i < a.pos.size(); ++i) {
        const std::filesystem::path p = a.pos[i];
        if (p.extension() == ".lst") {
            std::ifstream in(p);
            if (!in) throw std::runtime_error("Could not open file " + p.string() + " for reading.");
            for (std::string line; std::getline(in, line);) files.push_back(line);
        } else files.push_back(std::filesystem::absolute(p).string());
    }
    const DgramImage d = build_dgram_index(files, std::strtoull(a.get("lower", "3").c_str(), nullptr, 10),
                                           std::strtoull(a.get("upper", "21").c_str(), nullptr, 10), 3, 0.05f,
                                           std::atoi(a.get("device", "0").c_str()));
    write_dgram_index_file(a.pos[0], d);  // the reference writes the name as given, no extension
    return 0;
}

// --align: the two columns behind a confirmed row, \t start \t cigar — start 1-based (end + 1 for a match that takes
// no target letter), the cigar like 12=1X30=2I7= ('I': a query letter with no target letter, 'D': a target letter skipped)
void append_alignment(std::string& row, const VerifiedHit& h) {
    row.append("\t").append(std::to_string((uint64_t)h.start + 1)).append("\t");
    for (const uint32_t run : h.runs) row.append(std::to_string(run >> 2)).append(1, "=XID"[run & 3]);
}
void trace_align_routes(const BinVerifier& verifier) {
    const BinVerifier::Aligned n = verifier.n_aligned();
    std::cerr << "[tetrex search] align routes: device " << n.device << ", host " << n.host << std::endl;
}

// tetrex search --translate: nucleotide records on a peptide index.  Every record is translated in its six
// frames on the device; frame f of a record is a query of its own with n_f values (the k-mers of the frame without a stop)
// and the plain rules with n = n_f: -e E gives t = max(n_f - k E, 0), --threshold F gives t = ceil(F n_f).  A frame with
// n_f = 0 or t = 0 reports nothing (a wrong frame is short and full of stops: "every bin" for it would be noise); a record
// none of whose frames is searched gets a note.  Rows: name \t bin path \t frame [\t count/n_f], by record, frame
// (+1 +2 +3 -1 -2 -3) and bin.  -e E --verify-frames: the rows are candidates; each is confirmed by the edit
// distance of the frame's residue letters to the bin's records (BinVerifier, the frames translated on the device) and only
// those within E edits are written, with distance \t target \t end appended; --align appends \t start \t cigar (append_alignment).
int search_translated(const Args& a, const IndexImage& image, unsigned long long errors, double fraction) {
    const bool verbose = a.has("verbose"), with_counts = a.has("counts"), by_fraction = a.has("threshold");
    const std::string dest = a.get("output", "-");
    const double t_start = now();
    DeviceIndex dev;
    dev.upload(image, std::atoi(a.get("device", "0").c_str()));
    const uint64_t k = dev.encoder().k();
    std::ofstream file;
    if (dest != "-") {
        file.open(dest);
        if (!file) throw std::runtime_error("Failed to open output file: " + dest);
    }
    std::ostream& out = dest == "-" ? std::cout : file;
    static const char* const kFrames[6] = {"+1", "+2", "+3", "-1", "-2", "-3"};
    const auto threshold_of = [&](uint64_t n) -> uint64_t {
        if (by_fraction) return (uint64_t)std::ceil(fraction * (double)n);
        return n > k * errors ? n - k * errors : 0;
    };
    // records go to the device in chunks of their bytes (search_translated cuts a chunk into batches of values)
    const size_t max_bytes = (size_t)64 << 20, max_records = (size_t)1 << 20;
    std::vector<std::string> names;
    std::string seq, row;
    std::vector<uint64_t> rec_offsets{0}, n_of, thresholds;
    std::vector<DeviceIndex::TranslatedHit> hits;
    // --verify-frames: every row is a candidate (frame, bin); only those within E residue edits are written
    const bool verify = a.has("verify-frames");
    std::unique_ptr<BinVerifier> verifier;
    if (verify) verifier = std::make_unique<BinVerifier>(image.bin_paths, false, (uint32_t)std::min<unsigned long long>(errors, 0xFFFFFFFEull));
    const bool align = verify && a.has("align");
    if (align) verifier->set_align(true);
    const bool all_targets = verify && a.has("all-targets");  // a row per target, not per bin
    std::vector<BinVerifier::Hit> confirmed;
    std::vector<std::vector<BinVerifier::Hit>> targets;
    auto flush = [&]() {
        if (names.empty()) return;
        dev.search_translated(seq, rec_offsets, threshold_of, with_counts, n_of, thresholds, hits, verifier.get(), verify ? &confirmed : nullptr,
                              all_targets ? &targets : nullptr);
        size_t h = 0;
        for (size_t r = 0; r < names.size(); ++r) {
            bool searched = false;
            for (size_t f = 0; f < 6; ++f) searched = searched || thresholds[6 * r + f] > 0;
            if (!searched)
                std::cerr << "[tetrex search] " << names[r] << ": no frame with " << k << "-mers enough for a threshold above 0, skipped" << std::endl;
            for (; h < hits.size() && hits[h].query < 6 * (r + 1); ++h) {
                const DeviceIndex::TranslatedHit& x = hits[h];
                const auto write = [&](const BinVerifier::Hit* v) {
                    row.assign(names[r]).append("\t").append(image.bin_paths[x.bin]).append("\t").append(kFrames[x.query % 6]);
                    if (with_counts) row.append("\t").append(std::to_string(x.count)).append("/").append(std::to_string(n_of[x.query]));
                    if (v) row.append("\t").append(std::to_string(v->distance)).append("\t").append(*v->target).append("\t").append(std::to_string(v->end));
                    if (align) append_alignment(row, *v);
                    out << row << '\n';
                };
                if (all_targets) {
                    for (const BinVerifier::Hit& v : targets[h]) write(&v);
                    continue;
                }
                if (verify && confirmed[h].distance == 0xFFFFFFFFu) continue;
                write(verify ? &confirmed[h] : nullptr);
            }
        }
        names.clear();
        seq.clear();
        rec_offsets.assign(1, 0);
    };
    for_each_record(a.pos[1], [&](const FastaRecord& r) {
        if (!names.empty() && (seq.size() + r.seq.size() > max_bytes || names.size() >= max_records)) flush();
        names.push_back(r.name);
        seq.append(r.seq);
        rec_offsets.push_back(seq.size());
    });
    flush();
    out.flush();
    if (verbose && verify) std::cerr << "Verified: " << verifier->n_confirmed() << " of " << verifier->n_candidates() << " candidate pairs" << std::endl;
    if (verbose && all_targets) std::cerr << "Targets: " << verifier->n_targets() << std::endl;
    if (verify && std::getenv("TETREX_TRACE")) {
        const BinVerifier::Routed n = verifier->n_routed();
        std::cerr << "[tetrex search] verify routes: device " << n.device << ", device-long " << n.device_long << ", host " << n.host << std::endl;
        if (align) trace_align_routes(*verifier);
    }
    if (verbose) std::cerr << "Search time: " << (now() - t_start) << " s" << std::endl;
    return 0;
}

// tetrex search --window W [--step S]: a local search for records longer than what they match.  A record of
// L letters is cut into windows of W letters at letter offsets 0, S, 2 S, ... while offset + W <= L, and one more at L - W where
// the last of these ends before L (every letter is covered); a record of at most W letters is one window.  A window of l
// letters has w = l - k + 1 values and the plain rules with n = w: -e E gives t = max(w - k E, 0), --threshold F gives
// t = ceil(F w).  A window with t = 0 is not searched and reports nothing; a record that had such a window gets one note.
// All windows of a batch of records are counted on the device by sliding (txq_count_windows_device) and only the hit list
// comes back.  Rows: for each (record, bin) every maximal run of consecutive hit windows is one row,
// name \t bin path \t begin \t end [\t count/w], begin and end the 1-based inclusive letter positions of the run's union,
// count/w those of the run's best window (the highest count, the earliest on a tie); by record, bin, begin.
int search_windowed(const Args& a, const IndexImage& image, unsigned long long errors, double fraction, uint64_t window, uint64_t step) {
    const bool verbose = a.has("verbose"), with_counts = a.has("counts"), by_fraction = a.has("threshold");
    const std::string dest = a.get("output", "-");
    const double t_start = now();
    DeviceIndex dev;
    dev.upload(image, std::atoi(a.get("device", "0").c_str()));
    const KmerEncoder enc = dev.encoder();
    const uint64_t k = enc.k();
    std::ofstream file;
    if (dest != "-") {
        file.open(dest);
        if (!file) throw std::runtime_error("Failed to open output file: " + dest);
    }
    std::ostream& out = dest == "-" ? std::cout : file;
    // records are collected up to 2^24 values (one longer record: alone); search_windows cuts their windows into device batches
    const size_t max_values = (size_t)1 << 24, max_windows = (size_t)1 << 22;
    struct Rec { std::string name; size_t w0, w1; };  // its windows [w0, w1)
    std::vector<Rec> recs;
    std::vector<uint64_t> values, begins, letter_at;  // letter_at[j]: the 0-based letter offset of window j in its record
    std::vector<uint32_t> lens, thresholds;
    std::vector<DeviceIndex::TranslatedHit> hits;
    std::string row;
    uint64_t n_searched = 0, n_hit = 0, n_rows = 0;
    auto flush = [&]() {
        if (recs.empty()) return;
        dev.search_windows(values, begins, lens, thresholds, with_counts, hits);
        size_t h = 0;
        std::vector<DeviceIndex::TranslatedHit> mine;
        for (const Rec& r : recs) {
            mine.clear();
            for (; h < hits.size() && hits[h].query < r.w1; ++h) mine.push_back(hits[h]);
            if (verbose) {
                for (size_t i = 0; i < mine.size(); ++i) n_hit += i == 0 || mine[i].query != mine[i - 1].query;
            }
            std::stable_sort(mine.begin(), mine.end(), [](const DeviceIndex::TranslatedHit& x, const DeviceIndex::TranslatedHit& y) { return x.bin < y.bin; });
            for (size_t i = 0; i < mine.size();) {  // a run: the same bin, windows j, j + 1, ...
                size_t e = i + 1, best = i;
                while (e < mine.size() && mine[e].bin == mine[i].bin && mine[e].query == mine[e - 1].query + 1) {
                    if (mine[e].count > mine[best].count) best = e;
                    ++e;
                }
                const uint32_t jf = mine[i].query, jl = mine[e - 1].query;
                row.assign(r.name).append("\t").append(image.bin_paths[mine[i].bin]).append("\t").append(std::to_string(letter_at[jf] + 1));
                row.append("\t").append(std::to_string(letter_at[jl] + lens[jl] + k - 1));
                if (with_counts) row.append("\t").append(std::to_string(mine[best].count)).append("/").append(std::to_string(lens[mine[best].query]));
                out << row << '\n';
                ++n_rows;
                i = e;
            }
        }
        recs.clear();
        values.clear();
        begins.clear();
        letter_at.clear();
        lens.clear();
        thresholds.clear();
    };
    std::vector<uint64_t> v;
    for_each_record(a.pos[1], [&](const FastaRecord& r) {
        v.clear();
        enc.record_values(r.seq, false, v);
        const uint64_t L = r.seq.size();
        if (v.empty()) {
            std::cerr << "[tetrex search] " << r.name << ": no k-mer of length " << k << ", skipped" << std::endl;
            return;
        }
        if (!recs.empty() && (values.size() + v.size() > max_values || begins.size() >= max_windows)) flush();
        const uint64_t base = values.size();
        values.insert(values.end(), v.begin(), v.end());
        Rec rec{r.name, begins.size(), 0};
        bool unsearched = false;
        const auto add = [&](uint64_t at, uint64_t letters) {
            const uint64_t w = letters - k + 1;
            uint64_t t;
            if (by_fraction) t = (uint64_t)std::ceil(fraction * (double)w);
            else t = w > k * errors ? w - k * errors : 0;
            unsearched = unsearched || t == 0;
            n_searched += t != 0;
            begins.push_back(base + at);
            letter_at.push_back(at);
            lens.push_back((uint32_t)w);
            thresholds.push_back((uint32_t)std::min<uint64_t>(t, 0xFFFFFFFEull));
        };
        if (L <= window) add(0, L);
        else {
            uint64_t at = 0;
            for (; at + window <= L; at += step) add(at, window);
            if (at - step + window < L) add(L - window, window);
        }
        rec.w1 = begins.size();
        recs.push_back(std::move(rec));
        if (unsearched) std::cerr << "[tetrex search] " << r.name << ": a window with threshold 0 is not searched" << std::endl;
    });
    flush();
    out.flush();
    if (verbose) std::cerr << "Windows: " << n_searched << " searched, " << n_hit << " hit, " << n_rows << " rows" << std::endl;
    if (verbose) std::cerr << "Search time: " << (now() - t_start) << " s" << std::endl;
    return 0;
}

// tetrex search --translate --frame-window W [--frame-step S]: the local search of --window in the six frames
// of nucleotide records.  A frame of R residues is cut like a record of R letters under --window (W and S count residues); a
// window is a query of its own with w = its stop-free k-mers — what n_f is to --translate — and t = max(w - k E, 0) or
// ceil(F w).  A window with t = 0 is not searched and reports nothing; a record none of whose windows is searched gets one
// note (wrong frames are full of stops: a note per window would be noise), a record with no k-mer in any window the note of
// --translate.  Translation, the windows' value ranges and the sliding count all stay on the device
// (DeviceIndex::search_translated_windows); the windows' w and the hit list come back.  Rows: for each (record, frame, bin)
// every maximal run of consecutive hit windows is one row, name \t bin path \t frame \t begin \t end [\t count/w]: begin and end
// the 1-based inclusive nucleotide positions of the run's residues on the record as given (begin <= end; the frame carries
// the strand), count/w those of the run's best window (the highest count, the earliest on a tie); by record, frame
// (+1 +2 +3 -1 -2 -3), bin, begin.
int search_translated_windowed(const Args& a, const IndexImage& image, unsigned long long errors, double fraction, uint32_t window, uint32_t step) {
    const bool verbose = a.has("verbose"), with_counts = a.has("counts"), by_fraction = a.has("threshold");
    const std::string dest = a.get("output", "-");
    const double t_start = now();
    DeviceIndex dev;
    dev.upload(image, std::atoi(a.get("device", "0").c_str()));
    const uint64_t k = dev.encoder().k();
    std::ofstream file;
    if (dest != "-") {
        file.open(dest);
        if (!file) throw std::runtime_error("Failed to open output file: " + dest);
    }
    std::ostream& out = dest == "-" ? std::cout : file;
    static const char* const kFrames[6] = {"+1", "+2", "+3", "-1", "-2", "-3"};
    const auto threshold_of = [&](uint64_t n) -> uint64_t {
        if (by_fraction) return (uint64_t)std::ceil(fraction * (double)n);
        return n > k * errors ? n - k * errors : 0;
    };
    // records go to the device in chunks of their bytes (search_translated_windows cuts a chunk into batches of values)
    const size_t max_bytes = (size_t)64 << 20, max_records = (size_t)1 << 20;
    std::vector<std::string> names;
    std::string seq, row;
    std::vector<uint64_t> rec_offsets{0}, win_offsets;
    std::vector<uint32_t> lens, thresholds;
    std::vector<DeviceIndex::TranslatedHit> hits, mine;
    uint64_t n_searched = 0, n_hit = 0, n_rows = 0;
    auto flush = [&]() {
        if (names.empty()) return;
        dev.search_translated_windows(seq, rec_offsets, window, step, threshold_of, with_counts, win_offsets, lens, thresholds, hits);
        size_t h = 0;
        for (size_t r = 0; r < names.size(); ++r) {
            const uint64_t L = rec_offsets[r + 1] - rec_offsets[r];
            bool searched = false, any_kmer = false;
            for (uint64_t j = win_offsets[6 * r]; j < win_offsets[6 * r + 6]; ++j) {
                searched = searched || thresholds[j] > 0;
                any_kmer = any_kmer || lens[j] > 0;
                n_searched += thresholds[j] > 0;
            }
            if (!any_kmer)
                std::cerr << "[tetrex search] " << names[r] << ": no frame with " << k << "-mers enough for a threshold above 0, skipped" << std::endl;
            else if (!searched)
                std::cerr << "[tetrex search] " << names[r] << ": no window with a threshold above 0, not searched" << std::endl;
            for (uint32_t f = 0; f < 6; ++f) {
                const uint64_t w0 = win_offsets[6 * r + f], w1 = win_offsets[6 * r + f + 1];
                mine.clear();
                for (; h < hits.size() && hits[h].query < w1; ++h) mine.push_back(hits[h]);
                if (mine.empty()) continue;
                const txq::fw::Frame plan = txq::fw::frame_plan(txq::tr::frame_len(L, f % 3), (uint32_t)k, window, step);
                for (size_t i = 0; i < mine.size(); ++i) n_hit += i == 0 || mine[i].query != mine[i - 1].query;
                std::stable_sort(mine.begin(), mine.end(), [](const DeviceIndex::TranslatedHit& x, const DeviceIndex::TranslatedHit& y) { return x.bin < y.bin; });
                for (size_t i = 0; i < mine.size();) {  // a run: the same bin, windows j, j + 1, ...
                    size_t e = i + 1, best = i;
                    while (e < mine.size() && mine[e].bin == mine[i].bin && mine[e].query == mine[e - 1].query + 1) {
                        if (mine[e].count > mine[best].count) best = e;
                        ++e;
                    }
                    const txq::fw::Window wf = txq::fw::window_at(plan, mine[i].query - w0), wl = txq::fw::window_at(plan, mine[e - 1].query - w0);
                    const txq::fw::Span at = txq::fw::residues_on_record(L, f, wf.a, wl.a + wl.len);
                    row.assign(names[r]).append("\t").append(image.bin_paths[mine[i].bin]).append("\t").append(kFrames[f]);
                    row.append("\t").append(std::to_string(at.begin)).append("\t").append(std::to_string(at.end));
                    if (with_counts) row.append("\t").append(std::to_string(mine[best].count)).append("/").append(std::to_string(lens[mine[best].query]));
                    out << row << '\n';
                    ++n_rows;
                    i = e;
                }
            }
        }
        names.clear();
        seq.clear();
        rec_offsets.assign(1, 0);
    };
    for_each_record(a.pos[1], [&](const FastaRecord& r) {
        if (!names.empty() && (seq.size() + r.seq.size() > max_bytes || names.size() >= max_records)) flush();
        names.push_back(r.name);
        seq.append(r.seq);
        rec_offsets.push_back(seq.size());
    });
    flush();
    out.flush();
    if (verbose) std::cerr << "Windows: " << n_searched << " searched, " << n_hit << " hit, " << n_rows << " rows" << std::endl;
    if (verbose) std::cerr << "Search time: " << (now() - t_start) << " s" << std::endl;
    return 0;
}

// tetrex search: each record of the query file is a query; its values are the index's k-mers of the record (n of them) and a
// bin is reported when at least t of them are in it (txq_count).  -e E: t = max(n - k E, 0) — a record within E edits of a
// substring of a bin shares at least n - k E k-mer positions with it (q-gram lemma), and a Bloom filter drops none of them,
// so that bin is always reported.  --threshold F (0 < F <= 1): t = ceil(F n).  Rows: name \t bin path [\t count/n].
// -e E --verify: the reported bins are candidates; each is confirmed by the edit distance of the record to the
// bin's records (BinVerifier) and only the bins within E edits are written, with distance \t target \t end [\t strand] appended.
// --align (with --verify or --verify-frames) appends \t start \t cigar to each of those rows; on strand - the cigar is
// that of the reverse-complemented record against the target, in the target's coordinates.
int cmd_search(int argc, char** argv) {
    const std::vector<OptSpec> spec = {{'e', "errors", true}, {'\0', "threshold", true}, {'\0', "counts", false}, {'o', "output", true},
                                       {'v', "verbose", false}, {'D', "device", true}, {'\0', "translate", false}, {'\0', "verify", false},
                                       {'\0', "verify-frames", false}, {'\0', "align", false}, {'\0', "all-targets", false},
                                       {'\0', "window", true}, {'\0', "step", true}, {'\0', "frame-window", true}, {'\0', "frame-step", true}};
    Args a;
    unsigned long long errors = 0, window = 0, step = 0, frame_window = 0, frame_step = 0;
    double fraction = 0;
    try {
        a = parse(argc, argv, 2, spec);
        if (a.pos.size() != 2) throw std::runtime_error("expected <index> <queries.fa>");
        if (a.has("step") && !a.has("window")) throw std::runtime_error("--step is the distance between the windows of --window W: it needs --window");
        if (a.has("frame-step") && !a.has("frame-window"))
            throw std::runtime_error("--frame-step is the distance between the windows of --frame-window W: it needs --frame-window");
        if (a.has("frame-window")) {
            if (!a.has("translate")) throw std::runtime_error("--frame-window cuts the translated frames of --translate into windows: it needs --translate");
            if (a.has("window")) throw std::runtime_error("--frame-window cannot be combined with --window: one counts residues of a translated frame, the other letters of the record");
            if (a.has("step")) throw std::runtime_error("--frame-window cannot be combined with --step: the distance between frame windows is --frame-step");
            if (a.has("verify-frames")) throw std::runtime_error("--frame-window cannot be combined with --verify-frames: frame windows are not verified in this version");
            if (a.has("all-targets")) throw std::runtime_error("--frame-window cannot be combined with --all-targets: frame windows are not verified in this version");
            if (a.has("align")) throw std::runtime_error("--frame-window cannot be combined with --align: frame windows are not verified in this version");
            if (a.has("verify")) throw std::runtime_error("--frame-window cannot be combined with --verify: frame windows are not verified in this version");
            if (!a.has("errors") && !a.has("threshold")) throw std::runtime_error("--frame-window needs -e E or --threshold F");
            const std::string w = a.get("frame-window", "");
            char* end = nullptr;
            frame_window = std::strtoull(w.c_str(), &end, 10);
            if (w.empty() || *end || w[0] == '-' || frame_window == 0 || frame_window > 0x7FFFFFFFull)
                throw std::runtime_error("--frame-window must be a number of residues >= k");
            frame_step = std::max<unsigned long long>(1, frame_window / 2);
            if (a.has("frame-step")) {
                const std::string s = a.get("frame-step", "");
                frame_step = std::strtoull(s.c_str(), &end, 10);
                if (s.empty() || *end || s[0] == '-' || frame_step < 1 || frame_step > frame_window)
                    throw std::runtime_error("--frame-step must be a number of residues in 1 .. --frame-window");
            }
        }
        if (a.has("window")) {
            if (a.has("translate")) throw std::runtime_error("--window cannot be combined with --translate: translated frames lose their positions where stops are taken out (translated records: --frame-window)");
            if (a.has("verify-frames")) throw std::runtime_error("--window cannot be combined with --verify-frames: it confirms translated frames, which --window does not search");
            if (a.has("all-targets")) throw std::runtime_error("--window cannot be combined with --all-targets: windows are not verified in this version");
            if (a.has("align")) throw std::runtime_error("--window cannot be combined with --align: windows are not verified in this version");
            if (a.has("verify")) throw std::runtime_error("--window cannot be combined with --verify: windows are not verified in this version");
            if (!a.has("errors") && !a.has("threshold")) throw std::runtime_error("--window needs -e E or --threshold F");
            const std::string w = a.get("window", "");
            char* end = nullptr;
            window = std::strtoull(w.c_str(), &end, 10);
            if (w.empty() || *end || w[0] == '-' || window == 0 || window > 0x7FFFFFFFull) throw std::runtime_error("--window must be a number of letters >= k");
            step = std::max<unsigned long long>(1, window / 2);
            if (a.has("step")) {
                const std::string s = a.get("step", "");
                step = std::strtoull(s.c_str(), &end, 10);
                if (s.empty() || *end || s[0] == '-' || step < 1 || step > window) throw std::runtime_error("--step must be a number of letters in 1 .. --window");
            }
        }
        if (a.has("verify-frames")) {
            if (a.has("verify")) throw std::runtime_error("--verify-frames cannot be combined with --verify: one confirms translated frames, the other plain records");
            if (!a.has("translate")) throw std::runtime_error("--verify-frames confirms the rows of --translate: it needs --translate");
            if (a.has("threshold")) throw std::runtime_error("--verify-frames confirms the bins of -e E: it cannot be combined with --threshold");
            if (!a.has("errors")) throw std::runtime_error("--verify-frames needs -e E: the number of residue edits a confirmed frame may be away");
        }
        if (a.has("align") && !a.has("verify") && !a.has("verify-frames"))
            throw std::runtime_error("--align gives the alignment of confirmed rows: it needs --verify, or --translate --verify-frames");
        if (a.has("all-targets") && !a.has("verify") && !a.has("verify-frames"))
            throw std::runtime_error("--all-targets lists every target of confirmed rows: it needs -e E --verify, or --translate -e E --verify-frames");
        if (a.has("verify") && a.has("threshold")) throw std::runtime_error("--verify confirms the bins of -e E: it cannot be combined with --threshold");
        if (a.has("verify") && a.has("translate")) throw std::runtime_error("--verify cannot be combined with --translate (translated rows are confirmed with --verify-frames)");
        if (a.has("verify") && !a.has("errors")) throw std::runtime_error("--verify needs -e E: the number of edits a confirmed bin may be away");
        if (a.has("errors") && a.has("threshold")) throw std::runtime_error("-e and --threshold exclude each other");
        if (a.has("errors")) {
            const std::string e = a.get("errors", "");
            char* end = nullptr;
            errors = std::strtoull(e.c_str(), &end, 10);
            if (e.empty() || *end || e[0] == '-') throw std::runtime_error("-e must be a number of errors >= 0");
        }
        if (a.has("threshold")) {
            const std::string f = a.get("threshold", "");
            char* end = nullptr;
            fraction = std::strtod(f.c_str(), &end);
            if (f.empty() || *end || !(fraction > 0.0 && fraction <= 1.0)) throw std::runtime_error("--threshold must be a fraction in (0, 1]");
        }
    } catch (const std::exception& e) {
        std::cerr << "[Search Parser Error] " << e.what() << "\n";
        return 1;
    }
    const bool verbose = a.has("verbose"), with_counts = a.has("counts");
    const std::string dest = a.get("output", "-");
    const double t_start = now();
    IndexImage image;
    try {
        image = read_index_file(a.pos[0]);
    } catch (const std::exception& e) {
        std::cerr << "Filepath to (H)IBF Index not valid" << std::endl;
        std::cerr << e.what() << '\n';
        return 1;
    }
    if (a.has("translate")) {
        if (image.molecule == "na" || image.k < 1 || image.k > 12) {
            std::cerr << "[tetrex search] --translate needs a peptide index with k in 1..12: " << a.pos[0] << " is a "
                      << (image.molecule == "na" ? "nucleotide index" : "peptide index with k = " + std::to_string(image.k)) << std::endl;
            return 1;
        }
        if (a.has("frame-window")) {
            const unsigned long long k = image.k;
            if (frame_window < k) {
                std::cerr << "[Search Parser Error] --frame-window must be a number of residues >= k: the index has k = " << k << "\n";
                return 1;
            }
            // -e E: a stop-free window has w = W - k + 1 values and t = max(w - k E, 0); with t = 0 no window at all would be searched
            if (a.has("errors") && (errors > 0xFFFFFFFFull || frame_window - k + 1 <= k * errors)) {
                std::cerr << "[Search Parser Error] --frame-window " << frame_window << " with -e " << errors << " leaves every window a threshold of 0 (k = "
                          << k << "): the smallest workable --frame-window is " << (k * errors + k) << "\n";
                return 1;
            }
            return search_translated_windowed(a, image, errors, fraction, (uint32_t)frame_window, (uint32_t)frame_step);
        }
        return search_translated(a, image, errors, fraction);
    }
    if (a.has("window")) {
        const unsigned long long k = image.k;
        if (window < k) {
            std::cerr << "[Search Parser Error] --window must be a number of letters >= k: the index has k = " << k << "\n";
            return 1;
        }
        // -e E: a full window has w = W - k + 1 values and t = max(w - k E, 0); with t = 0 no full window would be searched
        if (a.has("errors") && (errors > 0xFFFFFFFFull || window - k + 1 <= k * errors)) {
            std::cerr << "[Search Parser Error] --window " << window << " with -e " << errors << " leaves every window a threshold of 0 (k = " << k
                      << "): the smallest workable --window is " << (k * errors + k) << "\n";
            return 1;
        }
        return search_windowed(a, image, errors, fraction, window, step);
    }
    DeviceIndex dev;
    dev.upload(image, std::atoi(a.get("device", "0").c_str()));
    const KmerEncoder enc = dev.encoder();
    const uint64_t bins = dev.bins(), W = dev.result_words();
    std::ofstream file;
    if (dest != "-") {
        file.open(dest);
        if (!file) throw std::runtime_error("Failed to open output file: " + dest);
    }
    std::ostream& out = dest == "-" ? std::cout : file;
    // queries go to the device in batches: at most 2^24 values, and at most 256 MiB of counts
    const size_t max_values = (size_t)1 << 24, max_queries = std::max<size_t>(1, ((size_t)256 << 20) / (W * 64 * 4));
    std::vector<std::string> names;
    std::vector<uint64_t> values, offsets{0}, n_of;
    std::vector<uint32_t> thresholds, counts;
    std::vector<uint64_t> hits;
    std::string row;
    const bool verify = a.has("verify"), dna = enc.molecule() == Molecule::DNA;
    std::unique_ptr<BinVerifier> verifier;
    if (verify) verifier = std::make_unique<BinVerifier>(image.bin_paths, dna, (uint32_t)std::min<unsigned long long>(errors, 0xFFFFFFFEull));
    const bool align = verify && a.has("align");
    if (align) verifier->set_align(true);
    const bool all_targets = verify && a.has("all-targets");  // a row per target, not per bin
    std::vector<std::string> seqs;  // --verify: the batch's records themselves
    std::vector<BinVerifier::Candidate> candidates;
    std::vector<BinVerifier::Hit> confirmed;
    std::vector<std::vector<BinVerifier::Hit>> targets;
    auto flush = [&]() {
        if (names.empty()) return;
        dev.count(values, offsets, thresholds, hits, with_counts ? &counts : nullptr);
        if (verify) {
            candidates.clear();
            for (size_t q = 0; q < names.size(); ++q)
                for (uint64_t u : set_bins(hits.data() + q * W, bins)) candidates.push_back({(uint32_t)q, (uint32_t)u});
            verifier->verify(seqs, candidates, confirmed, all_targets ? &targets : nullptr);
            for (size_t c = 0; c < candidates.size(); ++c) {
                const size_t q = candidates[c].query, u = candidates[c].bin;
                const auto write = [&](const BinVerifier::Hit& h) {
                    row.assign(names[q]).append("\t").append(image.bin_paths[u]);
                    if (with_counts) row.append("\t").append(std::to_string(counts[q * W * 64 + u])).append("/").append(std::to_string(n_of[q]));
                    row.append("\t").append(std::to_string(h.distance)).append("\t").append(*h.target).append("\t").append(std::to_string(h.end));
                    if (dna) row.append("\t").append(1, h.strand);
                    if (align) append_alignment(row, h);
                    out << row << '\n';
                };
                if (all_targets) {
                    for (const BinVerifier::Hit& h : targets[c]) write(h);
                    continue;
                }
                const BinVerifier::Hit& h = confirmed[c];
                if (h.distance == 0xFFFFFFFFu) continue;
                write(h);
            }
            seqs.clear();
        } else {
            for (size_t q = 0; q < names.size(); ++q) {
                for (uint64_t u : set_bins(hits.data() + q * W, bins)) {
                    row.assign(names[q]).append("\t").append(image.bin_paths[u]);
                    if (with_counts) row.append("\t").append(std::to_string(counts[q * W * 64 + u])).append("/").append(std::to_string(n_of[q]));
                    out << row << '\n';
                }
            }
        }
        names.clear();
        values.clear();
        offsets.assign(1, 0);
        n_of.clear();
        thresholds.clear();
    };
    std::vector<uint64_t> v;
    for_each_record(a.pos[1], [&](const FastaRecord& r) {
        v.clear();
        enc.record_values(r.seq, false, v);
        const uint64_t n = v.size();
        if (n == 0) {
            std::cerr << "[tetrex search] " << r.name << ": no k-mer of length " << enc.k() << ", skipped" << std::endl;
            return;
        }
        uint64_t t;
        if (a.has("threshold")) t = (uint64_t)std::ceil(fraction * (double)n);
        else t = n > (uint64_t)enc.k() * errors ? n - (uint64_t)enc.k() * errors : 0;
        if (t == 0) std::cerr << "[tetrex search] " << r.name << ": threshold 0, every bin is reported" << std::endl;
        if (values.size() + n > max_values || names.size() >= max_queries) flush();
        names.push_back(r.name);
        if (verify) seqs.push_back(r.seq);
        values.insert(values.end(), v.begin(), v.end());
        offsets.push_back(values.size());
        n_of.push_back(n);
        thresholds.push_back((uint32_t)std::min<uint64_t>(t, 0xFFFFFFFFull));
    });
    flush();
    out.flush();
    if (verbose && verify) std::cerr << "Verified: " << verifier->n_confirmed() << " of " << verifier->n_candidates() << " candidate pairs" << std::endl;
    if (verbose && all_targets) std::cerr << "Targets: " << verifier->n_targets() << std::endl;
    if (verify && std::getenv("TETREX_TRACE")) {
        const BinVerifier::Routed n = verifier->n_routed();
        std::cerr << "[tetrex search] verify routes: device " << n.device << ", device-long " << n.device_long << ", host " << n.host << std::endl;
        if (align) trace_align_routes(*verifier);
    }
    if (verbose) std::cerr << "Search time: " << (now() - t_start) << " s" << std::endl;
    return 0;
}

int cmd_inspect(int argc, char** argv) {
    if (argc != 3) { std::cerr << "[Error TetRex Index Inspection module expected <index>\n"; return 0; }
    std::cerr << "Reading Index from Disk... ";
    const double t1 = now();
    const IndexImage ix = read_index_file(argv[2]);
    std::cerr << "DONE in " << (now() - t1) << "s" << std::endl;
    const bool dna = ix.molecule == "na";
    if (ix.is_hibf) {
        std::cout << "INDEX TYPE: HIBF" << std::endl;
        std::cout << "FALSE POSITIVE RATE: " << std::fixed << std::setprecision(2) << ix.fpr << std::endl;
    } else {
        std::cout << "INDEX TYPE: IBF" << std::endl;
        std::cout << "BIN COUNT (BFs): " << ix.ibf.bins << std::endl;
        std::cout << "BIN SIZE (bits): " << ix.ibf.bin_size << std::endl;
    }
    std::cout << "HASH COUNT (hash functions): " << unsigned(ix.hash_count) << std::endl;
    std::cout << "KMER LENGTH (" << (dna ? "bases" : "residues") << "): " << unsigned(ix.k) << std::endl;
    std::cout << "MOLECULE TYPE (alphabet): " << (dna ? "Nucleic Acid" : "Amino Acid") << " [REDUCTION=";
    if (dna && ix.is_hibf) std::cout << "NONE";
    else std::cout << unsigned(ix.reduction);  // the reference streams the uint8_t itself
    std::cout << "]" << std::endl;
    std::cout << "ACID LIBRARY (filepaths):" << std::endl;
    for (const auto& p : ix.bin_paths) std::cout << "\t- " << p << std::endl;
    std::cerr << "DONE" << std::endl;
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    try {
        if (argc < 2) { std::cerr << "[Error] usage: tetrex {index|query|search|inspect} ...\n"; return -1; }
        const std::string sub = argv[1];
        if (sub == "query") return cmd_query(argc, argv);
        if (sub == "index") return cmd_index(argc, argv);
        if (sub == "search") return cmd_search(argc, argv);
        if (sub == "inspect") return cmd_inspect(argc, argv);
        if (sub == "track") return cmd_track(argc, argv);
        std::cerr << "[Error] unknown sub-command " << sub << "\n";
        return -1;
    } catch (const std::exception& e) {
        std::cerr << "[Error] " << e.what() << std::endl;
        return 1;
    }
}
