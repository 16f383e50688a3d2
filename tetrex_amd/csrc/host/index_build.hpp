// Host side: `tetrex index` and `tetrex track` — FASTA files to an index image, the bits set on the GPU through the C-ABI
// (include/txq.h).  Product code; requires a gfx950 GPU.
#pragma once
#include "index_file.hpp"

#include <string>
#include <vector>

namespace tetrex {

struct BuildOptions {
    unsigned k = 6;
    float fpr = 0.05f;
    unsigned hash_count = 3;
    bool dna = false;
    bool hibf = true;       // the reference's default flavour
    unsigned reduction = 0; // 0 None, 1 murphy, 2 li
    bool dna_wraparound = true;  // reproduce include/nucleotide_decomposer.h:106-110
    int device = 0;
    // HIBF layout: kUniform, this project's two-level tree (the default); kSized, host/layout.hpp with t_max = tmax
    // (0: default_tmax(B)), built by the kernels of txq_build.hip
    enum Layout { kUniform = 0, kSized = 1 };
    int layout = kUniform;
    uint64_t tmax = 0;
    // kSized only: before the layout, chain similar bins inside intervals of the sorted order (host/layout.hpp
    // rearrange_intervals / rearrange_chain, txq_pair_unions_device).  0: off; else the interval ratio in (0, 1].
    double rearrange_ratio = 0;
};
// `tetrex index`: FASTA files -> index image, bits set on the GPU (txq_emplace_device).
IndexImage build_index(const std::vector<std::string>& bin_files, const BuildOptions& opt, size_t* n_sequences = nullptr);
// `tetrex track`: FASTA files -> d-gram index (reference src/dGramIndex.cpp:22-38, include/dGramIndex.h:105-157)
DgramImage build_dgram_index(const std::vector<std::string>& bin_files, uint64_t min_gap, uint64_t max_gap, unsigned hash_count,
                             float fpr, int device = 0);

}  // namespace tetrex
