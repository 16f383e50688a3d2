// The address arithmetic of six-frame translation (txq_translate.hip): how the bytes of a batch are cut
// into units and steps, where the codon at a start position lands in each direction, and how a run of residue letters is
// split into stores that cover only its own bytes.  Plain functions, no HIP: tests/native/frames_plan_sim.cpp walks records
// with them on the CPU under sanitizers, the kernels call them and restate nothing.
#pragma once
#include "txq_text.hpp"

namespace txq {
namespace tr {

constexpr uint32_t kUnits = 8192;          // waves of a translation call
constexpr uint32_t kTile = 192;            // start positions per step: 64 lanes x 3 frames
constexpr uint64_t kMinChunk = 4 * kTile;  // start positions per unit, at least

// start positions per unit for `total` bytes: a multiple of kTile, so that at most kUnits units cover them
TXQ_TEXT_FN uint64_t chunk_len(uint64_t total) {
    const uint64_t c = (total + kUnits - 1) / kUnits;
    const uint64_t tiles = (c + kTile - 1) / kTile;
    return tiles * kTile < kMinChunk ? kMinChunk : tiles * kTile;
}

// T/U = 0, C = 1, A = 2, G = 3 in either case; anything else is ambiguous (4).  The complement is code ^ 2.
TXQ_TEXT_FN uint32_t nucleotide(uint8_t c) {
    switch (c & 0xDFu) {
        case 'T': case 'U': return 0u;
        case 'C': return 1u;
        case 'A': return 2u;
        case 'G': return 3u;
        default: return 4u;
    }
}

// ---- frames as letters (txq_translate_frames*) ------------------------------------------------------------------------
// Frame f = 0..5 of a record of L bytes has frame_len(L, f mod 3) residues.  The codon at start position p (p + 3 <= L) is
// residue p / 3 of frame p mod 3 and, reverse-complemented, residue (L - 3 - p) / 3 of frame 3 + (L - 3 - p) mod 3: each of
// the two maps is one to one between the start positions 0 .. L - 3 and the residues of its three frames (start_of is the
// way back), so whoever writes exactly the codons of its own start positions writes every residue exactly once.

TXQ_TEXT_FN uint64_t frame_len(uint64_t L, uint32_t o) { return L >= o ? (L - o) / 3 : 0; }
TXQ_TEXT_FN uint32_t fwd_frame(uint64_t p) { return (uint32_t)(p % 3); }
TXQ_TEXT_FN uint64_t fwd_index(uint64_t p) { return p / 3; }
TXQ_TEXT_FN uint32_t rev_frame(uint64_t L, uint64_t p) { return 3u + (uint32_t)((L - 3 - p) % 3); }
TXQ_TEXT_FN uint64_t rev_index(uint64_t L, uint64_t p) { return (L - 3 - p) / 3; }
TXQ_TEXT_FN uint64_t start_of(uint64_t L, uint32_t frame, uint64_t i) { return frame < 3 ? 3 * i + frame : L - 3 - (3 * i + (frame - 3)); }

// the start positions [lo, hi) of the record [rs, re) (L >= 3 bytes) that belong to the unit [ua, ub): lo >= hi, none
struct Owned {
    uint64_t lo, hi;
};
TXQ_TEXT_FN Owned owned_starts(uint64_t rs, uint64_t re, uint64_t ua, uint64_t ub) {
    const uint64_t L = re - rs, fit = L - 2, cut = (ub < re ? ub : re) - rs;
    return {(ua > rs ? ua : rs) - rs, cut < fit ? cut : fit};
}

// A step at t0 (a multiple of 3) takes the start positions [t0, t0 + kTile) that are the unit's.  Those with p mod 3 = j are
// consecutive residues of forward frame j in ascending p, and of one reverse frame in descending p: six runs a step, run
// c = 0, 1, 2 forward, c = 3 + j the same codons reverse-complemented.
constexpr uint32_t kRuns = 6;
TXQ_TEXT_FN uint32_t run_frame(uint64_t L, uint32_t c) { return c < 3 ? c : 3u + (uint32_t)((L - (c - 3)) % 3); }
struct Run {
    uint64_t first, count;  // residues [first, first + count) of frame run_frame(L, c); count <= kTile / 3
};
TXQ_TEXT_FN Run step_run(uint64_t L, uint64_t t0, Owned o, uint32_t c) {
    const uint32_t j = c < 3 ? c : c - 3;
    const uint64_t a = o.lo > t0 ? o.lo : t0, b = o.hi < t0 + kTile ? o.hi : t0 + kTile;
    if (a >= b) return {0, 0};
    const uint64_t pf = a + (j + 3 - (uint32_t)(a % 3)) % 3;  // the first and the last start position of the run
    if (pf >= b) return {0, 0};
    const uint64_t pl = pf + (b - 1 - pf) / 3 * 3;
    return {c < 3 ? fwd_index(pf) : rev_index(L, pl), (pl - pf) / 3 + 1};
}

// A run goes to the bytes [a0, a1) of the output (addresses; a1 - a0 <= 64, any alignment).  The units on either side write
// the bytes next to it, so a store may cover owned bytes only: the run is cut along the 16-byte blocks of the address space,
// at most kRunBlocks of them; a block that is the run's altogether is one 16-byte store, in a ragged block the aligned
// 4-byte words that are the run's altogether are 4-byte stores and what remains is byte stores.  Nothing is read back.
constexpr uint32_t kRunBlocks = 5;                   // 15 + 64 bytes at most from the first block's start
constexpr uint32_t kStageRow = 16 * kRunBlocks;      // a run staged at its address modulo 16
TXQ_TEXT_FN uintptr_t block_floor(uintptr_t a) { return a & ~(uintptr_t)15; }
// bit i: byte g + i of the block at g (a multiple of 16) is one of [a0, a1)
TXQ_TEXT_FN uint32_t block_mask(uintptr_t a0, uintptr_t a1, uintptr_t g) {
    const uint32_t lo = a0 > g ? (a0 - g < 16 ? (uint32_t)(a0 - g) : 16u) : 0u;
    const uint32_t hi = a1 > g ? (a1 - g < 16 ? (uint32_t)(a1 - g) : 16u) : 0u;
    return lo < hi ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
}
// sink.store16(address, src) / store4(address, src) / store1(address, byte); src: the block's 16 staged bytes
template <class Sink>
TXQ_TEXT_FN void store_block(uint32_t mask, uintptr_t g, const uint8_t* src, Sink& sink) {
    if (mask == 0xFFFFu) {
        sink.store16(g, src);
        return;
    }
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
        const uint32_t nib = (mask >> (4 * w)) & 15u;
        if (nib == 15u) {
            sink.store4(g + 4 * w, src + 4 * w);
            continue;
        }
#pragma unroll
        for (uint32_t b = 0; b < 4; ++b)
            if ((nib >> b) & 1u) sink.store1(g + 4 * w + b, src[4 * w + b]);
    }
}

// the letters of the codon (x, y, z) (nucleotide codes) in both directions; table: NCBI table 1 by 16 x + 4 y + z
TXQ_TEXT_FN void codon_letters(const char* table, uint32_t x, uint32_t y, uint32_t z, uint8_t* fwd, uint8_t* rev) {
    if ((x | y | z) & 4u) *fwd = *rev = (uint8_t)'X';
    else {
        *fwd = (uint8_t)table[16u * x + 4u * y + z];
        *rev = (uint8_t)table[16u * (z ^ 2u) + 4u * (y ^ 2u) + (x ^ 2u)];
    }
}

}  // namespace tr
}  // namespace txq
