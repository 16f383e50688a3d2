// The windows of a translated frame (txq_translate_windows*, txq_translate.hip; `tetrex search --translate --frame-window`,
// DESIGN.md §18): how many windows a frame of R residues has, where window j lies, which window slots the k-mer position
// ("codon") c serves as a begin or as an end, and where a run of residues lies on the record in nucleotides.  Plain
// functions, no HIP: tests/native/frame_windows_sim.cpp walks records with them on the CPU under sanitizers, the kernel and the
// host call them and restate nothing.
//
// A frame of R residues has M = R - k + 1 k-mer positions 0 .. M - 1 (none where R < k).  Its windows, W residues long and S
// apart (k <= W, 1 <= S <= W), are those of a record of R letters under `tetrex search --window`:
//   R < k           none
//   R <= W          one, [0, R)
//   otherwise       [j S, j S + W) for j = 0, 1, ... while j S + W <= R (the regular windows), and one more, [R - W, R), where
//                   the last of these ends before R (the tail window).
// Window [a, a + l) owns the k-mer positions [a, a + l - k + 1): its begin boundary is a, its end boundary a + l - k + 1.  The
// stop-free k-mers of a frame are compacted in order, so with V(c) = the number of stop-free k-mers at positions below c the
// window owns the frame's values [V(a), V(a + l - k + 1)).  V(M) is the frame's value count; M is the end boundary of the
// frame's last window and of no other, and no k-mer position equals it.
#pragma once
#include "txq_frames_plan.hpp"

namespace txq {
namespace fw {

constexpr uint64_t kNone = ~(uint64_t)0;

struct Frame {
    uint64_t R;        // residues
    uint64_t M;        // k-mer positions (0: no window)
    uint64_t regular;  // windows at 0, S, 2 S, ... (the one window of a frame with R <= W counts as regular)
    uint64_t count;    // regular, + 1 with a tail window
    uint64_t tail_at;  // the tail window's begin, R - W (kNone: no tail window)
    uint32_t D, S, W;  // D = W - k + 1: k-mer positions from a full window's begin boundary to its end boundary
};

// (c / s, c mod s), in 32 bits where c fits them: the kernel asks this of every lane
struct DivMod {
    uint64_t q, r;
};
TXQ_TEXT_FN DivMod div_mod(uint64_t c, uint32_t s) {
    if ((c >> 32) == 0) return {(uint32_t)c / s, (uint32_t)c % s};
    return {c / s, c % s};
}

TXQ_TEXT_FN Frame frame_plan(uint64_t R, uint32_t k, uint32_t W, uint32_t S) {
    Frame f{R, 0, 0, 0, kNone, W - k + 1, S, W};
    if (R < k) return f;
    f.M = R - k + 1;
    if (R <= W) {
        f.regular = f.count = 1;
        return f;
    }
    f.regular = (R - W) / S + 1;
    f.count = f.regular;
    if ((f.regular - 1) * S + W < R) {
        f.tail_at = R - W;
        ++f.count;
    }
    return f;
}
TXQ_TEXT_FN uint64_t window_count(uint64_t R, uint32_t k, uint32_t W, uint32_t S) { return frame_plan(R, k, W, S).count; }

// window j < count of the frame: residues [a, a + len)
struct Window {
    uint64_t a, len;
};
TXQ_TEXT_FN Window window_at(const Frame& f, uint64_t j) {
    if (f.R <= f.W) return {0, f.R};
    if (j < f.regular) return {j * f.S, f.W};
    return {f.tail_at, f.W};
}

// The window slots of the frame that k-mer position c < M serves: `begin` the window whose begin boundary is c, `end` the
// window whose end boundary is c (kNone: none).  Every begin slot of the frame has exactly one c; so has every end slot but
// that of the frame's last window, whose end boundary is M: its value is the frame's value count, and whoever knows that
// writes it.  A regular and a tail window never begin at the same c (the tail begins strictly between two regular begins).
struct Slots {
    uint64_t begin, end;
};
TXQ_TEXT_FN Slots codon_slots(const Frame& f, uint64_t c) {
    Slots s{kNone, kNone};
    if (c == f.tail_at) s.begin = f.regular;
    else {
        const DivMod b = div_mod(c, f.S);
        if (b.r == 0 && b.q < f.regular) s.begin = b.q;
    }
    if (c >= f.D) {  // (a frame with R <= W has M <= D: never)
        const DivMod e = div_mod(c - f.D, f.S);
        if (e.r == 0 && e.q < f.regular) s.end = e.q;
    }
    return s;
}

// the k-mer positions of the start position p of a record of L bytes (p + 3 k <= L): position p / 3 of forward frame p mod 3,
// and, reverse-complemented, position (L - p - 3 k) / 3 of frame 3 + (L - p - 3 k) mod 3
TXQ_TEXT_FN uint64_t rev_kmer_index(uint64_t L, uint64_t p, uint32_t k) { return (L - p - 3ull * k) / 3; }
TXQ_TEXT_FN uint32_t rev_kmer_frame(uint64_t L, uint64_t p, uint32_t k) { return 3u + (uint32_t)((L - p - 3ull * k) % 3); }

// The residues [ra, rb) of frame f = 0..5 of a record of L bytes, as 1-based inclusive nucleotide positions on the record as
// given (begin <= end; the strand is the frame's): cutting those letters out, reverse-complementing them on a reverse frame
// and translating in frame +1 gives exactly these residues.
struct Span {
    uint64_t begin, end;
};
TXQ_TEXT_FN Span residues_on_record(uint64_t L, uint32_t f, uint64_t ra, uint64_t rb) {
    const uint64_t o = f % 3;
    if (f < 3) return {o + 3 * ra + 1, o + 3 * rb};
    return {L - o - 3 * rb + 1, L - o - 3 * ra};
}

}  // namespace fw
}  // namespace txq
