// The windows of a translated frame (txq_translate_windows*, txq_translate.hip; `tetrex search --translate --frame-window`,
// DESIGN.md §18): how many windows a frame of R residues has, where window j lies, which window slots the k-mer position
// ("codon") c serves as a begin or as an end, and where a run of residues lies on the record in nucleotides.  Plain
// functions, no HIP: tests/native/frame_windows_sim.cpp walks records with them on the CPU under sanitizers, the kernel and the
// host call them and restate nothing.  The last part says where a window's letters lie in the frames buffer, counts its stops
// and gives its threshold (txq_frame_window_letters*, txq_frame_letters.hip); tests/native/frame_window_letters_sim.cpp
// walks that part.
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

// ---- the letters of a window (txq_frame_window_letters*) ---------------------------------------------------
// Window j of a batch is window j - win_offsets[q] of frame q, the last q with win_offsets[q] <= j (window_finish_kernel's
// search); its residues [a, a + l) are the letters [frame_offsets[q] + a, + l) of the frames buffer.  Its stops are counted in
// the 16-byte blocks of the address space that hold those letters: a block is loaded whole where it lies inside the buffer,
// byte by byte where the buffer begins or ends in it (load_block), so no byte at or behind the buffer's end is read whatever
// the arrays say, and the bytes of a block that are not the window's — its head and its tail — are masked out of the compare.

// the frame of window j < win_offsets[m] (m >= 1 frames)
TXQ_TEXT_FN uint64_t frame_of_window(const uint64_t* win_offsets, uint64_t m, uint64_t j) {
    uint64_t lo = 0, hi = m;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (win_offsets[mid] <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

// how many of the four bytes of x that `nib` selects (bit i: byte i) equal `letter`
TXQ_TEXT_FN uint32_t equal_bytes(uint32_t x, uint32_t nib, uint8_t letter) {
    const uint32_t d = x ^ (letter * 0x01010101u);
    const uint32_t zero = ~(((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d | 0x7F7F7F7Fu);  // 0x80 in every byte of d that is 0, exactly
    const uint32_t sel = ((nib * 0x00204081u) & 0x01010101u) << 7;                 // bit i of nib to bit 8 i + 7
    return (uint32_t)__builtin_popcount(zero & sel);
}

// The stops among the letters at the addresses [a0, a1) of a buffer at [lo, hi) (a1 <= hi is the caller's to see to: what lies
// outside the buffer is not read and counts as no stop).  load(blk, lo, hi) gives the block's 16 bytes as load_block does.
template <class Load>
TXQ_TEXT_FN uint32_t count_stops(uintptr_t lo, uintptr_t hi, uintptr_t a0, uintptr_t a1, Load&& load) {
    uint32_t stops = 0;
    if (a1 > hi) a1 = hi;
    if (a0 < lo) a0 = lo;
    if (a0 >= a1) return 0;
    for (uintptr_t blk = tr::block_floor(a0); blk < a1; blk += 16) {
        const uint32_t mask = tr::block_mask(a0, a1, blk);  // head and tail: the block's bytes that are the window's
        const text4 w = load(blk, lo, hi);
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) stops += equal_bytes(w[i], (mask >> (4 * i)) & 15u, (uint8_t)'*');
    }
    return stops;
}

constexpr uint32_t kNotSearched = 0xFFFFFFFFu;
// `tetrex search --verify-frame-windows`: a window of w stop-free k-mers and s stops under E edits.  Each stop costs an edit of
// its own, so s > E is out of reach; the E - s edits that remain touch at most k of the w k-mers each.
TXQ_TEXT_FN uint32_t stop_threshold(uint32_t w, uint32_t s, uint32_t k, uint32_t edits) {
    if (s > edits) return kNotSearched;
    const uint64_t lost = (uint64_t)k * (edits - s);
    return (uint64_t)w > lost ? (uint32_t)(w - lost) : kNotSearched;
}

// window j of a batch: its letters [begin, begin + len) in the frames buffer (len 0: the arrays disagree, there is no such window)
struct Letters {
    uint64_t begin;
    uint32_t len;
};
TXQ_TEXT_FN Letters window_letters(const uint64_t* rec, const uint64_t* frame_offsets, const uint64_t* win_offsets, uint64_t m, uint64_t j, uint32_t k,
                                   uint32_t W, uint32_t S) {
    if (m == 0 || j >= win_offsets[m]) return {0, 0};
    const uint64_t q = frame_of_window(win_offsets, m, j), r = q / 6;
    const uint64_t rs = rec[r], re = rec[r + 1];
    const Frame f = frame_plan(tr::frame_len(re >= rs ? re - rs : 0, (uint32_t)(q % 3)), k, W, S);  // (q mod 3 = (q mod 6) mod 3)
    if (j - win_offsets[q] >= f.count) return {0, 0};
    const Window at = window_at(f, j - win_offsets[q]);
    return {frame_offsets[q] + at.a, (uint32_t)at.len};
}
// are the letters there to be read?  A window that is none, or whose letters leave the buffer, is not searched
TXQ_TEXT_FN bool letters_inside(const Letters& at, uint64_t frames_bytes) { return at.len > 0 && at.begin <= frames_bytes && at.len <= frames_bytes - at.begin; }

}  // namespace fw
}  // namespace txq
