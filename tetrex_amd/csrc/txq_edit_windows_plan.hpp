// The bundles of the windowed edit-distance kernel (txq_edit_windows.hip; include/txq.h txq_edit_windows_device; DESIGN.md
// §19): which pairs walk a group's text together, how far the bundle reaches and where its shared walk starts.  Plain
// functions, no HIP: the plan kernel and edit_windows_kernel call them, and tests/native/edit_windows_sim.cpp runs the same
// code on the CPU under sanitizers.
//
// A pair is (window, group, cap e).  Consecutive pairs of one group whose windows have the same word count are COMPATIBLE:
// one walk over the group's text can step all of their Myers states.  The pairs are cut into bundles from purely local
// information — pair i looks at itself and at pair i - 1 —, so the cut is deterministic and every pair is in exactly one
// bundle: pair i is a HEAD iff i % K == 0, or pair i - 1 is not compatible with it, or either of them was refused; a bundle is
// a head and the non-heads behind it, at most K pairs (K = bundle_size(words, cap): K words <= 8, so that the states stay in
// registers).  A head carries the units of its group's text, a non-head none: pair_of_unit (txq_text.hpp) steps over it.
#pragma once
#include "txq_text.hpp"

namespace txq {
namespace ew {

constexpr uint32_t kMaxBundle = 4;

// 64-bit words of a window of m letters, as the kernels are instantiated: 1, 2, 4 or 8
TXQ_TEXT_FN uint32_t words_of(uint32_t m) { return m <= 64 ? 1u : m <= 128 ? 2u : m <= 256 ? 4u : 8u; }

// pairs of one bundle at `words` words a state: K words <= 8, and at most `cap` (TXQ_EDIT_WINDOWS_BUNDLE: 1, 2 or 4)
TXQ_TEXT_FN uint32_t bundle_size(uint32_t words, uint32_t cap) {
    const uint32_t most = words >= 8 ? 1u : words == 4 ? 2u : kMaxBundle;
    return most < cap ? most : cap;
}

// what the cut needs to know of a pair; ok = false: refused (an index, an offset or a length outside what the call takes)
struct Member {
    bool ok;
    uint32_t group, words;
};

// is pair i the head of a bundle?  `prev` is pair i - 1 (anything where i = 0)
TXQ_TEXT_FN bool is_head(uint64_t i, const Member& prev, const Member& cur, uint32_t cap) {
    if (!cur.ok || i == 0) return true;
    if (i % bundle_size(cur.words, cap) == 0) return true;
    return !prev.ok || prev.group != cur.group || prev.words != cur.words;
}

// the pairs of the bundle whose head is pair h (an accepted one): h and the non-heads behind it, at most bundle_size of them
// (the pair behind a full bundle is a head by the first rule: it is not looked at).  member(i) gives pair i.
template <class MemberOf>
TXQ_TEXT_FN uint32_t bundle_extent(uint64_t h, uint64_t n_pairs, uint32_t cap, MemberOf&& member) {
    uint32_t n = 1;
    Member prev = member(h);
    const uint32_t most = bundle_size(prev.words, cap);
    while (n < most && h + n < n_pairs) {
        const Member cur = member(h + n);
        if (is_head(h + n, prev, cur, cap)) break;
        prev = cur;
        ++n;
    }
    return n;
}

// the bytes in front of its chunk that a lane walks for a window of m letters at cap e: an alignment of cost <= e that ends at
// j begins no earlier than j - m - e + 1, and no cost above m is ever the least
TXQ_TEXT_FN uint64_t lead_of(uint32_t m, uint32_t e) { return (uint64_t)m + (e < m ? e : m); }

// Where the walk of a lane whose chunk begins at ca starts, in a record that begins at rs, with `lead` the largest lead_of of
// the bundle.  A state that starts earlier than its own lead asks for is still exact: D[0][j] = 0 lets a match begin
// anywhere, so more text in front can only bring a score down to its true value, never below it.
TXQ_TEXT_FN uint64_t walk_start(uint64_t ca, uint64_t rs, uint64_t lead) { return ca - rs > lead ? ca - lead : rs; }

}  // namespace ew
}  // namespace txq
