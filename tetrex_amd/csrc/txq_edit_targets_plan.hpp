// The slot arithmetic and the flush rule of the per-record edit-distance kernels (txq_edit_targets.hip), where
// a CPU can run them.  Plain functions, no HIP: the kernels call them and do not restate them, and
// tests/native/edit_targets_sim.cpp runs the lane schedules of both kernels on the CPU under sanitizers with the same functions.
//
// txq_edit_search* keeps one 64-bit key per pair, the least over the group.  Here every (pair, record of its group) has a key
// of its own, a slot: the slots of pair i are slots[spref[i] .. spref[i + 1]), spref the prefix of the pairs' record counts,
// slot spref[i] + (r - r0) being record r of a group that begins with record r0.  The key format is that of
// txq_edit_common.hpp — distance << 48 | position in the GROUP — so the least key over a pair's slots is the key the search
// kernels keep, and edit_answer turns a slot's key into (d, r, j) unchanged.
#pragma once
#include "txq_edit_common.hpp"

namespace txq {

constexpr uint32_t kTargetsRefused = 0xFFFFFFFEu;  // d_status of a pair that was not answered
constexpr uint32_t kTargetsBlock = 256;            // slots per block of the compaction
constexpr uint64_t kNoSlot = ~0ULL;

// slots a pair needs: the records of its group (a pair that failed its checks needs none)
TXQ_TEXT_FN uint64_t targets_slots_of(bool ok, uint64_t r0, uint64_t r1) { return ok ? r1 - r0 : 0; }

// pair i is answered only where its slots end inside the caller's n_slots (spref: the inclusive scan, spref[0] = 0)
TXQ_TEXT_FN bool targets_fits(const uint64_t* spref, uint64_t i, uint64_t n_slots) { return spref[i + 1] <= n_slots; }

// the slots in use: those of the pairs, or the caller's n_slots where they are fewer
TXQ_TEXT_FN uint64_t targets_used(const uint64_t* spref, uint64_t n_pairs, uint64_t n_slots) {
    return spref[n_pairs] < n_slots ? spref[n_pairs] : n_slots;
}

// the slot of record r of a pair whose slots begin at `base` and whose group is records [r0, r1); kNoSlot for a record outside
// the group, so that no offset table, whatever it holds, takes a store outside the pair's slots
TXQ_TEXT_FN uint64_t targets_slot(uint64_t base, uint64_t r, uint64_t r0, uint64_t r1) { return r >= r0 && r < r1 ? base + (r - r0) : kNoSlot; }

// what a slot holds before the kernels run: end 0 of its record, the empty match of distance m, where the cap allows it
TXQ_TEXT_FN uint64_t targets_initial_key(uint32_t m, uint32_t e, const uint64_t* rec, uint64_t r, uint64_t r0, uint64_t gs) {
    return m <= e ? (uint64_t)m << kPosBits | (rec[r] - gs + (r - r0)) : kNoKey;
}

// The flush rule.  A lane (txq_edit.hip's mapping) or the scoring lane of a lane group (txq_edit_long.hip's) keeps `best`, the
// least key it has seen in its CURRENT record.  Where its walk leaves the record — the branch that resets the recurrence — and
// once behind its last byte, it flushes: where best is a key, the key goes into the record's slot by a 64-bit minimum (an
// atomicMin on the device: several lanes and units may hold bytes of one record) and best starts again.  A lane that saw no
// score within the cap stores nothing.  Returns the slot to lower, or kNoSlot.
TXQ_TEXT_FN uint64_t targets_flush(uint64_t best, uint64_t base, uint64_t r, uint64_t r0, uint64_t r1) {
    return best != kNoKey ? targets_slot(base, r, r0, r1) : kNoSlot;
}

// ---- compaction: the slots that hold a key, in slot order, as (pair, d, r, j) ---------------------------------------------
TXQ_TEXT_FN uint64_t targets_blocks(uint64_t n_slots) { return (n_slots + kTargetsBlock - 1) / kTargetsBlock; }

// the row of slot s: the hit of record r0 + (s - base) of the pair that owns s
TXQ_TEXT_FN void targets_row(uint32_t* row, uint64_t pair, uint64_t key, const uint64_t* rec, uint64_t r0, uint64_t r1, uint64_t gs) {
    const EditAnswer a = edit_answer(key, rec, r0, r1, gs);
    row[0] = (uint32_t)pair, row[1] = a.d, row[2] = a.r, row[3] = a.j;
}

}  // namespace txq
