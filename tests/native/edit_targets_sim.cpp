// Stand-alone check of csrc/txq_edit_targets_plan.hpp: the lane schedules of the two per-record edit-distance kernels
// (txq_edit_targets.hip) run on the CPU — the short kernel's lanes on their chunks, the long kernel's lane groups as arrays
// with the cross-lane move as a shift by one —, units, chunks and spans cut as the kernels cut them, the text read through
// load_block, slots, first keys, the flush rule and the rows taken from the plan header, against edit_targets_group of
// host/edit_distance.hpp.  Built with sanitizers by tests/test_edit_targets_sim.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/edit_targets_sim.cpp -o sim && ./sim
// Prints "edit_targets_sim ok: <cases> cases, <hits> hits" and exits 0, or names the first case that differs and exits 1.
#include "../../tetrex_amd/csrc/host/edit_distance.hpp"
#include "../../tetrex_amd/csrc/txq_edit_long_plan.hpp"
#include "../../tetrex_amd/csrc/txq_edit_targets_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

using namespace txq;

namespace {

struct Text {
    const uint8_t* bytes;
    uint64_t n;
    const uint64_t* rec;
};

struct Pair {
    uint32_t m, e;
    uint64_t r0, r1, gs, ge, base;  // base: the pair's first slot
};

// what atomicMin does to a slot, with the store checked against the slots' size
void lower(std::vector<uint64_t>& slots, uint64_t slot, uint64_t key) {
    if (slot == kNoSlot) return;
    if (slot >= slots.size()) std::printf("edit_targets_sim: slot %llu of %zu\n", (unsigned long long)slot, slots.size()), std::exit(1);
    slots[slot] = std::min(slots[slot], key);
}

// one lane of targets_kernel<W> on its chunk [ca, cb)
void run_lane(const Text& t, const uint64_t* peq, const uint8_t* codes, uint32_t W, const Pair& v, uint64_t ca, uint64_t cb, std::vector<uint64_t>& slots) {
    if (ca >= v.ge) return;
    const uintptr_t text_lo = (uintptr_t)t.bytes, text_hi = text_lo + t.n;
    const uint32_t m = v.m, e = v.e, hw = (m - 1) >> 6, hs = (m - 1) & 63;
    const uint64_t lead = (uint64_t)m + (e < m ? e : m);
    uint64_t best = kNoKey;
    uint64_t r = record_of(t.rec, v.r0, v.r1, ca);
    uint64_t rs = t.rec[r], re = t.rec[r + 1];
    if (rs < v.gs || rs > ca) rs = ca;
    const uint64_t start = ca - rs > lead ? ca - lead : rs;
    std::vector<uint64_t> pv(W, ~0ULL), mv(W, 0);
    uint32_t score = m;
    const uintptr_t first = (text_lo + start) & ~(uintptr_t)15, last = text_lo + cb;
    for (uintptr_t blk = first; blk < last; blk += 16) {
        const TextBlock raw = load_block(blk, text_lo, text_hi, 0);
        for (uint32_t i = 0; i < 16; ++i) {
            const uint64_t at = raw.t0 + i;
            if (at < start || at >= cb) continue;
            if (at >= re) {
                lower(slots, targets_flush(best, v.base, r, v.r0, v.r1), best);
                best = kNoKey;
                re = long_next_record(t.rec, r, v.r1, v.ge, at);  // (the loop the kernel spells out)
                std::fill(pv.begin(), pv.end(), ~0ULL);
                std::fill(mv.begin(), mv.end(), 0);
                score = m;
            }
            const uint32_t cls = codes[(raw.w[i >> 2] >> (8 * (i & 3))) & 255u];
            uint64_t carry = 0, ph_in = 0, mh_in = 0;
            for (uint32_t w = 0; w < W; ++w) {
                const uint64_t eq = peq[cls * W + w], p = pv[w], n = mv[w];
                const uint64_t xv = eq | n, x = eq & p;
                const uint64_t s1 = x + p, s2 = s1 + carry;
                carry = (uint64_t)(s1 < x) | (uint64_t)(s2 < s1);
                const uint64_t xh = (s2 ^ p) | eq;
                uint64_t ph = n | ~(xh | p), mh = p & xh;
                if (w == hw) score += (uint32_t)((ph >> hs) & 1) - (uint32_t)((mh >> hs) & 1);
                const uint64_t ph_out = ph >> 63, mh_out = mh >> 63;
                ph = (ph << 1) | ph_in;
                mh = (mh << 1) | mh_in;
                ph_in = ph_out, mh_in = mh_out;
                pv[w] = mh | ~(xv | ph);
                mv[w] = ph & xv;
            }
            if (at >= ca && score <= e) best = std::min(best, edit_key(score, at, v.gs, r, v.r0));
        }
    }
    lower(slots, targets_flush(best, v.base, r, v.r0, v.r1), best);
}

// one group of G lanes of targets_long_kernel<G> on its span [ca, cb)
void run_span(const Text& t, const uint64_t* peq, const uint8_t* codes, uint32_t G, const Pair& v, uint64_t ca, uint64_t cb, std::vector<uint64_t>& slots) {
    if (ca >= v.ge) return;
    const uintptr_t text_lo = (uintptr_t)t.bytes, text_hi = text_lo + t.n;
    const uint32_t m = v.m, e = v.e, hw = (m - 1) >> 6;
    uint64_t rf = record_of(t.rec, v.r0, v.r1, ca), rf_end = t.rec[rf + 1];
    const uint64_t start = long_start(ca, t.rec[rf], v.gs, m, e);
    const uintptr_t base = (text_lo + start) & ~(uintptr_t)15;
    const uint64_t t0 = (uint64_t)(base - text_lo), columns = (uint64_t)(text_lo + cb - base), steps = long_steps(columns, m);
    std::vector<uint64_t> pv(G, ~0ULL), mv(G, 0);
    std::vector<uint32_t> out(G, 0), in(G, 0);
    uint64_t rs = rf, best = kNoKey;
    uint32_t score = m;
    for (uint64_t s0 = 0; s0 < steps; s0 += 16) {
        TextBlock raw{};
        if (s0 < columns) raw = load_block(base + s0, text_lo, text_hi, 0);
        for (uint32_t i = 0; i < 16; ++i) {
            const uint64_t s = s0 + i;
            for (uint32_t w = G - 1; w > 0; --w) in[w] = out[w - 1];  // the cross-lane move
            in[0] = 0;
            const uint64_t at0 = t0 + s;
            if (s < columns && at0 >= start && at0 < cb) {
                const bool reset = at0 >= rf_end;
                if (reset) rf_end = long_next_record(t.rec, rf, v.r1, v.ge, at0);
                in[0] = long_feed(codes[(raw.w[i >> 2] >> (8 * (i & 3))) & 255u], reset);
            }
            for (uint32_t w = 0; w < G; ++w) {
                const uint32_t bit = w == hw ? (m - 1) & 63 : 63u;
                out[w] = long_block_step(pv[w], mv[w], peq[(in[w] & kMsgClass) * G + w], in[w], bit);
                if (w == hw && (out[w] & kMsgValid)) {
                    const uint64_t at = t0 + s - hw;
                    if (out[w] & kMsgReset) {
                        lower(slots, targets_flush(best, v.base, rs, v.r0, v.r1), best);
                        best = kNoKey;
                        score = m;
                        (void)long_next_record(t.rec, rs, v.r1, v.ge, at);
                    }
                    score += (uint32_t)long_hin(out[w]);
                    if (at >= ca && score <= e) best = std::min(best, edit_key(score, at, v.gs, rs, v.r0));
                }
            }
        }
    }
    lower(slots, targets_flush(best, v.base, rs, v.r0, v.r1), best);
}

// A call of two pairs (groups [r0, R) and [0, R) of one pattern, cap e) with n_slots slots: plan, first keys, the kernels'
// walks, the compaction.  long_form: targets_long_kernel's mapping, else targets_kernel's.
std::vector<uint32_t> run_call(const Text& t, const std::vector<uint8_t>& p, const uint8_t* codes, uint64_t r0, uint64_t R, uint32_t e, uint32_t cut,
                               bool long_form, uint64_t n_slots, std::vector<uint32_t>& status) {
    const uint32_t m = (uint32_t)p.size();
    const uint32_t lanes_w = long_form ? long_group_lanes(m) : (m <= 64 ? 1u : m <= 128 ? 2u : m <= 256 ? 4u : 8u);  // G, or W
    uint8_t cls[256];
    for (unsigned b = 0; b < 256; ++b) cls[b] = codes[b] < 31 ? codes[b] : (uint8_t)31;
    std::vector<uint64_t> peq(32 * lanes_w, 0);
    for (uint32_t i = 0; i < m; ++i)
        if (cls[p[i]] < 31) peq[cls[p[i]] * lanes_w + (i >> 6)] |= 1ULL << (i & 63);
    const uint64_t firsts[2] = {r0, 0};
    std::vector<uint64_t> spref{0};
    for (uint64_t f : firsts) spref.push_back(spref.back() + targets_slots_of(true, f, R));
    std::vector<uint64_t> slots(n_slots, 0x5555555555555555ULL);  // (what the init does not write is never read)
    const uint64_t used = targets_used(spref.data(), 2, n_slots);
    status.assign(2, 0);
    std::vector<Pair> pairs;
    for (uint64_t i = 0; i < 2; ++i) {
        pairs.push_back({m, e, firsts[i], R, t.rec[firsts[i]], t.rec[R], spref[i]});
        if (!targets_fits(spref.data(), i, n_slots)) status[i] = kTargetsRefused;
    }
    for (uint64_t s = 0; s < used; ++s) {
        const uint64_t pair = pair_of_unit(spref.data(), 2, s);
        const Pair& v = pairs[pair];
        slots[s] = targets_fits(spref.data(), pair, n_slots) ? targets_initial_key(m, e, t.rec, v.r0 + (s - spref[pair]), v.r0, v.gs) : kNoKey;
    }
    for (uint64_t i = 0; i < 2; ++i) {
        const Pair& v = pairs[i];
        if (!targets_fits(spref.data(), i, n_slots)) continue;
        const uint32_t lanes = long_form ? long_groups(lanes_w) : 64;
        const uint64_t units = units_of(v.ge - v.gs, lanes, cut);
        for (uint64_t slice = 0; slice < units; ++slice)
            for (uint32_t lane = 0; lane < lanes; ++lane) {
                const ChunkBounds c = chunk_bounds(v.gs, v.ge, slice, lanes, lane, cut);
                if (long_form) run_span(t, peq.data(), cls, lanes_w, v, c.ca, c.cb, slots);
                else run_lane(t, peq.data(), cls, lanes_w, v, c.ca, c.cb, slots);
            }
    }
    std::vector<uint32_t> rows;
    for (uint64_t b = 0; b < targets_blocks(n_slots); ++b)
        for (uint64_t s = b * kTargetsBlock; s < std::min<uint64_t>((b + 1) * kTargetsBlock, used); ++s)
            if (slots[s] != kNoKey) {
                const uint64_t pair = pair_of_unit(spref.data(), 2, s);
                rows.resize(rows.size() + 4);
                targets_row(rows.data() + rows.size() - 4, pair, slots[s], t.rec, pairs[pair].r0, pairs[pair].r1, pairs[pair].gs);
            }
    return rows;
}

}  // namespace

int main() {
    std::mt19937_64 rng(20250607);
    size_t cases = 0, hits = 0;
    const uint32_t lengths[] = {1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1025, 2049, 4096};
    for (unsigned letters : {4u, 20u}) {
        uint8_t codes[256];
        for (unsigned b = 0; b < 256; ++b) codes[b] = 255;
        for (unsigned l = 0; l < letters; ++l) codes['A' + l] = codes['a' + l] = (uint8_t)l;
        const auto letter = [&]() -> uint8_t {
            if (rng() % 25 == 0) return rng() % 2 ? (uint8_t)'#' : (uint8_t)(rng() % 256);  // mostly no class
            return (uint8_t)((rng() % 2 ? 'A' : 'a') + rng() % letters);
        };
        for (uint32_t m : lengths) {
            std::vector<uint8_t> p(m);
            for (uint8_t& c : p) c = letter();
            const auto edited = [&](unsigned edits) {
                std::vector<uint8_t> copy = p;
                for (; edits > 0 && !copy.empty(); --edits) {
                    const size_t at = (size_t)(rng() % copy.size());
                    switch (rng() % 3) {
                        case 0: copy[at] = letter(); break;
                        case 1: copy.insert(copy.begin() + (long)at, letter()); break;
                        default: copy.erase(copy.begin() + (long)at); break;
                    }
                }
                return copy;
            };
            // records: empty ones at the front, between and at the end; one byte; m - 1 bytes; three with edited copies, one
            // of them twice; a run of tiny records (many flushes inside one chunk)
            std::vector<uint8_t> text;
            std::vector<uint64_t> rec{0};
            const auto add = [&](const std::vector<uint8_t>& body, size_t before, size_t behind) {
                for (size_t i = 0; i < before; ++i) text.push_back(letter());
                text.insert(text.end(), body.begin(), body.end());
                for (size_t i = 0; i < behind; ++i) text.push_back(letter());
                rec.push_back(text.size());
            };
            add({}, 0, 0);
            add({}, 1, 0);
            add(edited(3), rng() % 40, rng() % 40);
            add({}, 0, 0);
            add({}, 0, 0);
            add({}, m - 1, 0);
            add(edited(2), rng() % 40, rng() % 40);
            for (unsigned k = 0; k < 12; ++k) add({}, k % 4, 0);
            add(p, rng() % 70, 0);
            {
                std::vector<uint8_t> twice = edited(1);
                for (unsigned k = 0; k < 30; ++k) twice.push_back(letter());
                twice.insert(twice.end(), p.begin(), p.end());
                add(twice, 3, 2);
            }
            add({}, 0, 0);
            const uint64_t n = text.size(), R = rec.size() - 1;
            for (unsigned shift : {0u, 3u}) {
                uint8_t* heap = (uint8_t*)std::aligned_alloc(16, (size_t)((n + shift + 15) / 16 * 16));
                std::memcpy(heap + shift, text.data(), (size_t)n);
                const Text t{heap + shift, n, rec.data()};
                tetrex::EditPattern ep(p.data(), m, codes);
                const uint32_t big = (uint32_t)((n + 16) / 16 * 16);
                const bool large = m > 600;   // (a short span then walks a lead-in of up to 2 m bytes for its few own ones)
                for (int long_form = m <= 512 ? 0 : 1; long_form < 2; ++long_form)
                    for (uint32_t cut : {16u, 64u, big}) {
                        if (shift && cut != 64) continue;
                        for (uint32_t cap : {0u, 3u, m - 1, m, m + 5}) {
                            if (large && cut == 16 && (cap != 3 || m != 2049 || letters != 4)) continue;
                            if (large && cut == 64 && (shift ? cap != m - 1 || m == 4096 : cap != 3 && (cap != m || m == 4096))) continue;
                            if (large && cut == big && cap != 3 && cap != m + 5) continue;
                            if (long_form && m <= 512 && (cut == big || cap == m - 1)) continue;  // (short patterns on the long mapping: fewer)
                            for (uint64_t r0 : {(uint64_t)3, R}) {
                                if (r0 == R && (cut != 64 || shift)) continue;
                                const uint64_t need = (R - r0) + R;
                                for (uint64_t n_slots : {need, need - 1, need + 300}) {
                                    if (n_slots != need && (cut != 64 || cap != 3 || large)) continue;
                                    std::vector<uint32_t> want, status;
                                    if (R - r0 <= n_slots) tetrex::edit_targets_group(ep, t.bytes, t.rec, r0, R, cap, 0, want);
                                    if (need <= n_slots) tetrex::edit_targets_group(ep, t.bytes, t.rec, 0, R, cap, 1, want);
                                    const std::vector<uint32_t> got = run_call(t, p, codes, r0, R, cap, cut, long_form != 0, n_slots, status);
                                    ++cases;
                                    hits += got.size() / 4;
                                    const bool status_ok = status[0] == (R - r0 <= n_slots ? 0u : kTargetsRefused) && status[1] == (need <= n_slots ? 0u : kTargetsRefused);
                                    if (got != want || !status_ok) {
                                        size_t at = 0;
                                        while (at < got.size() && at < want.size() && got[at] == want[at]) ++at;
                                        at = at / 4 * 4;
                                        std::printf("edit_targets_sim: %u letters, m = %u, %s mapping, cut %u, cap %u, records %llu..%llu, %llu slots, text at +%u: "
                                                    "%zu rows, the host %zu; status %u %u; first difference at row %zu",
                                                    letters, m, long_form ? "long" : "short", cut, cap, (unsigned long long)r0, (unsigned long long)R,
                                                    (unsigned long long)n_slots, shift, got.size() / 4, want.size() / 4, status[0], status[1], at / 4);
                                        if (at + 4 <= got.size()) std::printf(": (%u, %u, %u, %u)", got[at], got[at + 1], got[at + 2], got[at + 3]);
                                        if (at + 4 <= want.size()) std::printf(", the host (%u, %u, %u, %u)", want[at], want[at + 1], want[at + 2], want[at + 3]);
                                        std::printf("\n");
                                        return 1;
                                    }
                                }
                            }
                        }
                    }
                std::free(heap);
            }
        }
    }
    std::printf("edit_targets_sim ok: %zu cases, %zu hits\n", cases, hits);
    return 0;
}
