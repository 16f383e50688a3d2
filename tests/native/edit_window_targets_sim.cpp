// Stand-alone check of csrc/txq_edit_window_targets_plan.hpp: a call of txq_edit_window_targets.hip run on the CPU — the plan
// kernel's view of every pair with its checks, units and slots, the two prefixes, the first keys, wt_walk_kernel's lanes on their
// chunks with the view's bounds handed to load_block, the flushes, the compaction and the rows, all taken from the plan headers
// — against edit_targets_group of host/edit_distance.hpp on the window written out.  Letters, texts, offsets, slots and rows
// live in allocations of their exact size, so a load or store that leaves one stops the program.  Built with sanitizers by
// tests/test_edit_window_targets_sim.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/edit_window_targets_sim.cpp -o sim && ./sim
// Prints "edit_window_targets_sim ok: <cases> cases, <hits> hits" and exits 0, or names the first case that differs and exits 1.
#include "../../tetrex_amd/csrc/host/edit_distance.hpp"
#include "../../tetrex_amd/csrc/txq_edit_long_plan.hpp"
#include "../../tetrex_amd/csrc/txq_edit_window_targets_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

using namespace txq;

namespace {

// what atomicMin does to a slot, with the store checked against the slots' size
void lower(std::vector<uint64_t>& slots, uint64_t slot, uint64_t key) {
    if (slot == kNoSlot) return;
    if (slot >= slots.size()) std::printf("edit_window_targets_sim: slot %llu of %zu\n", (unsigned long long)slot, slots.size()), std::exit(1);
    slots[slot] = std::min(slots[slot], key);
}

// one lane of wt_walk_kernel<W> on its chunk [ca, cb) of pair v, whose slots begin at `base`
void run_lane(const wt::Pair& v, const uint64_t* peq, const uint8_t* codes, uint32_t W, uint64_t base, uint64_t ca, uint64_t cb, std::vector<uint64_t>& slots) {
    if (ca >= v.ge) return;
    const uint64_t* const rec = v.v.rec;
    const uintptr_t text_lo = (uintptr_t)v.v.text, text_hi = text_lo + v.v.text_bytes;
    const uint32_t m = v.m, e = v.e, hw = (m - 1) >> 6, hs = (m - 1) & 63;
    uint64_t best = kNoKey;
    uint64_t r = record_of(rec, 0, v.r1, ca);
    uint64_t re = rec[r + 1];
    const uint64_t start = wt::walk_start(ca, rec[r], v.gs, wt::lead_of(m, e));
    std::vector<uint64_t> pv(W, ~0ULL), mv(W, 0);
    uint32_t score = m;
    const uintptr_t first = (text_lo + start) & ~(uintptr_t)15, last = text_lo + cb;
    for (uintptr_t blk = first; blk < last; blk += 16) {
        const TextBlock raw = load_block(blk, text_lo, text_hi, 0);
        for (uint32_t i = 0; i < 16; ++i) {
            const uint64_t at = raw.t0 + i;
            if (at < start || at >= cb) continue;
            if (at >= re) {
                lower(slots, targets_flush(best, base, r, 0, v.r1), best);
                best = kNoKey;
                re = long_next_record(rec, r, v.r1, v.ge, at);  // (the loop the kernel spells out)
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
            if (at >= ca && score <= e) best = std::min(best, edit_key(score, at, v.gs, r, 0));
        }
    }
    lower(slots, targets_flush(best, base, r, 0, v.r1), best);
}

struct Call {
    const uint8_t* letters;
    uint64_t letters_bytes;
    const uint64_t* win_begin;
    const uint32_t* win_len;
    uint64_t n_win;
    const wt::View* views;
    uint64_t n_views;
    const uint32_t* pairs;
    uint64_t n_pairs;
};

// the call: plan, prefixes, first keys, the walk of every unit, the compaction
std::vector<uint32_t> run_call(const Call& c, const uint8_t* codes, uint32_t cut, uint64_t n_slots, std::vector<uint32_t>& status) {
    uint8_t cls[256];
    for (unsigned b = 0; b < 256; ++b) cls[b] = codes[b] < 31 ? codes[b] : (uint8_t)31;
    const auto view = [&](uint64_t i) { return wt::view_pair(c.pairs, i, c.win_begin, c.win_len, c.n_win, c.letters_bytes, c.views, c.n_views); };
    std::vector<uint64_t> pref{0}, spref{0};
    status.assign(c.n_pairs, 0);
    for (uint64_t i = 0; i < c.n_pairs; ++i) {  // wt_plan_kernel and the scans
        const wt::Pair v = view(i);
        pref.push_back(pref.back() + wt::units_of_pair(v, cut));
        spref.push_back(spref.back() + targets_slots_of(v.ok, 0, v.r1));
        status[i] = v.ok ? 0u : kTargetsRefused;
    }
    // (exact size: what the init does not write is never read, what lies behind n_slots never written)
    std::vector<uint64_t> slots(n_slots, 0x5555555555555555ULL);
    const uint64_t used = targets_used(spref.data(), c.n_pairs, n_slots);
    for (uint64_t i = 0; i < c.n_pairs; ++i)  // wt_init_kernel
        if (!targets_fits(spref.data(), i, n_slots)) status[i] = kTargetsRefused;
    for (uint64_t s = 0; s < used; ++s) {
        const uint64_t pair = pair_of_unit(spref.data(), c.n_pairs, s);
        uint64_t key = kNoKey;
        if (targets_fits(spref.data(), pair, n_slots)) {
            const wt::Pair v = view(pair);
            key = targets_initial_key(v.m, v.e, v.v.rec, s - spref[pair], 0, v.gs);
        }
        slots[s] = key;
    }
    for (uint64_t u = 0; u < pref.back(); ++u) {  // wt_walk_kernel<W>: the instance of the pair's word count takes the unit
        const uint64_t pair = pair_of_unit(pref.data(), c.n_pairs, u);
        const wt::Pair v = view(pair);
        if (!v.ok || !targets_fits(spref.data(), pair, n_slots)) continue;
        const uint32_t W = wt::words_of(v.m);
        std::vector<uint64_t> peq(32 * W, 0);
        for (uint32_t i = 0; i < v.m; ++i) {
            const uint32_t k = cls[c.letters[v.p0 + i]];
            if (k < 31) peq[k * W + (i >> 6)] |= 1ULL << (i & 63);
        }
        const uint64_t slice = u - pref[pair];
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const ChunkBounds b = chunk_bounds(v.gs, v.ge, slice, 64, lane, cut);
            run_lane(v, peq.data(), cls, W, spref[pair], b.ca, b.cb, slots);
        }
    }
    std::vector<uint32_t> rows;  // wt_count_kernel, wt_write_kernel
    for (uint64_t b = 0; b < targets_blocks(n_slots); ++b)
        for (uint64_t s = b * kTargetsBlock; s < std::min<uint64_t>((b + 1) * kTargetsBlock, used); ++s)
            if (slots[s] != kNoKey) {
                const uint64_t pair = pair_of_unit(spref.data(), c.n_pairs, s);
                const wt::Pair v = view(pair);
                rows.resize(rows.size() + 4);
                targets_row(rows.data() + rows.size() - 4, pair, slots[s], v.v.rec, 0, v.r1, v.gs);
            }
    return rows;
}

// bytes in an allocation of their exact size that begins `shift` bytes behind a 16-byte boundary
struct Exact {
    uint8_t* heap;
    uint8_t* at;
    Exact(const std::vector<uint8_t>& bytes, unsigned shift) {
        // (malloc's blocks begin at a 16-byte boundary; the bytes in front of `at` are not the text's)
        heap = (uint8_t*)std::malloc(bytes.size() + shift + (bytes.size() + shift == 0));
        at = heap + shift;
        std::memset(heap, 0xEE, shift);
        if (!bytes.empty()) std::memcpy(at, bytes.data(), bytes.size());
    }
    ~Exact() { std::free(heap); }
    Exact(const Exact&) = delete;
};

}  // namespace

int main() {
    std::mt19937_64 rng(20250922);
    size_t cases = 0, hits = 0;
    const uint32_t lengths[] = {1, 63, 64, 65, 128, 129, 256, 257, 512};
    for (unsigned letters : {4u, 20u}) {
        uint8_t codes[256];
        for (unsigned b = 0; b < 256; ++b) codes[b] = 255;
        for (unsigned l = 0; l < letters; ++l) codes['A' + l] = codes['a' + l] = (uint8_t)l;
        const auto letter = [&]() -> uint8_t {
            if (rng() % 25 == 0) return rng() % 2 ? (uint8_t)'#' : (uint8_t)(rng() % 256);  // mostly no class
            return (uint8_t)((rng() % 2 ? 'A' : 'a') + rng() % letters);
        };
        for (uint32_t m : lengths) {
            // the letter buffer: the window in the middle of it, a second window that overlaps it by all but 3 letters, and a third
            // that ends with the buffer
            const uint32_t front = (uint32_t)(rng() % 20), behind = 3 + (uint32_t)(rng() % 20);
            std::vector<uint8_t> buffer(front + m + behind);
            for (uint8_t& c : buffer) c = letter();
            const std::vector<uint8_t> p(buffer.begin() + front, buffer.begin() + front + m);
            const auto edited = [&](const std::vector<uint8_t>& of, unsigned edits) {
                std::vector<uint8_t> copy = of;
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
            const std::vector<uint8_t> tail(buffer.end() - m, buffer.end());
            // view 0: empty records at the front, between and at the end; one byte; m - 1 bytes; three with edited copies, one of
            // them twice; a run of records of 0..3 bytes (many flushes inside one chunk)
            std::vector<uint8_t> text;
            std::vector<uint64_t> rec{0};
            const auto add = [&](const std::vector<uint8_t>& body, size_t before, size_t after) {
                for (size_t i = 0; i < before; ++i) text.push_back(letter());
                text.insert(text.end(), body.begin(), body.end());
                for (size_t i = 0; i < after; ++i) text.push_back(letter());
                rec.push_back(text.size());
            };
            add({}, 0, 0);
            add({}, 1, 0);
            add(edited(p, 3), rng() % 40, rng() % 40);
            add({}, 0, 0);
            add({}, 0, 0);
            add({}, m - 1, 0);
            add(edited(p, 2), rng() % 40, rng() % 40);
            for (unsigned k = 0; k < 12; ++k) add({}, k % 4, 0);
            add(p, rng() % 70, 0);
            {
                std::vector<uint8_t> twice = edited(p, 1);
                for (unsigned k = 0; k < 30; ++k) twice.push_back(letter());
                twice.insert(twice.end(), p.begin(), p.end());
                add(twice, 3, 2);
            }
            add(edited(tail, 1), 5, 0);
            add({}, 0, 0);
            // view 1: another text somewhere else, its offsets not from 0 (the bytes in front of rec[0] belong to no record)
            std::vector<uint8_t> text1;
            for (unsigned k = 0; k < 7; ++k) text1.push_back(letter());
            std::vector<uint64_t> rec1{7};
            for (unsigned k = 0; k < 3; ++k) {
                const std::vector<uint8_t> body = edited(k == 1 ? tail : p, k);
                for (unsigned i = 0; i < 10 * k; ++i) text1.push_back(letter());
                text1.insert(text1.end(), body.begin(), body.end());
                rec1.push_back(text1.size());
            }
            const std::vector<uint64_t> rec_none{3};  // view 2: no records
            for (unsigned shift : {0u, 3u}) {
                const Exact let(buffer, shift ? 5 : 0), t0(text, shift), t1(text1, shift ? 1 : 0);
                // (offsets in vectors of their exact size: ASan sees a read behind rec[n_rec])
                const std::vector<uint64_t> r0v(rec), r1v(rec1);
                const std::vector<wt::View> views{{t0.at, r0v.data(), r0v.size() - 1, text.size()},
                                                  {t1.at, r1v.data(), r1v.size() - 1, text1.size()},
                                                  {t1.at, rec_none.data(), 0, text1.size()},
                                                  {t0.at, r0v.data(), r0v.size() - 1, text.size() - 1},     // its offsets leave text_bytes
                                                  {t1.at, r1v.data() + 1, 1, 4}};                            // ends beyond text_bytes
                const std::vector<uint64_t> wb{front, (uint64_t)front + 3, buffer.size() - m, buffer.size() - m + 1, 0, buffer.size() + 1};
                const std::vector<uint32_t> wl{m, m, m, m, 0, 1};  // (windows 3 and 5 leave the buffer, window 4 is empty)
                tetrex::EditPattern ep0(p.data(), m, codes), ep1(buffer.data() + front + 3, m, codes), ep2(tail.data(), m, codes);
                tetrex::EditPattern* const eps[3] = {&ep0, &ep1, &ep2};
                const uint32_t big = (uint32_t)((text.size() + 16) / 16 * 16);
                for (uint32_t cut : {16u, 64u, big}) {
                    if (shift && cut != 64) continue;
                    for (uint32_t cap : {0u, 3u, m - 1, m, m + 5}) {
                        // pairs: good ones between one of every refusal; the view of no records; the same view twice
                        const std::vector<uint32_t> pairs{0, 0, cap, 3, 0, cap, 1, 1, cap, 0, 5, cap, 2, 0, cap, 0, 2, cap, 4, 0, cap, 0, 3, cap,
                                                          2, 1, cap, 6, 0, cap, 5, 1, cap, 0, 4, cap, 1, 0, cap, 0xFFFFFFFFu, 0xFFFFFFFFu, cap, 0, 1, cap};
                        const uint64_t n_pairs = pairs.size() / 3;
                        const Call call{let.at, buffer.size(), wb.data(), wl.data(), wb.size(), views.data(), views.size(), pairs.data(), n_pairs};
                        std::vector<bool> good(n_pairs);
                        uint64_t need = 0;
                        for (uint64_t i = 0; i < n_pairs; ++i) {
                            const uint32_t w = pairs[3 * i], g = pairs[3 * i + 1];
                            good[i] = w < 3 && g < 3;
                            if (good[i]) need += views[g].n_rec;
                        }
                        for (uint64_t n_slots : {need, need - 1, need + 300}) {
                            if (n_slots != need && (cut != 64 || cap != 3)) continue;
                            std::vector<uint32_t> want, want_status(n_pairs, kTargetsRefused), status;
                            uint64_t at = 0;
                            for (uint64_t i = 0; i < n_pairs; ++i) {
                                if (!good[i]) continue;
                                const wt::View& v = views[pairs[3 * i + 1]];
                                at += v.n_rec;
                                if (at > n_slots) continue;
                                want_status[i] = 0;
                                tetrex::edit_targets_group(*eps[pairs[3 * i]], v.text, v.rec, 0, v.n_rec, cap, (uint32_t)i, want);
                            }
                            const std::vector<uint32_t> got = run_call(call, codes, cut, n_slots, status);
                            ++cases;
                            hits += got.size() / 4;
                            if (got != want || status != want_status) {
                                size_t d = 0;
                                while (d < got.size() && d < want.size() && got[d] == want[d]) ++d;
                                d = d / 4 * 4;
                                std::printf("edit_window_targets_sim: %u letters, m = %u, cut %u, cap %u, %llu slots, shift %u: %zu rows, the host %zu; first "
                                            "difference at row %zu",
                                            letters, m, cut, cap, (unsigned long long)n_slots, shift, got.size() / 4, want.size() / 4, d / 4);
                                if (d + 4 <= got.size()) std::printf(": (%u, %u, %u, %u)", got[d], got[d + 1], got[d + 2], got[d + 3]);
                                if (d + 4 <= want.size()) std::printf(", the host (%u, %u, %u, %u)", want[d], want[d + 1], want[d + 2], want[d + 3]);
                                std::printf("; status");
                                for (uint64_t i = 0; i < n_pairs; ++i) std::printf(" %x/%x", status[i], want_status[i]);
                                std::printf("\n");
                                return 1;
                            }
                        }
                    }
                }
            }
        }
    }
    std::printf("edit_window_targets_sim ok: %zu cases, %zu hits\n", cases, hits);
    return 0;
}
