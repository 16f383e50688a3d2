// Stand-alone check of csrc/txq_edit_windows_plan.hpp: the windowed edit-distance kernel (txq_edit_windows.hip) run on the CPU
// the way the device runs it — the plan kernel's heads and unit counts, a prefix over them, every unit looked up with
// pair_of_unit, the bundle's extent, the 64 lanes' chunks, the shared lead-in, the text read through load_block and the K
// states of a bundle stepped per byte — against edit_search_group of host/edit_distance.hpp on the written-out window.
// It also asserts that every pair belongs to exactly one bundle.  Built with sanitizers by tests/test_edit_windows_sim.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/edit_windows_sim.cpp -o sim && ./sim
// Prints "edit_windows_sim ok: <pairs> pairs, <bundles> bundles" and exits 0, or names the first difference and exits 1.
#include "../../tetrex_amd/csrc/host/edit_distance.hpp"
#include "../../tetrex_amd/csrc/txq_edit_common.hpp"
#include "../../tetrex_amd/csrc/txq_edit_windows_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace txq;

namespace {

constexpr uint32_t kMaxWindow = 512;

struct Call {
    const uint8_t* letters;
    uint64_t letters_bytes;
    std::vector<uint64_t> win_begin;
    std::vector<uint32_t> win_len;
    TextGroups t;
    std::vector<uint32_t> pairs;  // (window, group, cap)
    const uint8_t* codes;
    uint32_t chunk, cap;
    uint64_t n_pairs() const { return pairs.size() / 3; }
};

struct View {
    bool ok = false;
    uint32_t m = 0, e = 0, g = 0;
    uint64_t p0 = 0, r0 = 0, r1 = 0, gs = 0, ge = 0;
};

// view_window of the kernel
View view(const Call& c, uint64_t i) {
    View v;
    const uint32_t p = c.pairs[3 * i];
    v.g = c.pairs[3 * i + 1], v.e = c.pairs[3 * i + 2];
    if (p >= c.win_begin.size()) return v;
    const uint64_t p0 = c.win_begin[p];
    const uint32_t m = c.win_len[p];
    if (m == 0 || m > kMaxWindow || p0 > c.letters_bytes || m > c.letters_bytes - p0) return v;
    const GroupView gv = view_group(c.t, v.g);
    v.ok = gv.ok, v.m = m, v.p0 = p0, v.r0 = gv.r0, v.r1 = gv.r1, v.gs = gv.gs, v.ge = gv.ge;
    return v;
}
ew::Member member(const Call& c, uint64_t i) {
    const View v = view(c, i);
    return {v.ok, v.g, v.ok ? ew::words_of(v.m) : 0u};
}

// one state: Myers' recurrence over `words` words
struct State {
    uint32_t m, e, words, score;
    std::vector<uint64_t> peq, pv, mv;  // peq[32 * words]
    uint64_t best = kNoKey;
    void reset() {
        std::fill(pv.begin(), pv.end(), ~0ULL);
        std::fill(mv.begin(), mv.end(), 0ULL);
        score = m;
    }
    void step(uint32_t cls) {
        const uint32_t hw = (m - 1) >> 6, hs = (m - 1) & 63;
        uint64_t carry = 0, ph_in = 0, mh_in = 0;
        uint32_t hp = 0, hm = 0;
        for (uint32_t w = 0; w < words; ++w) {
            const uint64_t eq = peq[cls * words + w], p = pv[w], n = mv[w];
            const uint64_t xv = eq | n, x = eq & p;
            const uint64_t s1 = x + p, s2 = s1 + carry;
            carry = (uint64_t)(s1 < x) | (uint64_t)(s2 < s1);
            const uint64_t xh = (s2 ^ p) | eq;
            uint64_t ph = n | ~(xh | p), mh = p & xh;
            if (w == hw) hp = (uint32_t)(ph >> hs) & 1u, hm = (uint32_t)(mh >> hs) & 1u;
            const uint64_t ph_out = ph >> 63, mh_out = mh >> 63;
            ph = (ph << 1) | ph_in;
            mh = (mh << 1) | mh_in;
            ph_in = ph_out, mh_in = mh_out;
            pv[w] = mh | ~(xv | ph);
            mv[w] = ph & xv;
        }
        score += hp - hm;
    }
};

// the whole call: out[3 i ..] = (d, r, j) as the device writes them; owner[i] counts the bundles pair i was a member of
bool run_call(const Call& c, std::vector<uint32_t>& out, std::vector<uint32_t>& owner, size_t& n_bundles) {
    const uint64_t N = c.n_pairs();
    std::vector<uint64_t> keys(N), pref(N + 1, 0);
    uint8_t cls[256];
    for (unsigned b = 0; b < 256; ++b) cls[b] = c.codes[b] < 31 ? c.codes[b] : (uint8_t)31;
    // the plan kernel, then the scan
    for (uint64_t i = 0; i < N; ++i) {
        const View v = view(c, i);
        uint64_t units = 0, key = kBadPair;
        if (v.ok) {
            const ew::Member prev = i ? member(c, i - 1) : ew::Member{};
            if (ew::is_head(i, prev, member(c, i), c.cap)) units = units_of(v.ge - v.gs, 64, c.chunk);
            key = v.r1 > v.r0 && v.m <= v.e ? (uint64_t)v.m << kPosBits : kNoKey;
        }
        pref[i + 1] = pref[i] + units;
        keys[i] = key;
    }
    owner.assign(N, 0);
    // every pair's bundle by the rule alone (a group of no bytes has no units, yet its pairs are in bundles all the same)
    for (uint64_t i = 0; i < N; ++i) {
        const ew::Member cur = member(c, i), prev = i ? member(c, i - 1) : ew::Member{};
        if (!ew::is_head(i, prev, cur, c.cap)) continue;
        ++n_bundles;
        const uint32_t n = cur.ok ? ew::bundle_extent(i, N, c.cap, [&](uint64_t x) { return member(c, x); }) : 1u;
        if (cur.ok && n > ew::bundle_size(cur.words, c.cap)) return std::printf("edit_windows_sim: a bundle of %u pairs at pair %llu\n", n, (unsigned long long)i), false;
        for (uint32_t k = 0; k < n; ++k) ++owner[i + k];
    }
    const uintptr_t text_lo = (uintptr_t)c.t.text, text_hi = text_lo + c.t.text_bytes;
    const uint64_t total = pref[N];
    for (uint64_t u = 0; u < total; ++u) {
        const uint64_t head = pair_of_unit(pref.data(), N, u);
        const View v = view(c, head);
        if (!v.ok) return std::printf("edit_windows_sim: unit %llu belongs to a refused pair\n", (unsigned long long)u), false;
        const uint32_t n = ew::bundle_extent(head, N, c.cap, [&](uint64_t x) { return member(c, x); });
        if (n > ew::bundle_size(ew::words_of(v.m), c.cap)) return std::printf("edit_windows_sim: no instance for a bundle of %u\n", n), false;
        const uint64_t slice = u - pref[head];
        std::vector<State> st(n);
        uint64_t lead = 0;
        for (uint32_t k = 0; k < n; ++k) {
            const View vk = view(c, head + k);
            if (!vk.ok || vk.g != v.g || ew::words_of(vk.m) != ew::words_of(v.m)) return std::printf("edit_windows_sim: a stranger in a bundle\n"), false;
            State& s = st[k];
            s.m = vk.m, s.e = vk.e, s.words = ew::words_of(vk.m);
            s.peq.assign(32 * s.words, 0), s.pv.resize(s.words), s.mv.resize(s.words);
            for (uint32_t i = 0; i < vk.m; ++i) {
                const uint32_t cl = cls[c.letters[vk.p0 + i]];
                if (cl < 31) s.peq[cl * s.words + (i >> 6)] |= 1ULL << (i & 63);
            }
            lead = std::max(lead, ew::lead_of(vk.m, vk.e));
        }
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const ChunkBounds cb = chunk_bounds(v.gs, v.ge, slice, 64, lane, c.chunk);
            const uint64_t ca = cb.ca, ce = cb.cb;
            if (ca >= v.ge) continue;
            uint64_t r = record_of(c.t.rec, v.r0, v.r1, ca);
            uint64_t rs = c.t.rec[r], re = c.t.rec[r + 1];
            if (rs < v.gs || rs > ca) rs = ca;
            const uint64_t start = ew::walk_start(ca, rs, lead);
            for (State& s : st) s.reset(), s.best = kNoKey;
            const uintptr_t first = (text_lo + start) & ~(uintptr_t)15, last = text_lo + ce;
            for (uintptr_t blk = first; blk < last; blk += 16) {
                const TextBlock raw = load_block(blk, text_lo, text_hi, 0);
                for (uint32_t i = 0; i < 16; ++i) {
                    const uint64_t t = raw.t0 + i;
                    if (t < start || t >= ce) continue;
                    if (t >= re) {
                        do {
                            ++r;
                            re = r + 1 <= v.r1 ? c.t.rec[r + 1] : v.ge;
                        } while (t >= re && r + 1 < v.r1);
                        if (re > v.ge || t >= re) re = v.ge;
                        for (State& s : st) s.reset();
                    }
                    const uint32_t cl = cls[(raw.w[i >> 2] >> (8 * (i & 3))) & 255u];
                    for (State& s : st) {
                        s.step(cl);
                        if (t >= ca && s.score <= s.e) s.best = std::min(s.best, edit_key(s.score, t, v.gs, r, v.r0));
                    }
                }
            }
            for (uint32_t k = 0; k < n; ++k) keys[head + k] = std::min(keys[head + k], st[k].best);
        }
    }
    // the finish kernel
    out.assign(3 * N, 0xFFFFFFFFu);
    for (uint64_t i = 0; i < N; ++i) {
        if (keys[i] == kBadPair) out[3 * i + 1] = out[3 * i + 2] = 0xFFFFFFFEu;
        else if (keys[i] != kNoKey) {
            const View v = view(c, i);
            const EditAnswer a = edit_answer(keys[i], c.t.rec, v.r0, v.r1, v.gs);
            out[3 * i] = a.d, out[3 * i + 1] = a.r, out[3 * i + 2] = a.j;
        }
    }
    return true;
}

}  // namespace

int main() {
    std::mt19937_64 rng(20250619);
    size_t n_checked = 0, n_bundles = 0, n_hits = 0;
    for (unsigned letters : {4u, 20u}) {
        uint8_t codes[256];
        for (unsigned b = 0; b < 256; ++b) codes[b] = 255;
        for (unsigned l = 0; l < letters; ++l) codes['A' + l] = codes['a' + l] = (uint8_t)l;
        const auto letter = [&]() -> uint8_t {
            if (rng() % 40 == 0) return rng() % 2 ? (uint8_t)'#' : (uint8_t)(rng() % 256);  // mostly no class
            return (uint8_t)((rng() % 2 ? 'A' : 'a') + rng() % letters);
        };
        // the text: three groups of records with empty ones in front, between and behind, and a group of no records
        std::vector<uint8_t> text;
        std::vector<uint64_t> rec{0};
        const auto add = [&](size_t n) {
            for (size_t i = 0; i < n; ++i) text.push_back(letter());
            rec.push_back(text.size());
        };
        for (size_t n : {0, 0, 700, 0, 1, 0, 0, 1300, 0}) add(n);   // group 0: records 0 .. 8
        for (size_t n : {900, 40}) add(n);                          // group 1: records 9, 10
        for (size_t n : {0, 0}) add(n);                             // group 3 (group 2 has none): two empty records
        const std::vector<uint64_t> grp{0, 9, 11, 11, 13};
        // the letters: one record with stretches cut from the text (edited), windows slid over it
        std::vector<uint8_t> let;
        const auto plant = [&](uint64_t from, size_t n, unsigned edits) {
            std::vector<uint8_t> cut(text.begin() + (long)from, text.begin() + (long)(from + n));
            for (; edits > 0; --edits) {
                const size_t at = (size_t)(rng() % cut.size());
                switch (rng() % 3) {
                    case 0: cut[at] = letter(); break;
                    case 1: cut.insert(cut.begin() + (long)at, letter()); break;
                    default: cut.erase(cut.begin() + (long)at); break;
                }
            }
            let.insert(let.end(), cut.begin(), cut.end());
        };
        plant(100, 600, 6);                            // from record 2
        for (int i = 0; i < 80; ++i) let.push_back(letter());
        plant(rec[7] + 200, 900, 12);                  // from record 7
        plant(rec[9] + 10, 700, 5);                    // from record 9 (group 1)
        const uint64_t L = let.size();
        std::vector<uint64_t> wb;
        std::vector<uint32_t> wl;
        std::vector<uint32_t> first_of_len;  // the first window of each length
        for (uint32_t m : {1u, 63u, 64u, 65u, 128u, 129u, 256u, 257u, 512u, 40u, 100u}) {
            first_of_len.push_back((uint32_t)wb.size());
            const uint32_t step = std::max(1u, m / 3);
            for (uint64_t at = 0; at + m <= L && wb.size() - first_of_len.back() < 24; at += step) wb.push_back(at), wl.push_back(m);
            wb.push_back(L - m), wl.push_back(m);  // the last byte of the buffer
        }
        const uint32_t n_win = (uint32_t)wb.size();
        wb.push_back(L - 3), wl.push_back(4);    // leaves the letters
        wb.push_back(0), wl.push_back(0);        // no letters
        wb.push_back(0), wl.push_back(513);      // too long
        for (unsigned shift : {0u, 3u}) {
            const uint64_t n = text.size();
            uint8_t* heap = (uint8_t*)std::aligned_alloc(16, (size_t)((n + shift + 15) / 16 * 16));
            std::memcpy(heap + shift, text.data(), (size_t)n);
            uint8_t* lheap = (uint8_t*)std::malloc((size_t)L);  // (exactly the letters: a read behind them is caught)
            std::memcpy(lheap, let.data(), (size_t)L);
            for (uint32_t chunk : {16u, 64u, 512u})
                for (uint32_t cap : {1u, 2u, 4u}) {
                    if (shift && (chunk != 16 || cap != 4)) continue;
                    Call c{lheap, L, wb, wl, {heap + shift, rec.data(), rec.size() - 1, n, grp.data(), grp.size() - 1}, {}, codes, chunk, cap};
                    // runs of windows per (length, group): lengths mix in the pair list so that runs begin at every i % K;
                    // caps change inside a run; refused pairs and group changes sit in the first half of a run, the second is unbroken
                    for (size_t li = 0; li < first_of_len.size(); ++li) {
                        const uint32_t w0 = first_of_len[li], w1 = li + 1 < first_of_len.size() ? first_of_len[li + 1] : n_win, m = wl[w0];
                        const uint32_t caps[] = {0u, 3u, m - 1, m, m + 5};
                        uint32_t at = 0;
                        for (uint32_t w = w0; w < w1; ++w, ++at) {
                            const uint32_t e = chunk == 16 && m > 300 ? 3u : caps[(at / 3) % 5];  // (long lead-ins at chunk 16: fewer caps)
                            c.pairs.insert(c.pairs.end(), {w, at % 11 == 7 ? 1u : 0u, e});
                            if (at >= 14) continue;  // (the rest of the run is unbroken: full bundles)
                            if (at % 9 == 4) c.pairs.insert(c.pairs.end(), {n_win + at % 3, 0u, 3u});       // refused: the window
                            if (at % 13 == 6) c.pairs.insert(c.pairs.end(), {w, 9u, 3u});                   // refused: the group
                            if (at % 10 == 3) c.pairs.insert(c.pairs.end(), {w, 2u, m + 5});                // a group of no records
                            if (at % 10 == 8) c.pairs.insert(c.pairs.end(), {w, 3u, m + 5});                // a group of empty records
                        }
                        c.pairs.insert(c.pairs.end(), {n_win + 7, 0u, 3u});  // refused: no such window
                    }
                    std::vector<uint32_t> got, owner;
                    if (!run_call(c, got, owner, n_bundles)) return 1;
                    for (uint64_t i = 0; i < c.n_pairs(); ++i) {
                        if (owner[i] != 1) return std::printf("edit_windows_sim: pair %llu is in %u bundles (cap %u)\n", (unsigned long long)i, owner[i], cap), 1;
                        const uint32_t p = c.pairs[3 * i], g = c.pairs[3 * i + 1], e = c.pairs[3 * i + 2];
                        uint32_t want[3] = {0xFFFFFFFFu, 0xFFFFFFFEu, 0xFFFFFFFEu};
                        if (p < n_win && g < grp.size() - 1) {
                            tetrex::EditPattern ep(let.data() + wb[p], wl[p], codes);
                            const tetrex::EditResult r = tetrex::edit_search_group(ep, c.t.text, rec.data(), grp[g], grp[g + 1], e);
                            want[0] = r.distance, want[1] = r.record, want[2] = r.end;
                            n_hits += r.distance != 0xFFFFFFFFu;
                        }
                        ++n_checked;
                        if (std::memcmp(want, got.data() + 3 * i, 12) != 0) {
                            std::printf("edit_windows_sim: %u letters, chunk %u, cap %u, text at +%u, pair %llu (window %u of %u at %llu, group %u, e %u): (%u, %u, %u), the host (%u, %u, %u)\n",
                                        letters, chunk, cap, shift, (unsigned long long)i, p, p < wl.size() ? wl[p] : 0u, (unsigned long long)(p < wb.size() ? wb[p] : 0), g, e,
                                        got[3 * i], got[3 * i + 1], got[3 * i + 2], want[0], want[1], want[2]);
                            return 1;
                        }
                    }
                }
            std::free(heap);
            std::free(lheap);
        }
    }
    if (n_hits * 4 < n_checked || n_hits * 4 > n_checked * 3) return std::printf("edit_windows_sim: %zu hits of %zu pairs: the cases show too little\n", n_hits, n_checked), 1;
    std::printf("edit_windows_sim ok: %zu pairs, %zu bundles, %zu hits\n", n_checked, n_bundles, n_hits);
    return 0;
}
