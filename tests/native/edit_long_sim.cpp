// Stand-alone check of csrc/txq_edit_long_plan.hpp: the systolic schedule of the long-pattern edit-distance kernel
// (txq_edit_long.hip) run on the CPU — the lanes of a group as an array, the cross-lane move as a shift by one, units and
// spans cut as the kernel cuts them, the text read through load_block — against edit_search_group of host/edit_distance.hpp.
// Built with sanitizers by tests/test_edit_long_sim.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/edit_long_sim.cpp -o sim && ./sim
// Prints "edit_long_sim ok: <cases> cases" and exits 0, or names the first case that differs and exits 1.
#include "../../tetrex_amd/csrc/host/edit_distance.hpp"
#include "../../tetrex_amd/csrc/txq_edit_long_plan.hpp"

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

// one group of G lanes on the span [ca, cb) of the text [gs, ge), records [r0, r1): the least key, as the kernel finds it
uint64_t run_span(const Text& t, const uint64_t* peq, const uint8_t* codes, uint32_t G, uint32_t m, uint32_t e, uint64_t r0, uint64_t r1, uint64_t gs,
                  uint64_t ge, uint64_t ca, uint64_t cb) {
    if (ca >= ge) return kNoKey;
    const uintptr_t text_lo = (uintptr_t)t.bytes, text_hi = text_lo + t.n;
    const uint32_t hw = (m - 1) >> 6;
    uint64_t rf = record_of(t.rec, r0, r1, ca), rf_end = t.rec[rf + 1];
    const uint64_t start = long_start(ca, t.rec[rf], gs, m, e);
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
            {
                const uint64_t at = t0 + s;
                if (s < columns && at >= start && at < cb) {
                    const bool reset = at >= rf_end;
                    if (reset) rf_end = long_next_record(t.rec, rf, r1, ge, at);
                    in[0] = long_feed(codes[(raw.w[i >> 2] >> (8 * (i & 3))) & 255u], reset);
                }
            }
            for (uint32_t w = 0; w < G; ++w) {
                const uint32_t bit = w == hw ? (m - 1) & 63 : 63u;
                out[w] = long_block_step(pv[w], mv[w], peq[(in[w] & kMsgClass) * G + w], in[w], bit);
                if (w == hw && (out[w] & kMsgValid)) {
                    const uint64_t at = t0 + s - hw;
                    if (out[w] & kMsgReset) {
                        score = m;
                        (void)long_next_record(t.rec, rs, r1, ge, at);
                    }
                    score += (uint32_t)long_hin(out[w]);
                    if (at >= ca && score <= e) best = std::min(best, edit_key(score, at, gs, rs, r0));
                }
            }
        }
    }
    return best;
}

tetrex::EditResult run_pair(const Text& t, const std::vector<uint8_t>& p, const uint8_t* codes, uint64_t r0, uint64_t r1, uint32_t e, uint32_t span) {
    const uint32_t m = (uint32_t)p.size(), G = long_group_lanes(m);
    uint8_t cls[256];
    for (unsigned b = 0; b < 256; ++b) cls[b] = codes[b] < 31 ? codes[b] : (uint8_t)31;
    std::vector<uint64_t> peq(32 * G, 0);
    for (uint32_t i = 0; i < m; ++i)
        if (cls[p[i]] < 31) peq[cls[p[i]] * G + (i >> 6)] |= 1ULL << (i & 63);
    const uint64_t gs = t.rec[r0], ge = t.rec[r1];
    uint64_t key = r1 > r0 && m <= e ? (uint64_t)m << kPosBits : kNoKey;  // (the plan kernel's part)
    const uint64_t units = long_units(ge - gs, G, span);
    for (uint64_t slice = 0; slice < units; ++slice)
        for (uint32_t group = 0; group < long_groups(G); ++group) {
            const ChunkBounds c = long_span(gs, ge, slice, G, group, span);
            key = std::min(key, run_span(t, peq.data(), cls, G, m, e, r0, r1, gs, ge, c.ca, c.cb));
        }
    tetrex::EditResult res;
    if (key != kNoKey) {
        const EditAnswer a = edit_answer(key, t.rec, r0, r1, gs);
        res.distance = a.d, res.record = a.r, res.end = a.j;
    }
    return res;
}

}  // namespace

int main() {
    std::mt19937_64 rng(20250111);
    size_t cases = 0;
    const uint32_t lengths[] = {1, 64, 65, 513, 1023, 1024, 1025, 2048, 2049, 4033, 4096};
    for (unsigned letters : {4u, 20u}) {
        uint8_t codes[256];
        for (unsigned b = 0; b < 256; ++b) codes[b] = 255;
        for (unsigned l = 0; l < letters; ++l) codes['A' + l] = codes['a' + l] = (uint8_t)l;
        const auto letter = [&]() -> uint8_t {
            if (rng() % 25 == 0) return rng() % 2 ? (uint8_t)'#' : (uint8_t)(rng() % 256);  // mostly no class
            return (uint8_t)((rng() % 2 ? 'A' : 'a') + rng() % letters);
        };
        for (uint32_t m : lengths) {
            if (long_group_lanes(m) < (m + 63) / 64 || long_group_lanes(m) > 64) return std::printf("edit_long_sim: group of m = %u\n", m), 1;
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
            // records: empty ones at the front, between and at the end; one byte; m - 1 bytes; two with edited copies
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
            add({}, 0, 0);
            // a heap copy of exactly the text's size, once at a 16-byte boundary and once 3 bytes behind one
            const uint64_t n = text.size(), R = rec.size() - 1;
            for (unsigned shift : {0u, 3u}) {
                uint8_t* heap = (uint8_t*)std::aligned_alloc(16, (size_t)((n + shift + 15) / 16 * 16));
                std::memcpy(heap + shift, text.data(), (size_t)n);
                const Text t{heap + shift, n, rec.data()};
                tetrex::EditPattern ep(p.data(), m, codes);
                const uint32_t big = (uint32_t)((n + 16) / 16 * 16);
                // Every m runs every cap (with one span over the whole text) and every span.  Patterns above 1100 bytes, where a
                // short span walks a lead-in of up to 2 m bytes for its few own ones, take the short spans at fewer caps: 3 at
                // span 16; 3 and m at span 64; m - 1 on the shifted text.
                const bool large = m > 1100;
                for (uint32_t span : {16u, 64u, big}) {
                    if (shift && span != 64) continue;
                    for (uint32_t cap : {0u, 3u, m - 1, m, m + 5}) {
                        if (large && span == 16 && cap != 3) continue;
                        if (large && span == 64 && (shift ? cap != m - 1 : cap != 3 && cap != m)) continue;
                        for (uint64_t r0 : {(uint64_t)0, (uint64_t)3, R}) {
                            if (r0 == 3 && (span == 16 || shift || (large && span == 64))) continue;
                            const tetrex::EditResult want = tetrex::edit_search_group(ep, t.bytes, t.rec, r0, R, cap);
                            const tetrex::EditResult got = run_pair(t, p, codes, r0, R, cap, span);
                            ++cases;
                            if (got.distance != want.distance || got.record != want.record || got.end != want.end) {
                                std::printf("edit_long_sim: %u letters, m = %u, span %u, cap %u, records %llu..%llu, text at +%u: (%u, %u, %u), the host (%u, %u, %u)\n",
                                            letters, m, span, cap, (unsigned long long)r0, (unsigned long long)R, shift, got.distance, got.record, got.end,
                                            want.distance, want.record, want.end);
                                return 1;
                            }
                        }
                    }
                }
                std::free(heap);
            }
        }
    }
    std::printf("edit_long_sim ok: %zu cases\n", cases);
    return 0;
}
