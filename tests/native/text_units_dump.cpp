// What the text kernels share (tetrex_amd/csrc/txq_text.hpp) without a GPU: commands come in on stdin, one per line, each
// answered by one line on stdout; tests/test_text_units.py holds the cases and what they must give.  Every array is a heap
// allocation of exactly its size, so that the address sanitizer sees a read outside it.
//   pair   n pref[0 .. n] u                                   -> pair_of_unit
//   record n rec[0 .. n] r0 r1 x                              -> record_of
//   group  g n_grp grp[0 .. n_grp] n_rec rec[0 .. n_rec] text_bytes -> "ok r0 r1 gs ge" of view_group
//   units  bytes lanes chunk                                  -> units_of
//   chunk  gs ge slice lanes lane chunk                       -> "ca cb" of chunk_bounds
//   load   residue len fill   -> load_block on every 16-byte block that meets a text of `len` bytes which begins `residue` bytes
//                                behind a 16-byte boundary: "t0 whole 32-hex-digits" per block, separated by ';'.  Text byte j is
//                                128 + (37 j + 11) mod 100.  The allocation ends with the text; the `residue` bytes in front
//                                of it hold 0xEE and are poisoned as far as the sanitizer's 8-byte granules allow.
#include "../../tetrex_amd/csrc/txq_text.hpp"

#include <sanitizer/asan_interface.h>

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace txq;

static bool numbers(std::vector<uint64_t>& v, size_t n) {
    v.assign(n, 0);
    v.shrink_to_fit();
    for (uint64_t& x : v)
        if (scanf("%" SCNu64, &x) != 1) return false;
    return true;
}

int main() {
    char cmd[16];
    std::vector<uint64_t> a, b, c;
    while (scanf("%15s", cmd) == 1) {
        bool ok = true;
        if (!strcmp(cmd, "pair")) {
            ok = numbers(a, 1) && numbers(b, a[0] + 1) && numbers(c, 1);
            if (ok) printf("%" PRIu64 "\n", pair_of_unit(b.data(), a[0], c[0]));
        } else if (!strcmp(cmd, "record")) {
            ok = numbers(a, 1) && numbers(b, a[0] + 1) && numbers(c, 3);
            if (ok) printf("%" PRIu64 "\n", record_of(b.data(), c[0], c[1], c[2]));
        } else if (!strcmp(cmd, "group")) {
            std::vector<uint64_t> grp, rec;
            ok = numbers(a, 2) && numbers(grp, a[1] + 1) && numbers(b, 1) && numbers(rec, b[0] + 1) && numbers(c, 1);
            if (ok) {
                const TextGroups t{nullptr, rec.data(), b[0], c[0], grp.data(), a[1]};
                const GroupView v = view_group(t, (uint32_t)a[0]);
                printf("%d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", (int)v.ok, v.r0, v.r1, v.gs, v.ge);
            }
        } else if (!strcmp(cmd, "units")) {
            ok = numbers(a, 3);
            if (ok) printf("%" PRIu64 "\n", units_of(a[0], (uint32_t)a[1], (uint32_t)a[2]));
        } else if (!strcmp(cmd, "chunk")) {
            ok = numbers(a, 6);
            if (ok) {
                const ChunkBounds cb = chunk_bounds(a[0], a[1], a[2], (uint32_t)a[3], (uint32_t)a[4], (uint32_t)a[5]);
                printf("%" PRIu64 " %" PRIu64 "\n", cb.ca, cb.cb);
            }
        } else if (!strcmp(cmd, "load")) {
            ok = numbers(a, 3) && a[0] < 16 && a[1] > 0;
            if (ok) {
                const size_t residue = a[0], len = a[1];
                void* mem = nullptr;
                if (posix_memalign(&mem, 16, residue + len)) return 2;
                uint8_t* base = static_cast<uint8_t*>(mem);
                memset(base, 0xEE, residue);
                for (size_t j = 0; j < len; ++j) base[residue + j] = (uint8_t)(128 + (37 * j + 11) % 100);
                ASAN_POISON_MEMORY_REGION(base, residue);
                const uintptr_t lo = (uintptr_t)base + residue, hi = lo + len;
                for (uintptr_t blk = (uintptr_t)base; blk < hi; blk += 16) {
                    const TextBlock t = load_block(blk, lo, hi, (uint8_t)a[2]);
                    printf("%s%" PRIu64 " %d ", blk == (uintptr_t)base ? "" : ";", t.t0, (int)t.whole);
                    for (int q = 0; q < 4; ++q)
                        for (int i = 0; i < 4; ++i) printf("%02x", (unsigned)((t.w[q] >> (8 * i)) & 255u));
                }
                printf("\n");
                ASAN_UNPOISON_MEMORY_REGION(base, residue);
                free(mem);
            }
        } else {
            fprintf(stderr, "text_units_dump: unknown command %s\n", cmd);
            return 2;
        }
        if (!ok) {
            fprintf(stderr, "text_units_dump: bad input for %s\n", cmd);
            return 2;
        }
    }
    return 0;
}
