"""The plan of the flat probe's sorted answer (csrc/txq_probe_plan.hpp plan_probe_sort, sort_tile) without a GPU:
tests/native/probe_sort_plan_dump.cpp, built with the address and undefined-behaviour sanitizers, answers one command per line.
Expected values are worked out by hand: a bucket is the largest power of two of rows within TXQ_PROBE_SORT_BUCKET_KB (1024 KiB of
128-byte rows: 2^13 rows), widened until at most 256 buckets cover the table; a workgroup of the answer is four waves, and the
tiles are dealt so that workgroup b stays within the eighth of the records that belongs to XCD b % 8."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("probe_sort_plan") / "probe_sort_plan_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(ROOT, "tests", "native", "probe_sort_plan_dump.cpp")], check=True, timeout=600)

    def run(lines):
        r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


N = 1 << 24
OFF = [0, 0, 0, 0, 0, 0, 0]


def _plan(kept=1, alive=0, root=0, lpk=8, stride=16, words=16, n=N, cap_rows=1 << 20, sort=1, sort_min=1 << 24, bucket_kb=1024, scratch_mb=512):
    return "plan %d %d %d %d %d %d %d %d %d %d %d %d" % (kept, alive, root, lpk, stride, words, n, cap_rows, sort, sort_min, bucket_kb, scratch_mb)


# the bench batch: 2^24 k-mers = 4096 chunks = 2^18 tiles, 2^15 tiles per XCD, 2^16 workgroups
BENCH = [4096, 1 << 18, 1 << 15, 1 << 16]

SHIFTS = [
    # 1024 bins (rows of 128 bytes): 2^13 rows per MiB
    (dict(cap_rows=1), [1, 13, 1] + BENCH),
    (dict(cap_rows=1 << 13), [1, 13, 1] + BENCH),
    (dict(cap_rows=(1 << 13) + 1), [1, 13, 2] + BENCH),
    (dict(cap_rows=1 << 20), [1, 13, 128] + BENCH),
    (dict(cap_rows=1 << 21), [1, 13, 256] + BENCH),
    (dict(cap_rows=(1 << 21) + 1), [1, 14, 129] + BENCH),   # 257 buckets: twice as wide
    (dict(cap_rows=1 << 24), [1, 16, 256] + BENCH),
    # 2048 bins (LPK 16, 256 bytes): 2^12 rows
    (dict(lpk=16, stride=32, words=32, cap_rows=1 << 20), [1, 12, 256] + BENCH),
    # the bucket size: 32 KiB = 2^8 rows, 1 KiB = 8 rows, less than a row = one row
    (dict(cap_rows=1 << 16, bucket_kb=32), [1, 8, 256] + BENCH),
    (dict(cap_rows=1 << 10, bucket_kb=1), [1, 3, 128] + BENCH),
    (dict(lpk=16, stride=32, words=32, cap_rows=100, bucket_kb=0), [1, 2, 25] + BENCH),   # (0 is read as 1 KiB: 4 rows)
    # strides that are no power of two have lanes without a chunk (LPK = the next power of two): never sorted
    (dict(lpk=8, stride=12, words=12), OFF),
    (dict(lpk=8, stride=10, words=10), OFF),
    (dict(lpk=16, stride=24, words=24), OFF),
    (dict(lpk=4, stride=6, words=6), OFF),
]


def test_shift_and_buckets(dump):
    got = dump([_plan(**kw) for kw, _ in SHIFTS])
    for (kw, want), g in zip(SHIFTS, got):
        assert g == want, kw


THRESHOLDS = [
    (dict(), 1),
    (dict(n=(1 << 24) - 1), 0), (dict(n=1 << 24), 1),
    (dict(n=99, sort_min=100), 0), (dict(n=100, sort_min=100), 1), (dict(n=1, sort_min=1), 1),
    (dict(n=0, sort_min=1), 0),
    (dict(n=(1 << 32) - 1, scratch_mb=1 << 16), 1), (dict(n=1 << 32, scratch_mb=1 << 16), 0),
    (dict(sort=0), 0),                                   # TXQ_PROBE_SORT=0
    (dict(kept=0), 0),                                   # fresh, or three launches
    (dict(alive=1), 0), (dict(root=1), 0),
    (dict(lpk=16, stride=32, words=32), 1), (dict(lpk=32, stride=64, words=64), 0),
    (dict(words=15), 0),                                 # an odd tail word
    (dict(lpk=8, stride=14, words=13), 0),
    (dict(cap_rows=0), 0),
    # rows narrower than 16 words: the records would be a large part of the masks themselves
    (dict(lpk=4, stride=8, words=8), 0), (dict(lpk=1, stride=2, words=2), 0),
    # the records (8 bytes per k-mer) within TXQ_KMER_TABLE_MB: 128 MiB hold 2^24 of them
    (dict(scratch_mb=128), 1), (dict(scratch_mb=127), 0), (dict(scratch_mb=0), 0),
    (dict(n=1 << 26, scratch_mb=512), 1), (dict(n=(1 << 26) + 1, scratch_mb=512), 0),
]


def test_thresholds(dump):
    got = dump([_plan(**kw) for kw, _ in THRESHOLDS])
    for (kw, want), g in zip(THRESHOLDS, got):
        assert g[0] == want, kw
        if not want:
            assert g == OFF, kw


def test_small_batches(dump):
    # n -> chunks, tiles, tiles per XCD (a multiple of 4), workgroups (a multiple of 8)
    cases = [(1, [1, 1, 4, 8]), (64, [1, 1, 4, 8]), (65, [1, 2, 4, 8]), (4096, [1, 64, 8, 16]), (4097, [2, 65, 12, 24]),
             (3 * 4096 + 17, [4, 193, 28, 56])]
    got = dump([_plan(n=n, sort_min=1) for n, _ in cases])
    for (n, want), g in zip(cases, got):
        assert g[0] == 1 and g[3:] == want, n


@pytest.mark.parametrize("n_tiles", [1, 7, 8, 9, 4 * 8 + 1, 1 << 18])
def test_remap_covers_every_tile_once(dump, n_tiles):
    for n in (64 * n_tiles, 64 * n_tiles - 63):   # a full last tile, a last tile of one k-mer
        tiles, covered, duplicates, out_of_range, other_xcd = dump(["remap %d" % n])[0]
        assert tiles == n_tiles
        assert covered == n_tiles and duplicates == 0
        assert other_xcd == 0
        per_xcd = (-(-n_tiles // 8) + 3) // 4 * 4
        assert out_of_range == 8 * per_xcd - n_tiles
