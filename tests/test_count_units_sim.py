"""The unit cut of the flat threshold count (csrc/txq_count_plan.hpp) without a GPU: tests/native/count_units_sim.cpp, built
with the address and undefined-behaviour sanitizers, walks the units of a call as count_flat_kernel does — seg_len, unit_start
at both ends of a unit, query_of at its first value, then query by query, empty ones skipped — and applies the tests of
count_zero_long_kernel and count_finish_kernel.  Every value must be counted by exactly one unit; a query of at most `seg`
values by one unit in one piece (written directly, once); a longer one only ever added to an accumulator that was zeroed; the
finish pass picks exactly the empty and the long queries; `offsets` is a heap block of exactly nq + 1 words.  Offset arrays: no
and one query; all empty; runs of empty queries at a unit's first and last position; seg - 1, seg, seg + 1 and 2 seg in every
order; short queries that begin 0 .. 3 values before a nominal boundary; totals of 8192 * 512 - 1, that, + 1, 8192 * 513 and
4 300 800 values (seg 512, 512, 513, 513, 525) as one query, as short queries and as the edge lengths in turn; 400 random
mixes; each with offsets[0] = 0 and = 1 000 003.  The program stops at the first difference with a non-zero exit status."""
import os
import subprocess

from conftest import ROOT


def test_unit_walk_counts_every_value_once(tmp_path):
    exe = str(tmp_path / "count_units_sim")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "native", "count_units_sim.cpp")], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    words = r.stdout.split()
    # 2 x (15 hand-picked + 48 edge orders + 60 before-a-boundary + 2 + 15 totals + 400 random) cases.  The 15 totals alone
    # make about 2 x 3 x 5 x 8190 units, of which those past the 4096th are a workgroup's second item; long queries: 2 in every
    # edge order and more.
    assert r.stdout.startswith("count_units_sim ok: ") and int(words[2]) == 2 * 540, r.stdout
    assert int(words[6]) > 200_000 and int(words[8]) > 2 * 96 and int(words[10]) > 100_000, r.stdout
