"""The sliding window count on an HIBF (csrc/txq_count_windows_tree_plan.hpp) without a GPU: tests/native/count_windows_tree_sim.cpp,
built with the address and undefined-behaviour sanitizers, descends a synthetic tree of 3 levels (merged bins, user bins, runs
of split bins, a user bin in two runs) level by level as count_windows_tree_kernel does — work items (unit, IBF, mask), the
walk over an item's visited windows with cw_step between two that need not be neighbours, a mask word per merged bin, the
children's items — with the plan header's functions only, and compares every (window, IBF) count vector, every child's visit
set, the user bins' hits and counts and the added and subtracted totals with an independent recount and descent of every
window on its own.  Units of 1, 2, 3, 16, 32 and 64 (clipped to 32) windows; the window sets of count_windows_sim.cpp;
thresholds of about half the length, some 0 and some above the length; counters poisoned before the first item and never
cleaned between items; one device call, a single unit per call and two units per call, with frontier buffers of exactly the
planned size; the call-cut formula at its edges.  The program stops at the first difference with a non-zero exit status."""
import os
import subprocess

from conftest import ROOT


def test_tree_walk_matches_independent_descent(tmp_path):
    exe = str(tmp_path / "count_windows_tree_sim")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "native", "count_windows_tree_sim.cpp")], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    words = r.stdout.split()
    # 103 window sets x (6 unit sizes in one call + 5 unit sizes x 2 call cuts) = 1648 cases; the walk must slide, and slide
    # across windows that did not visit the IBF (those happen only below the root)
    assert r.stdout.startswith("count_windows_tree_sim ok: ") and int(words[2]) == 103 * 16 and int(words[4]) > 100000, r.stdout
    assert int(words[6]) > 20000 and int(words[8]) > 1000, r.stdout
