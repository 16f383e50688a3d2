"""The bundles of the windowed edit-distance kernel (csrc/txq_edit_windows_plan.hpp) without a GPU:
tests/native/edit_windows_sim.cpp, built with the address and undefined-behaviour sanitizers, walks pair lists the way
txq_edit_windows.hip does — the plan kernel's heads and unit counts, pair_of_unit over their prefix, the bundle's extent, the
lanes' chunks, the shared lead-in, K states stepped per byte — and compares every (distance, record, end) with
edit_search_group of host/edit_distance.hpp on the written-out window.  Windows of 1 .. 512 letters on either side of every
word count, overlapping and at the last byte of the letter buffer; runs that begin at every i % K and are broken by group
changes, refused pairs, groups of no records and of empty records; caps 0, 3, m - 1, m, m + 5; chunks of 16, 64 and 512 bytes;
bundles of 1, 2 and 4; a text that is not 16-byte aligned.  It asserts that every pair is in exactly one bundle and stops at
the first difference with a non-zero exit status."""
import os
import subprocess

from conftest import ROOT


def test_bundled_walk_matches_host(tmp_path):
    exe = str(tmp_path / "edit_windows_sim")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "native", "edit_windows_sim.cpp")], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    words = r.stdout.split()
    assert r.stdout.startswith("edit_windows_sim ok: ") and int(words[2]) > 5000 and int(words[4]) < int(words[2]), r.stdout
