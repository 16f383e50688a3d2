"""The step logic of the long-pattern edit-distance kernel (csrc/txq_edit_long_plan.hpp) without a GPU:
tests/native/edit_long_sim.cpp, built with the address and undefined-behaviour sanitizers, runs the kernel's systolic schedule
on the CPU — the lanes of a group as an array, the cross-lane move as a shift by one, units and spans cut as the kernel cuts
them — and compares every (distance, record, end) with edit_search_group of host/edit_distance.hpp, which
tests/native/edit_fuzz.cpp holds to the O(mn) table.  Patterns of 1 .. 4096 bytes on either side of every group size and word
count, alphabets of 4 and 20 letters with bytes of no class, groups with empty records at the front, between and at the
end, spans of 16 and 64 bytes and one longer than the text, caps 0, 3, m - 1, m and m + 5.  The program stops at the first
difference with a non-zero exit status."""
import os
import subprocess

from conftest import ROOT


def test_systolic_schedule_matches_host(tmp_path):
    exe = str(tmp_path / "edit_long_sim")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "native", "edit_long_sim.cpp")], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.startswith("edit_long_sim ok: ") and int(r.stdout.split()[2]) > 500, r.stdout
