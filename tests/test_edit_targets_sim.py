"""The slot arithmetic and the flush rule of the per-record edit-distance kernels (csrc/txq_edit_targets_plan.hpp) without a
GPU: tests/native/edit_targets_sim.cpp, built with the address and undefined-behaviour sanitizers, runs the lane schedules of
both kernels on the CPU — the short kernel's lanes on their chunks, the long kernel's lane groups with the cross-lane move as
a shift by one, units, chunks and spans cut as the kernels cut them — with slots, first keys, flushes and rows taken from the
plan header, and compares every hit list with edit_targets_group of host/edit_distance.hpp, which
tests/test_edit_targets_cpu.py holds to the O(mn) table.  Patterns of 1 .. 4096 bytes on either side of every word count and
group size, alphabets of 4 and 20 letters with bytes of no class, groups with empty records at the front, between and at the
end and a run of records of 0 .. 3 bytes, chunks and spans of 16 and 64 bytes and one longer than the text, caps 0, 3, m - 1, m
and m + 5, two pairs a call with exactly the slots they need, one fewer (the second pair refused) and more.  The program
stops at the first difference with a non-zero exit status."""
import os
import subprocess

from conftest import ROOT


def test_lane_schedules_match_host(tmp_path):
    exe = str(tmp_path / "edit_targets_sim")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "native", "edit_targets_sim.cpp")], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    words = r.stdout.split()
    assert r.stdout.startswith("edit_targets_sim ok: ") and int(words[2]) > 500 and int(words[4]) > 5000, r.stdout
