"""How a (window, view) pair of the window-targets kernel finds its pattern and its text (csrc/txq_edit_window_targets_plan.hpp,
DESIGN.md §22) without a GPU: tests/native/edit_window_targets_sim.cpp, built with the address and undefined-behaviour
sanitizers, runs a call the way txq_edit_window_targets.hip does — the view checks of every pair, units and slots, the two
prefixes, first keys, the lanes of the walk on their chunks with the VIEW's bounds handed to the clipped 16-byte load, flushes,
compaction and rows, all from the plan headers — and compares every hit list and every status word with edit_targets_group of
host/edit_distance.hpp on the window written out, which tests/test_edit_targets_cpu.py holds to the O(mn) table.  Windows of
1, 63, 64, 65, 128, 129, 256, 257 and 512 letters that overlap and end with their buffer, alphabets of 4 and 20 letters with
bytes of no class, a view with empty records at the front, between and at the end and a run of records of 0 .. 3 bytes, a view
whose offsets do not begin at 0, a view of no records, texts at odd addresses in allocations of their exact size, chunks of 16
and 64 bytes and one longer than the text, caps 0, 3, m - 1, m and m + 5, fifteen pairs a call — one of every refusal between
good ones — with exactly the slots they need, one fewer (the last pair that has records refused, and what lies behind it) and
more.  The program stops at the first difference with a non-zero exit status."""
import os
import subprocess

from conftest import ROOT


def test_call_matches_host(tmp_path):
    exe = str(tmp_path / "edit_window_targets_sim")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "native", "edit_window_targets_sim.cpp")], check=True,
                   timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    words = r.stdout.split()
    assert r.stdout.startswith("edit_window_targets_sim ok: ") and int(words[2]) > 400 and int(words[4]) > 10000, r.stdout
