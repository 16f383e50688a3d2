"""The window form of the alignment kernel (csrc/txq_edit_align_plan.hpp: align_window_ok, align_window_kind)
without a GPU: tests/native/edit_align_windows_sim.cpp, built with the address and undefined-behaviour sanitizers, answers pairs
(window, view, cap) as a wave of the kernel does — the admission of the window and of the triple inside its view, then the lane
schedule — over one letter buffer and a table of three views (one record; seven records with empty ones in front of the target
and a match clipped at byte 0 of the text; no records), and compares every word with edit_align_pair on the window written out.
Windows of 1 .. 700 letters on either side of 64 and of the 512 the instance holds, windows that overlap in all but one letter,
in descending order, repeated, one ending at the buffer's last byte; every refusal and every decline of include/txq.h at
txq_edit_align_windows_device, with guard words around the answers and exact-size arrays.  The program stops at the first
difference with a non-zero exit status."""
import os
import subprocess

from conftest import ROOT


def test_window_admission_and_lane_schedule_match_host_twin(tmp_path):
    exe = str(tmp_path / "edit_align_windows_sim")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "native", "edit_align_windows_sim.cpp")], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.startswith("edit_align_windows_sim ok: ") and int(r.stdout.split()[2]) > 5000, r.stdout
