"""The window pass of txq_translate_windows_device (csrc/txq_frame_windows_plan.hpp) without a GPU:
tests/native/frame_windows_sim.cpp, built with the address and undefined-behaviour sanitizers, walks records as
translate_windows_kernel's units and steps of kTile start positions do — the count pass that leaves the units' tails, the fill
pass in which the lane of a start position holds the rank of its k-mer position in its forward and in its reverse frame and
stores it into the window slots codon_slots names, window_finish_kernel — and compares every window's (begin, len) with a
brute-force count over translate_frame's letters, the windows cut by a restatement of `tetrex search --window`.  Every slot
must be written exactly once, the end slot of a frame's last window by the finishing pass alone.  k = 1, 6, 12; ten (W, S)
shapes each, with S = 1, S = W and steps that do not divide R - W; frames of R = k - 1, k, W - 1, W, W + 1, W + S - 1, W + S,
W + S + 1 and W + 3 S + 2 residues at each of the three offsets; stops at the first and the last codon, on the windows'
boundaries, in every k-mer of one window and of all (len 0); a record across three units with and without stops; 300 records
of 30 to 60 bytes inside one unit; empty records; the batch at byte 0 and at byte 5 of its buffer.  The program stops at the
first difference with a non-zero exit status."""
import os
import subprocess

from conftest import ROOT


def test_every_window_slot_written_once_and_equal_to_brute_force(tmp_path):
    exe = str(tmp_path / "frame_windows_sim")
    subprocess.run(["g++", "-std=c++20", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "native", "frame_windows_sim.cpp"),
                    os.path.join(ROOT, "tetrex_amd", "csrc", "host", "encoder.cpp")], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    words = r.stdout.split()
    # 3 k x 10 shapes x 2 buffer positions; the long records alone give thousands of windows a batch, and the wrong frames and
    # the planted stops leave many of them empty
    assert r.stdout.startswith("frame_windows_sim ok: ") and int(words[2]) == 60 and int(words[4]) > 300000 and int(words[6]) > 10000, r.stdout
