"""The unit cut and the entering and leaving ranges of the sliding window count (csrc/txq_count_windows_plan.hpp) without a
GPU: tests/native/count_windows_sim.cpp, built with the address and undefined-behaviour sanitizers, walks units and windows as
count_windows_kernel does — the first window of a unit in full, every next one by adding the values that enter and subtracting
those that leave, the counters zeroed where the windows do not overlap — over a synthetic membership bit per (value, bin), and
compares every window's counts with a recount from nothing.  Units of 1, 2, 3, 16 and 64 windows; windows of 0, 1, 63, 64, 65
and 300 values at steps 1, 7, the length (touching) and the length + 5 (gaps); a length that shrinks, then grows; the
end-aligned tail window of `tetrex search --window`; repeated windows; empty windows in gaps; 0, 1, 37 and 130 windows (no
multiple of the larger units).  The program stops at the first difference with a non-zero exit status."""
import os
import subprocess

from conftest import ROOT


def test_sliding_walk_matches_recount(tmp_path):
    exe = str(tmp_path / "count_windows_sim")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "native", "count_windows_sim.cpp")], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    words = r.stdout.split()
    # 103 window sets x 5 unit sizes.  Slid windows: the 8 sets of 130 and of 37 windows of 63 .. 300 values at steps 1 and 7 alone
    # slide every window that does not open a unit: 8 * ((65 + 86 + 121 + 127) + (18 + 24 + 34 + 36)) = 4088.
    assert r.stdout.startswith("count_windows_sim ok: ") and int(words[2]) >= 500 and int(words[4]) > 20000 and int(words[6]) >= 4088, r.stdout
