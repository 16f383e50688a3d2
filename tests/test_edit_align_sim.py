"""The step logic of the alignment kernel (csrc/txq_edit_align_plan.hpp) without a GPU: tests/native/edit_align_sim.cpp, built
with the address and undefined-behaviour sanitizers, runs the kernel's lane schedule on the CPU — the 64 lanes as arrays, a
cross-lane move as an index, a ballot as a loop, rows in blocks of 64 with the block's bytes fetched as the kernel fetches them, the
walk back over the direction words — and compares every word of every answer with edit_align_pair of host/edit_distance.hpp,
which tests/test_edit_align_cpu.py holds to the full matrix.  Patterns of 1 .. 4097 bytes on either side of 64, 512 and 4096,
distances 0, 1, 2, 5, 31 and the declined 32 and 33, copies at the start of a record (the window clipped), inside and at its
end, alphabets of 4 and 20 letters with bytes of no class, triples that are no cell of the matrix.  The program stops at the
first difference with a non-zero exit status."""
import os
import subprocess

from conftest import ROOT


def test_lane_schedule_matches_host_twin(tmp_path):
    exe = str(tmp_path / "edit_align_sim")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "native", "edit_align_sim.cpp")], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.startswith("edit_align_sim ok: ") and int(r.stdout.split()[2]) > 5000, r.stdout
