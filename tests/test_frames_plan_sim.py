"""The address arithmetic of txq_translate_frames_device (csrc/txq_frames_plan.hpp) without a GPU:
tests/native/frames_plan_sim.cpp, built with the address and undefined-behaviour sanitizers, walks records as frames_kernel's
units and steps do — every length 0 .. 40, lengths around one and two units and around a step, a record of 20 011 bytes that
spans many units, empty records between them, ambiguous bytes and lower case mixed in, the batch at byte 0 and at byte 5 of
its buffer — and stores the six runs of every step through store_block into a guarded buffer at every alignment 0 .. 15, at
the full capacity, at about half of it and at 0.  Every store must be aligned to its width and lie inside the frames and
below the capacity, no byte may be stored twice, every frame byte below the capacity is stored, nothing around the frames
changes, and the bytes equal translate_frame of host/encoder.cpp.  The program stops at the first difference with a non-zero
exit status."""
import os
import subprocess

from conftest import ROOT


def test_frames_plan_writes_every_frame_byte_once(tmp_path):
    exe = str(tmp_path / "frames_plan_sim")
    subprocess.run(["g++", "-std=c++20", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "native", "frames_plan_sim.cpp"),
                    os.path.join(ROOT, "tetrex_amd", "csrc", "host", "encoder.cpp")], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    words = r.stdout.split()
    assert r.stdout.startswith("frames_plan_sim ok: ") and int(words[2]) > 50000 and int(words[4]) > 1000000, r.stdout
