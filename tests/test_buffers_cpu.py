"""The owners of libtxq's device memory (tetrex_amd/csrc/txq_buffers.hpp) without a GPU: tests/native/buffers_sim.cpp
instantiates the header with a counting allocator that can fail on the n-th call, and is built with the address and
undefined-behaviour sanitizers.  Each case of the program checks itself and prints its counts; this file runs it and holds
the counts to what the cases must leave behind: nothing live, nothing freed twice."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CASES = ["keeps", "growth", "outgrown", "failure", "moves", "session"]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("buffers") / "buffers_sim")
    subprocess.run(["g++", "-std=c++20", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(ROOT, "tests", "native", "buffers_sim.cpp")], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return r


def test_every_case_holds_and_the_sanitizers_are_silent(sim):
    assert sim.returncode == 0, (sim.stdout[-3000:], sim.stderr[-3000:])
    assert "FAILED" not in sim.stdout and sim.stdout.splitlines()[-1] == "ok"
    assert sim.stderr == ""


@pytest.mark.parametrize("case", CASES)
def test_nothing_is_left_and_nothing_is_freed_twice(sim, case):
    m = re.search(r"^%s: (\d+) allocations, (\d+) frees, (\d+) live, (\d+) double frees$" % case, sim.stdout, re.M)
    assert m, sim.stdout
    allocations, frees, live, double = map(int, m.groups())
    assert live == 0 and double == 0
    assert frees <= allocations  # (an allocation that was told to fail is counted, and never freed)
    assert allocations > 0


def test_handles_are_destroyed_once(sim):
    assert re.search(r"^handles: 2 destroyed$", sim.stdout, re.M), sim.stdout
