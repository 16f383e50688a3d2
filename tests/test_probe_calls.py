"""Sequences of flat-probe calls on one domain table without a GPU (tests/native/probe_calls_sim.cpp, built with the address and
undefined-behaviour sanitizers): the three call shapes of DESIGN.md "Domain table" - fresh (sample, build, answer), kept in one
launch, kept in three launches (TXQ_PROBE_TABLE_FUSED=0) - played with the functions of csrc/txq_probe_plan.hpp in the order
probe_flat and its kernels use them, on a model of the table ("row v written since the last fresh call") and of the state words.
The program checks on every call that each row read from the table was written by an EARLIER call, that the statistics slot
the call adds into starts at zero, that "add", "read" and "zero" are three slots and the valid-rows word read is not the one
written, and that no state word is read and written by one launch.  The extension rule's cases below are worked by hand."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("probe_calls") / "probe_calls_sim")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(ROOT, "tests", "native", "probe_calls_sim.cpp")], check=True, timeout=600)

    def run(lines):
        r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


# valid, top, count, ratio, cap_rows -> V, E
EXTEND = [
    ((1000, 3000, 8000, 4, 17472), (1000, 3000)),      # equality at the gate: 8000 = 4 * (3000 - 1000)
    ((1000, 3000, 7999, 4, 17472), (1000, 1000)),      # one k-mer short: the extension does not pay
    ((1000, 3000, 12000, 4, 17472), (1000, 3000)),     # (the gate is over the NEW rows, not over top: 12000 = 4 * 3000 too)
    ((1000, 1001, 0, 0, 17472), (1000, 1001)),         # ratio 0 (TXQ_PROBE_TABLE=1): whenever top > V
    ((1000, 1000, 0, 0, 17472), (1000, 1000)),
    ((3000, 3000, 99999, 4, 17472), (3000, 3000)),     # top <= V: nothing to build
    ((3000, 2999, 99999, 4, 17472), (3000, 3000)),
    ((3000, 0, 0, 4, 17472), (3000, 3000)),            # the call before gathered nothing below its capacity
    ((0, 64, 256, 4, 17472), (0, 64)),                 # the first rows
    ((1000, 20000, 1 << 30, 4, 17472), (1000, 1000)),  # a top beyond the table (it never is): not believed, E <= cap_rows
    ((1000, 17472, 1 << 30, 4, 17472), (1000, 17472)),  # the whole table
    ((20000, 100, 5, 4, 17472), (17472, 17472)),       # `valid` beyond the table (it never is): clamped
    ((17472, 17472, 5, 4, 17472), (17472, 17472)),
    ((0, 1 << 30, 1000, 4, 1 << 31), (0, 0)),          # ratio * (top - V) = 2^32: zero in 32 bits, which would pass
    ((0, 1 << 30, (1 << 32) - 1, 4, 1 << 31), (0, 0)),  # ... and the largest count there is stays below 2^32
    ((0, (1 << 30) - 1, (1 << 32) - 4, 4, 1 << 31), (0, (1 << 30) - 1)),  # equality just below 2^32
    ((5, (1 << 30) + 5, (1 << 32) - 1, 4, 1 << 31), (5, 5)),  # (top - V) itself is what is multiplied
    ((0, (1 << 32) - 1, (1 << 32) - 1, 1, (1 << 32) - 1), (0, (1 << 32) - 1)),  # count * 1 at the top of 32 bits
]


def test_extension_rule(sim):
    out = sim(["ext " + " ".join(str(x) for x in args) for args, _ in EXTEND])
    for (args, want), got in zip(EXTEND, out):
        assert tuple(int(x) for x in got.split()) == want, args


def test_slot_rotation(sim):
    """Call c + 1 reads as V the word call c stored, reads the statistics call c added into, adds into the slot call c zeroed,
    and samples into the accumulator call c zeroed; within a call the three statistics slots and the two valid-rows words differ."""
    numbers = list(range(8)) + [(1 << 40) + i for i in range(7)] + [(1 << 64) - 2]
    calls = [c for n in numbers for c in (n, n + 1)]
    out = [tuple(int(x) for x in l.split()) for l in sim(["slots %d" % c for c in calls])]
    for i in range(0, len(out), 2):
        acc, acc_zero, v_read, v_write, s_add, s_read, s_zero = out[i]
        acc1, _, v_read1, _, s_add1, s_read1, _ = out[i + 1]
        assert len({s_add, s_read, s_zero}) == 3 and v_read != v_write and acc != acc_zero, calls[i]
        assert (acc1, v_read1, s_add1, s_read1) == (acc_zero, v_write, s_zero, s_add), calls[i]
        words = [acc, acc + 1, acc_zero, acc_zero + 1, v_read, v_write, s_add, s_add + 1, s_read, s_read + 1, s_zero, s_zero + 1]
        assert sorted(words) == list(range(12)), calls[i]  # every state word has one meaning per call
    assert out[0] == (0, 2, 4, 5, 6, 10, 8)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_sequences_of_calls(sim, seed):
    # fresh, kept, failed launches, generation changes and growth mixed; FUSED and KEEP switched within a sequence
    assert sim(["sim %d 1000 12" % seed]) == ["ok 1000"]


def test_long_sequences_of_calls(sim):
    assert sim(["sim 7 100 200"]) == ["ok 100"]


def test_steady_batch_settles_within_three_calls(sim):
    assert sim(["steady 11 2000"]) == ["ok 2000"]
