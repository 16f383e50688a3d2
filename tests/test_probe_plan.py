"""The host's half of the flat probe's domain table (csrc/txq_probe_plan.hpp) without a GPU: tests/native/probe_plan_dump.cpp,
built with the address and undefined-behaviour sanitizers, answers one command per line.  The expected values below are worked
out by hand from the rules in DESIGN.md "Domain table": the capacity a call may ask for, the rows [lo, rows) a call builds and
reads (the arithmetic both kernels share), and whether a call keeps the table's rows or starts them over."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("probe_plan") / "probe_plan_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(ROOT, "tests", "native", "probe_plan_dump.cpp")], check=True, timeout=600)

    def run(lines):
        r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


# probe_table (TXQ_PROBE_TABLE: -1 unset), table_mb, bin_size, stride, hash_funs, n -> rows
CAPACITY = [
    ((-1, 512, 4099, 16, 3, 70000), 17472),        # n / 4 = 17500, down to a multiple of 64
    ((-1, 512, 4099, 16, 3, 65535), 0),            # 16383 -> 16320 rows: below 2^14, the plain kernel
    ((-1, 512, 4099, 16, 3, 65536), 16384),        # the smallest n that reaches the automatic gate
    ((-1, 512, 1247045, 16, 3, 1 << 24), 1 << 22),  # the bench batch: n / 4 = the budget of 512 MiB / 128 B
    ((-1, 512, 1247045, 16, 3, 1 << 26), 1 << 22),  # the budget bounds it
    ((-1, 1, 4099, 16, 3, 70000), 0),              # a budget of 8192 rows is below 2^14
    ((1, 512, 4099, 16, 3, 100), 65536),           # =1: at least 2^16 rows, whatever n
    ((1, 512, 4099, 16, 3, 100000), 99968),
    ((1, 1, 4099, 4, 3, 70000), 32768),            # =1 takes whatever the budget gives: 1 MiB / 32 B
    ((0, 512, 4099, 16, 3, 70000), 0),             # =0
    ((-1, 0, 4099, 16, 3, 70000), 0),              # TXQ_KMER_TABLE_MB=0
    ((-1, 512, 4099, 1, 3, 70000), 0),             # one word per row: probe_w1_kernel
    ((-1, 512, 4099, 3, 3, 70000), 0),             # (an odd stride does not exist; refused all the same)
    ((-1, 512, 4099, 16, 1, 70000), 0),            # h = 1: a table row would be the IBF's own row
    ((-1, 512, 1 << 32, 16, 3, 70000), 0),         # rows >= 2^32: the big-rows kernel
]

# fresh, built, top, count, ratio, sample, cap_rows -> lo, rows
ROWS = [
    ((1, 999, 1024, 4375, 4, 16, 17472), (0, 1024)),        # fresh: `built` is not believed
    ((0, 1024, 4096, 4375, 4, 16, 17472), (1024, 4096)),    # an extension
    ((0, 4096, 16000, 4375, 4, 16, 17472), (4096, 16000)),
    ((0, 16000, 512, 4375, 4, 16, 17472), (16000, 16000)),  # lo > top: nothing to build, every row stays readable
    ((0, 4096, 0, 0, 4, 16, 17472), (4096, 4096)),          # no value below the capacity: the rows stay
    ((1, 4096, 0, 0, 4, 16, 17472), (0, 0)),
    ((0, 100, 10000, 2499, 4, 16, 17472), (100, 100)),      # 2499 * 16 < 4 * 10000: the domain does not pay, no extension
    ((0, 100, 10000, 2500, 4, 16, 17472), (100, 10000)),    # ... and at equality it does
    ((1, 100, 10000, 2499, 4, 16, 17472), (0, 0)),          # fresh and refused: no row is read
    ((0, 0, 5, 0, 0, 16, 65536), (0, 5)),                   # ratio 0 (TXQ_PROBE_TABLE=1): whenever D != 0
    ((0, 0, 1000, 1 << 28, 4, 16, 1 << 22), (0, 1000)),     # count * sample = 2^32: zero in 32 bits
    ((0, 0, 1 << 30, 1000, 4, 16, 1 << 31), (0, 0)),        # ratio * D = 2^32: zero in 32 bits, which would pass
    ((0, 20000, 100, 4375, 4, 16, 17472), (17472, 17472)),  # `built` beyond the table (it never is): clamped
    ((0, 0, 20000, 4375, 4, 16, 17472), (0, 0)),            # a D beyond the table (it never is): not believed
    ((0, 17472, 17472, 4375, 4, 16, 17472), (17472, 17472)),  # the whole table is built
]

# one table's history: (index generation, table just (re)allocated, TXQ_PROBE_TABLE_KEEP) -> fresh, zero_state, parity
HISTORY = [
    ("call 0 1 1", (1, 1, 0)),  # first call: new memory
    ("call 0 0 1", (0, 0, 1)),  # steady state
    ("call 0 0 1", (0, 0, 0)),
    ("call 1 0 1", (1, 0, 1)),  # txq_emplace_device came between
    ("call 1 0 1", (0, 0, 0)),
    ("call 1 0 0", (1, 0, 1)),  # TXQ_PROBE_TABLE_KEEP=0
    ("call 1 0 1", (0, 0, 0)),  # ... leaves valid rows behind
    ("call 1 1 1", (1, 0, 1)),  # growth
    ("call 3 0 1", (1, 0, 0)),  # two emplace calls
    ("call 3 0 1", (0, 0, 1)),
    ("fail", None),             # the launches of a call failed: the state words may be anything
    ("call 3 0 1", (1, 1, 0)),
    ("call 3 0 1", (0, 0, 1)),
    ("call 3 1 0", (1, 0, 0)),
    ("call 4 1 0", (1, 0, 1)),
]


def test_table_capacity(dump):
    out = dump(["cap " + " ".join(str(x) for x in args) for args, _ in CAPACITY])
    for (args, want), got in zip(CAPACITY, out):
        assert int(got) == want, args


def test_table_rows(dump):
    out = dump(["rows " + " ".join(str(x) for x in args) for args, _ in ROWS])
    for (args, want), got in zip(ROWS, out):
        assert tuple(int(x) for x in got.split()) == want, args


def test_the_answers_store_of_built_is_idempotent(dump):
    """The answer kernel's waves read `built` while one thread stores rows into it: with either value they compute the same rows."""
    lines = []
    for args, (_, rows) in ROWS:
        lines.append("rows " + " ".join(str(x) for x in (args[0], rows) + args[2:]))
    out = dump(lines)
    for (args, (_, rows)), got in zip(ROWS, out):
        assert int(got.split()[1]) == rows, args


def test_fresh_or_keep_over_a_history_of_calls(dump):
    out = dump([cmd for cmd, _ in HISTORY])
    for i, ((cmd, want), got) in enumerate(zip(HISTORY, out)):
        if want is None:
            assert got == "failed"
        else:
            assert tuple(int(x) for x in got.split()) == want, (i, cmd)


def test_two_tables_do_not_share_their_history(dump):
    # (a second process = a second table: its first call is fresh whatever the other has seen)
    assert dump(["call 7 0 1"]) == ["1 1 0"]
    assert dump(["call 7 0 1", "call 7 0 1"]) == ["1 1 0", "0 0 1"]
