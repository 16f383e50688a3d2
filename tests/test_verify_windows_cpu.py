"""`tetrex search --window --verify-windows` without a GPU: the merge of confirmed windows into rows —
plan::confirmed_runs of csrc/host/search_plan.hpp, printed by tests/native/verify_windows_dump.cpp under sanitizers, against
the Python restatement tests/verify_windows_ref.py (which tests/test_gpu_search_verify_windows.py holds the command to) — and
the refusals the command makes while it parses its options, before it reads an index or touches a device."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from search_window_ref import windows_of
from verify_windows_ref import merge_confirmed, revcomp

TETREX = os.path.join(ROOT, "bin", "tetrex")
K = 6


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("verify_windows") / "verify_windows_dump")
    subprocess.run(["g++", "-std=c++20", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(ROOT, "tests", "native", "verify_windows_dump.cpp")], check=True, timeout=600)

    def run(per_bin):
        """per_bin: {bin: {window: (count, distance, strand)}} -> [(bin, strand, first, last, best, nearest)] in row order"""
        lines = ["%d %d %d %d %s\n" % (j, u, c, d, s) for u in per_bin for j, (c, d, s) in per_bin[u].items()]
        r = subprocess.run([exe], input="".join(reversed(lines)), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        return [(int(f[0]), f[1], int(f[2]), int(f[3]), int(f[4]), int(f[5])) for f in (line.split() for line in r.stdout.splitlines())]
    return run


def ref_rows(wins, per_bin, with_strand):
    """the same through merge_confirmed: [(bin, begin, end, count/w, distance, target, end[, strand])], the target naming the
    window the distance came from"""
    out = []
    for u in sorted(per_bin):
        conf = {j: (c, d, "w%d" % j, 100 + j, s if with_strand else "") for j, (c, d, s) in per_bin[u].items()}
        out += [(u,) + row for row in merge_confirmed(wins, K, conf, True)]
    return out


def as_rows(wins, runs, per_bin, with_strand):
    out = []
    for u, s, first, last, best, near in runs:
        row = (u, wins[first][0] + 1, wins[last][0] + wins[last][1], "%d/%d" % (per_bin[u][best][0], wins[best][1] - K + 1),
               per_bin[u][near][1], "w%d" % near, 100 + near)
        out.append(row + ((s,) if with_strand else ()))
    return out


CASES = {
    "one window": {0: {2: (50, 1, "+")}},
    "a whole record": {0: {j: (50, 2, "+") for j in range(10)}},
    "split by a gap": {0: {0: (50, 1, "+"), 1: (51, 0, "+"), 3: (49, 2, "+"), 4: (55, 2, "+")}},
    "split by a bin": {0: {0: (50, 1, "+"), 1: (51, 0, "+")}, 3: {2: (49, 2, "+"), 3: (55, 2, "+")}, 1: {1: (40, 0, "+")}},
    "split by a strand": {0: {0: (50, 1, "+"), 1: (51, 0, "-"), 2: (49, 2, "-"), 3: (55, 2, "+"), 4: (55, 1, "+")}},
    "strands interleaved": {0: {0: (50, 1, "-"), 1: (51, 0, "+"), 2: (49, 2, "-"), 3: (55, 2, "+"), 5: (55, 1, "-"), 6: (1, 1, "+")}},
    "ties in distance": {0: {1: (40, 2, "+"), 2: (44, 1, "+"), 3: (44, 1, "+"), 4: (45, 3, "+")}},
    "ties in count": {0: {4: (41, 2, "+"), 2: (41, 2, "+"), 3: (40, 2, "+")}},
    "best and nearest differ": {2: {5: (55, 2, "+"), 6: (30, 0, "+"), 7: (54, 1, "+")}},
}


@pytest.mark.parametrize("case", list(CASES))
def test_run_merge_matches_restatement(dump, case):
    wins = windows_of(195, K, 60, 15)  # offsets 0, 15, ..., 135
    assert len(wins) == 10
    per_bin = CASES[case]
    for with_strand in (True, False):
        if not with_strand:  # one strand: every window on +
            per_bin = {u: {j: (c, d, "+") for j, (c, d, _) in w.items()} for u, w in per_bin.items()}
        got = as_rows(wins, dump(per_bin), per_bin, with_strand)
        assert got == ref_rows(wins, per_bin, with_strand), (case, with_strand)
        assert got == sorted(got, key=lambda r: (r[0], r[1])), "rows by bin, then begin"


def test_run_merge_by_hand():
    wins = windows_of(195, K, 60, 15)
    c = lambda count, d, s="": (count, d, "t", 7 + d, s)
    # a run broken by one unconfirmed window: two rows, though their letters overlap
    assert merge_confirmed(wins, K, {0: c(50, 1), 1: c(51, 0), 3: c(49, 2), 4: c(55, 2)}) == [(1, 75, 0, "t", 7), (46, 120, 2, "t", 9)]
    assert merge_confirmed(wins, K, {0: c(50, 1), 1: c(51, 0), 3: c(49, 2), 4: c(55, 2)}, True) == [(1, 75, "51/55", 0, "t", 7), (46, 120, "55/55", 2, "t", 9)]
    # two strands: runs of a strand only; a - run between two + runs; + before - where they begin together (they cannot: one strand a window)
    rows = merge_confirmed(wins, K, {0: c(1, 1, "+"), 1: c(1, 0, "-"), 2: c(1, 2, "-"), 3: c(1, 2, "+")})
    assert rows == [(1, 60, 1, "t", 8, "+"), (16, 90, 0, "t", 7, "-"), (46, 105, 2, "t", 9, "+")]
    # the earliest of equal distances, not the first seen
    conf = {3: (9, 1, "late", 5, ""), 2: (9, 1, "early", 4, ""), 1: (9, 2, "far", 3, "")}
    assert merge_confirmed(wins, K, conf) == [(16, 105, 1, "early", 4)]
    assert merge_confirmed(wins, K, {}) == []


def test_reverse_complement():
    assert revcomp("ACGTU") == "AACGT" and revcomp("acgn-x") == "NNNCGT" and revcomp("") == ""
    rng = np.random.default_rng(3)
    s = "".join(rng.choice(list("ACGT"), size=50))
    assert revcomp(revcomp(s)) == s


REFUSALS = [
    (["--verify-windows", "-e", "1"], "--window"),
    (["--window", "60", "--verify-windows"], "-e E"),
    (["--window", "60", "--threshold", "0.5", "--verify-windows"], "--threshold"),
    (["--window", "60", "-e", "1", "--verify-windows", "--translate"], "--translate"),
    (["--translate", "--frame-window", "30", "-e", "1", "--verify-windows"], "--frame-window cannot be combined with --verify-windows"),
    (["--window", "60", "-e", "1", "--verify-windows", "--verify"], "--verify-windows cannot be combined with --verify:"),
    (["--window", "60", "-e", "1", "--verify-windows", "--verify-frames"], "--verify-frames"),
    (["--window", "60", "-e", "1", "--verify-windows", "--align"], "--align"),
    (["--window", "60", "-e", "1", "--verify-windows", "--all-targets"], "--all-targets"),
    (["--window", "60", "-e", "1", "--verify"], "--verify-windows"),  # the old refusal points to the new flag
    (["--window", "0", "-e", "1", "--verify-windows"], "--window must be"),
    (["--window", "60", "--step", "61", "-e", "1", "--verify-windows"], "--step must be"),
]


@pytest.mark.parametrize("flags,word", REFUSALS, ids=[" ".join(f) for f, _ in REFUSALS])
def test_cli_refuses_at_parse_time(tmp_path, flags, word):
    """None of these reaches the index file (which does not exist) or a device."""
    out = tmp_path / "out.tsv"
    r = subprocess.run([TETREX, "search"] + flags + ["-o", str(out), str(tmp_path / "none.ibf"), str(tmp_path / "none.fa")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0, r.stderr
    assert r.stderr.startswith("[Search Parser Error] ") and word in r.stderr, r.stderr
    assert r.stdout == "" and not out.exists()


def test_the_flag_parses(tmp_path):
    """with every option it needs, the command gets as far as the index file"""
    r = subprocess.run([TETREX, "search", "--window", "60", "--step", "15", "-e", "1", "--verify-windows", "--counts", str(tmp_path / "none.ibf"), str(tmp_path / "none.fa")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Parser Error" not in r.stderr and "Index not valid" in r.stderr, r.stderr
