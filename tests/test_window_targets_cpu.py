"""`tetrex search ... --verify-windows --window-targets` without a GPU: the merge of target hits into rows —
plan::target_runs of csrc/host/search_plan.hpp, printed by tests/native/window_targets_dump.cpp under sanitizers, against the
Python restatement tests/window_targets_ref.py (which tests/test_gpu_search_window_targets.py holds the command to) —, the
restatement by hand, and what the command decides while it parses its options, before it reads an index or touches a device:
the new flag's refusals, the old refusals of --all-targets next to the window modes, which now name the new flag, and the flag
accepted by both windowed commands up to the missing index file."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from search_window_ref import windows_of
from window_targets_ref import merge_targets, nearest_of, union_of

TETREX = os.path.join(ROOT, "bin", "tetrex")
K = 6


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("window_targets") / "window_targets_dump")
    subprocess.run(["g++", "-std=c++20", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(ROOT, "tests", "native", "window_targets_dump.cpp")], check=True, timeout=600)

    def run(per_bin):
        """per_bin: {bin: {(window, target): (count, distance, strand)}} -> [(bin, target, strand, first, last, best, nearest)] in row order"""
        lines = ["%d %d %d %d %d %s\n" % (j, u, t, c, d, s) for u in per_bin for (j, t), (c, d, s) in per_bin[u].items()]
        r = subprocess.run([exe], input="".join(reversed(lines)), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        return [(int(f[0]), int(f[1]), f[2], int(f[3]), int(f[4]), int(f[5]), int(f[6])) for f in (line.split() for line in r.stdout.splitlines())]
    return run


def ref_rows(wins, per_bin, with_strand):
    """the same through merge_targets: [(bin, begin, end, count/w, distance, target, end[, strand])], the target end naming the
    window the distance came from"""
    out = []
    for u in sorted(per_bin):
        hits = {(j, t): (c, d, "t%d" % t, 100 + j, s if with_strand else "") for (j, t), (c, d, s) in per_bin[u].items()}
        out += [(u,) + row for row in merge_targets(wins, K, hits, True)]
    return out


def as_rows(wins, runs, per_bin, with_strand):
    out = []
    for u, t, s, first, last, best, near in runs:
        row = (u, wins[first][0] + 1, wins[last][0] + wins[last][1], "%d/%d" % (per_bin[u][best, t][0], wins[best][1] - K + 1),
               per_bin[u][near, t][1], "t%d" % t, 100 + near)
        out.append(row + ((s,) if with_strand else ()))
    return out


CASES = {
    "one hit": {0: {(2, 0): (50, 1, "+")}},
    "one target, a whole record": {0: {(j, 1): (50, 2, "+") for j in range(10)}},
    "two targets, the same windows": {0: {(j, t): (50 + j, t, "+") for j in range(3, 7) for t in (0, 2)}},
    "a second target on a longer and a shifted stretch": {0: dict([((j, 0), (50, 1, "+")) for j in range(2, 5)] + [((j, 3), (50, 2, "+")) for j in range(1, 8)] +
                                                           [((j, 1), (50, 0, "+")) for j in range(4, 6)])},
    "a later target only": {0: {(0, 0): (50, 1, "+"), (1, 0): (50, 1, "+"), (2, 4): (50, 0, "+"), (3, 4): (50, 2, "+")}},
    "split by a gap per target": {0: {(0, 0): (50, 1, "+"), (1, 0): (51, 0, "+"), (3, 0): (49, 2, "+"), (1, 1): (51, 2, "+"), (2, 1): (51, 1, "+"), (3, 1): (49, 2, "+")}},
    "split by a bin": {0: {(0, 0): (50, 1, "+"), (1, 0): (51, 0, "+")}, 3: {(2, 1): (49, 2, "+"), (3, 1): (55, 2, "+"), (3, 0): (55, 1, "+")}, 1: {(1, 5): (40, 0, "+")}},
    "strands per target": {0: {(0, 0): (50, 1, "+"), (1, 0): (51, 0, "-"), (2, 0): (49, 2, "-"), (3, 0): (55, 2, "+"), (1, 1): (51, 0, "+"), (2, 1): (49, 2, "+"),
                               (0, 2): (50, 1, "-"), (1, 2): (51, 1, "-")}},
    "ties in distance and count": {0: {(1, 0): (44, 2, "+"), (2, 0): (44, 1, "+"), (3, 0): (44, 1, "+"), (2, 1): (44, 1, "+"), (3, 1): (40, 1, "+"), (4, 1): (44, 0, "+")}},
    "best and nearest differ per target": {2: {(5, 0): (55, 2, "+"), (6, 0): (30, 0, "+"), (7, 0): (54, 1, "+"), (5, 1): (55, 0, "+"), (6, 1): (30, 2, "+"), (7, 1): (54, 1, "+")}},
}


@pytest.mark.parametrize("case", list(CASES))
def test_run_merge_matches_restatement(dump, case):
    wins = windows_of(195, K, 60, 15)  # offsets 0, 15, ..., 135
    assert len(wins) == 10
    per_bin = CASES[case]
    for with_strand in (True, False):
        if not with_strand:  # one strand: every hit on +
            per_bin = {u: {key: (c, d, "+") for key, (c, d, _) in w.items()} for u, w in per_bin.items()}
        runs = dump(per_bin)
        got = as_rows(wins, runs, per_bin, with_strand)
        assert got == ref_rows(wins, per_bin, with_strand), (case, with_strand)
        assert [(r[0], r[1]) for r in runs] == sorted((r[0], r[1]) for r in runs), "rows by bin, then target"
        for (u, t) in {(r[0], r[1]) for r in runs}:
            begins = [(r[3], r[2] == "-") for r in runs if (r[0], r[1]) == (u, t)]
            assert begins == sorted(begins), "then by begin, + before -"


def test_run_merge_by_hand():
    wins = windows_of(195, K, 60, 15)
    c = lambda count, d, t, s="": (count, d, "t%d" % t, 7 + d, s)
    # two members of a family: the first on windows 2..4, the second on the longer stretch 1..6 — a row each, the second's interval wider
    hits = dict([((j, 0), c(50, 1, 0)) for j in (2, 3, 4)] + [((j, 1), c(50, 2 if j != 5 else 0, 1)) for j in range(1, 7)])
    assert merge_targets(wins, K, hits) == [(31, 120, 1, "t0", 8), (16, 150, 0, "t1", 7)]
    # a window that hits only the later record; a gap splits one target's run and not the other's
    hits = {(0, 0): c(9, 1, 0), (1, 0): c(9, 1, 0), (3, 0): c(9, 0, 0), (2, 2): c(9, 2, 2), (3, 2): c(9, 2, 2), (1, 2): c(9, 2, 2)}
    assert merge_targets(wins, K, hits) == [(1, 75, 1, "t0", 8), (46, 105, 0, "t0", 7), (16, 105, 2, "t2", 9)]
    # strands per target: + before - where a + and a - run of one target begin with neighbours
    hits = {(0, 0): c(1, 1, 0, "-"), (1, 0): c(1, 1, 0, "+"), (0, 1): c(1, 0, 1, "+")}
    assert merge_targets(wins, K, hits) == [(1, 60, 1, "t0", 8, "-"), (16, 75, 1, "t0", 8, "+"), (1, 60, 0, "t1", 7, "+")]
    assert merge_targets(wins, K, {}) == []


def test_invariant_helpers_by_hand():
    d = {(0, 1, 2, 0): (2, "a", 9, ""), (0, 1, 2, 1): (1, "b", 8, ""), (0, 1, 2, 3): (1, "c", 7, ""), (0, 2, 2, 3): (0, "c", 7, "")}
    assert nearest_of(d) == {(0, 1, 2): (1, "b", 8, ""), (0, 2, 2): (0, "c", 7, "")}
    rows = [("q", "x", "1", "60"), ("q", "x", "16", "90"), ("q", "x", "100", "120"), ("q", "y", "5", "9"), ("q", "x", "91", "95")]
    assert union_of(rows) == {("q", "x"): [(1, 95), (100, 120)], ("q", "y"): [(5, 9)]}


WINDOW = ["--window", "60", "-e", "1"]
FRAME = ["--translate", "--frame-window", "30", "-e", "1"]
REFUSALS = [
    (["-e", "1", "--window-targets"], ["--window-targets", "--verify-windows", "--verify-frame-windows"]),
    (WINDOW + ["--window-targets"], ["--window-targets", "--verify-windows"]),
    (FRAME + ["--window-targets"], ["--window-targets", "--verify-frame-windows"]),
    (["-e", "1", "--verify", "--window-targets"], ["--window-targets", "--verify-windows"]),
    (["-e", "1", "--verify", "--all-targets", "--window-targets"], ["--window-targets", "--verify-windows"]),
    # --all-targets next to the window modes stays refused where it was, and the message now names the flag that is meant
    (WINDOW + ["--verify-windows", "--all-targets"], ["--verify-windows cannot be combined with --all-targets", "--window-targets"]),
    (FRAME + ["--verify-frame-windows", "--all-targets"], ["--frame-window cannot be combined with --all-targets", "--window-targets"]),  # (the first of the two refusals, as before)
    (WINDOW + ["--verify-windows", "--window-targets", "--all-targets"], ["--all-targets", "--window-targets"]),
    (WINDOW + ["--all-targets"], ["--window cannot be combined with --all-targets", "--window-targets"]),
    (FRAME + ["--all-targets"], ["--frame-window cannot be combined with --all-targets", "--window-targets"]),
    # the new flag changes none of the other refusals of the window modes
    (WINDOW + ["--verify-windows", "--window-targets", "--align"], ["--align", "--align-windows"]),
    (WINDOW + ["--verify-windows", "--window-targets", "--verify"], ["--verify-windows cannot be combined with --verify:"]),
    (["--window", "60", "--threshold", "0.5", "--verify-windows", "--window-targets"], ["--threshold"]),
]


@pytest.mark.parametrize("flags,words", REFUSALS, ids=[" ".join(f) for f, _ in REFUSALS])
def test_cli_refuses_at_parse_time(tmp_path, flags, words):
    """None of these reaches the index file (which does not exist) or a device."""
    out = tmp_path / "out.tsv"
    r = subprocess.run([TETREX, "search"] + flags + ["-o", str(out), str(tmp_path / "none.ibf"), str(tmp_path / "none.fa")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0, r.stderr
    assert r.stderr.startswith("[Search Parser Error] ") and all(w in r.stderr for w in words), r.stderr
    assert r.stdout == "" and not out.exists()


@pytest.mark.parametrize("flags", [WINDOW + ["--step", "15", "--verify-windows", "--window-targets"],
                                   WINDOW + ["--verify-windows", "--window-targets", "--align-windows", "--counts", "-v"],
                                   FRAME + ["--frame-step", "10", "--verify-frame-windows", "--window-targets"],
                                   FRAME + ["--verify-frame-windows", "--window-targets", "--align-windows", "--counts", "-v"]], ids=" ".join)
def test_the_flag_parses(tmp_path, flags):
    """with every option it needs, either windowed command gets as far as the index file"""
    r = subprocess.run([TETREX, "search"] + flags + [str(tmp_path / "none.ibf"), str(tmp_path / "none.fa")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Parser Error" not in r.stderr and "Index not valid" in r.stderr, r.stderr
