"""`tetrex search --window` without a GPU: the window layout and the run merge of tests/search_window_ref.py (the restatement
tests/test_gpu_search_window.py holds the command to) at their edges, and the refusals the command makes while it parses its
options, before it reads an index or touches a device."""
import os
import subprocess

import pytest

from conftest import ROOT
from search_window_ref import windows_of, merge_rows, threshold_of, search_rows

TETREX = os.path.join(ROOT, "bin", "tetrex")


def test_window_layout_edges():
    k, W, S = 6, 60, 15
    assert windows_of(k - 1, k, W, S) == []
    assert windows_of(k, k, W, S) == [(0, k)]
    assert windows_of(W - 1, k, W, S) == [(0, W - 1)]
    assert windows_of(W, k, W, S) == [(0, W)]
    assert windows_of(W + 1, k, W, S) == [(0, W), (1, W)]                      # the end-aligned tail, 1 < S behind
    assert windows_of(W + S, k, W, S) == [(0, W), (S, W)]                      # (no tail: the last window ends at L)
    assert windows_of(W + S + 1, k, W, S) == [(0, W), (S, W), (S + 1, W)]
    assert windows_of(W + S - 1, k, W, S) == [(0, W), (S - 1, W)]
    assert windows_of(0, k, W, S) == []


@pytest.mark.parametrize("W,S", [(60, 1), (60, 60), (60, 15), (6, 1), (6, 6), (7, 3), (150, 50), (16, 16)])
def test_every_letter_is_covered_and_windows_slide(W, S):
    k = min(6, W)
    for L in list(range(k, 3 * W + 2 * S + 3)):
        wins = windows_of(L, k, W, S)
        covered = set()
        for b, n in wins:
            assert 0 <= b and b + n <= L and n >= k and (n == W or (n == L and L <= W))
            covered.update(range(b, b + n))
        assert covered == set(range(L)), (L, W, S)
        begins = [b for b, _ in wins]
        ends = [b + n for b, n in wins]
        assert begins == sorted(set(begins)) and ends == sorted(set(ends))   # strictly sliding: no window twice
        gaps = [y - x for x, y in zip(begins, begins[1:])]
        assert all(g == S for g in gaps[:-1]) and all(1 <= g <= S for g in gaps[-1:])
        # any stretch of W + S - 1 letters holds a whole window
        for at in range(0, L - (W + S - 1) + 1):
            assert any(at <= b and b + n <= at + W + S - 1 for b, n in wins), (L, at)


def test_step_one_and_step_window():
    assert windows_of(10, 3, 8, 1) == [(0, 8), (1, 8), (2, 8)]
    assert windows_of(24, 3, 8, 8) == [(0, 8), (8, 8), (16, 8)]
    assert windows_of(25, 3, 8, 8) == [(0, 8), (8, 8), (16, 8), (17, 8)]


def test_thresholds():
    assert threshold_of(55, 6, errors=2) == 43
    assert threshold_of(12, 6, errors=2) == 0 and threshold_of(13, 6, errors=2) == 1
    assert threshold_of(55, 6, fraction=0.5) == 28 and threshold_of(1, 6, fraction=0.01) == 1


def test_run_merge():
    k = 6
    wins = windows_of(135, k, 60, 15)  # offsets 0, 15, ..., 75
    assert [b for b, _ in wins] == [0, 15, 30, 45, 60, 75]
    assert merge_rows(wins, k, {}) == []
    assert merge_rows(wins, k, {0: 50}) == [(1, 60)]
    assert merge_rows(wins, k, {5: 50}) == [(76, 135)]
    assert merge_rows(wins, k, {j: 50 for j in range(6)}) == [(1, 135)]
    # a run broken by one missing window: two rows, though their letters overlap
    assert merge_rows(wins, k, {0: 50, 1: 51, 3: 49, 4: 55}) == [(1, 75), (46, 120)]
    assert merge_rows(wins, k, {0: 50, 1: 51, 3: 49, 4: 55}, True) == [(1, 75, "51/55"), (46, 120, "55/55")]
    # ties in counts: the earliest window of the run
    assert merge_rows(wins, k, {1: 40, 2: 44, 3: 44}, True) == [(16, 105, "44/55")]
    tail = windows_of(70, k, 60, 15)  # (0, 60), (10, 60): the tail window
    assert merge_rows(tail, k, {0: 30, 1: 30}, True) == [(1, 70, "30/55")]
    short = windows_of(20, k, 60, 15)
    assert merge_rows(short, k, {0: 9}, True) == [(1, 20, "9/15")]


def test_best_window_tie_is_the_earliest_not_the_first_seen():
    wins = windows_of(200, 6, 60, 15)
    assert merge_rows(wins, 6, {4: 41, 2: 41, 3: 40}, True) == [(31, 120, "41/55")]
    # (the w of the best window, where windows differ in length, is its own: a single short record)
    assert merge_rows([(0, 30)], 6, {0: 25}, True) == [(1, 30, "25/25")]


def test_search_rows_order_and_notes():
    k, W, S = 3, 8, 4
    records = [("a", "x" * 16), ("tiny", "xx"), ("b", "x" * 9)]
    # bin 0 is hit everywhere, bin 1 in the windows that begin at letter 0 only
    def count_fn(r, b, n):
        return [n - k + 1, n - k + 1 if b == 0 else 0]
    rows, (skipped, unsearched) = search_rows(records, k, W, S, count_fn, 2, errors=1, with_counts=True)
    assert skipped == ["tiny"] and unsearched == []
    assert rows == [("a", 0, 1, 16, "6/6"), ("a", 1, 1, 8, "6/6"), ("b", 0, 1, 9, "6/6"), ("b", 1, 1, 8, "6/6")]
    rows, (skipped, unsearched) = search_rows([("c", "x" * 5)], k, W, S, count_fn, 2, errors=1)
    assert rows == [] and unsearched == ["c"]  # w = 3 = k E: threshold 0, not searched


REFUSALS = [
    (["--step", "3", "-e", "1"], "--step"),
    (["--window", "60", "-e", "1", "--translate"], "--translate"),
    (["--window", "60", "-e", "1", "--verify"], "--verify:"),
    (["--window", "60", "-e", "1", "--translate", "--verify-frames"], "--translate"),
    (["--window", "60", "-e", "1", "--verify-frames"], "--verify-frames"),
    (["--window", "60", "-e", "1", "--align"], "--align"),
    (["--window", "60", "-e", "1", "--verify", "--all-targets"], "--all-targets"),
    (["--window", "60"], "-e E or --threshold F"),
    (["--window", "0", "-e", "1"], "--window must be"),
    (["--window", "-5", "-e", "1"], "--window must be"),
    (["--window", "x", "-e", "1"], "--window must be"),
    (["--window", "60", "--step", "0", "-e", "1"], "--step must be"),
    (["--window", "60", "--step", "61", "-e", "1"], "--step must be"),
    (["--window", "60", "--step", "s", "-e", "1"], "--step must be"),
    (["--window", "60", "-e", "1", "--threshold", "0.5"], "exclude each other"),
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
