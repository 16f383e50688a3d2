"""`tetrex search --translate --frame-window` without a GPU: the properties of tests/frame_window_ref.py (the restatement
tests/test_gpu_translate_windows.py and tests/test_gpu_search_frame_window.py hold the library and the command to) — the
nucleotides of a run of residues cut out and translated give the run back, on both strands and at all offsets; the windows
cover every residue; begins and ends never decrease — the refusals the command makes while it parses its options, before it
reads an index or touches a device, and txq_translate_windows_bound (which needs no GPU) against the restatement."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from frame_window_ref import (frame_len, frame_windows, window_ranges, translate_windows, window_count, residues_on_record, cut_and_translate,
                              merge_rows, search_rows)
from translate_ref import translate_frame

TETREX = os.path.join(ROOT, "bin", "tetrex")


def _nt(rng, n, junk=0.0):
    s = rng.choice(list("ACGT"), size=n)
    if junk:
        s = np.where(rng.random(n) < junk, rng.choice(list("NnRu-"), size=n), s)
    return "".join(s)


def test_cut_and_translate_gives_the_residues_back():
    rng = np.random.default_rng(7)
    for L in list(range(0, 40)) + [100, 101, 102]:
        seq = _nt(rng, L, 0.05)
        for f in range(6):
            residues = translate_frame(seq, f)
            assert len(residues) == frame_len(L, f % 3)
            for ra in range(len(residues) + 1):
                for rb in (ra + 1, ra + 5, len(residues)):
                    if ra < rb <= len(residues):
                        b, e = residues_on_record(L, f, ra, rb)
                        assert 1 <= b <= e <= L and e - b + 1 == 3 * (rb - ra)
                        assert cut_and_translate(seq, f, b, e) == residues[ra:rb], (L, f, ra, rb)


@pytest.mark.parametrize("k,W,S", [(6, 40, 10), (6, 40, 1), (6, 40, 40), (1, 1, 1), (5, 7, 3), (12, 12, 12), (12, 25, 9)])
def test_windows_cover_the_frame_and_slide(k, W, S):
    rng = np.random.default_rng(k * 1000 + W * 10 + S)
    for L in list(range(0, 3 * (W + 2 * S + 3) + 3)):
        seq = _nt(rng, L, 0.02)
        last_begin = last_end = 0
        offsets, win_offsets, begins, lens = translate_windows([seq], k, W, S)
        at = 0
        for f in range(6):
            R = frame_len(L, f % 3)
            wins = frame_windows(L, f, k, W, S)
            assert len(wins) == int(win_offsets[f + 1] - win_offsets[f])
            covered = set()
            for a, n in wins:
                assert 0 <= a and a + n <= R and n >= k
                covered.update(range(a, a + n))
            assert covered == (set(range(R)) if R >= k else set())
            for (b, w), (a, n) in zip(window_ranges(seq, f, k, W, S), wins):
                assert 0 <= w <= n - k + 1
                assert int(begins[at]) == int(offsets[f]) + b and int(lens[at]) == w
                assert int(begins[at]) + w <= int(offsets[f + 1])
                # over the whole array, frame after frame: begins and ends never decrease
                assert int(begins[at]) >= last_begin and int(begins[at]) + w >= last_end
                last_begin, last_end = int(begins[at]), int(begins[at]) + w
                at += 1
        assert at == begins.size


def test_a_window_of_stops_is_empty_and_keeps_its_place():
    k, W, S = 3, 6, 3
    seq = "GCT" * 6 + "TAA" * 8 + "GCT" * 6  # frame +1: AAAAAA ******** AAAAAA
    got = window_ranges(seq, 0, k, W, S)
    wins = frame_windows(len(seq), 0, k, W, S)
    assert [a for a, _ in wins] == [0, 3, 6, 9, 12, 14]
    assert got == [(0, 4), (3, 1), (4, 0), (4, 0), (4, 2), (4, 4)]


def test_run_merge_and_coordinates():
    k, W, S = 6, 40, 10
    L = 3 * 100 + 2
    wins = frame_windows(L, 1, k, W, S)  # frame +2: 100 residues, windows at 0, 10, ..., 60
    assert [a for a, _ in wins] == [0, 10, 20, 30, 40, 50, 60]
    ws = [35] * 7
    assert merge_rows(L, 1, wins, ws, {}) == []
    assert merge_rows(L, 1, wins, ws, {0: 30}) == [(2, 121)]
    assert merge_rows(L, 1, wins, ws, {1: 30, 2: 33, 3: 33, 5: 31}, True) == [(32, 211, "33/35"), (152, 271, "31/35")]
    # the reverse strand: frame -2 of 302 bytes has 100 residues, residue 0 ends at byte 301
    assert merge_rows(L, 4, wins, ws, {0: 30}) == [(182, 301)]
    assert merge_rows(L, 4, wins, ws, {6: 30}) == [(2, 121)]
    # the w of the best window is its own
    assert merge_rows(L, 0, wins, [35, 20, 35, 35, 35, 35, 35], {0: 18, 1: 19}, True) == [(1, 150, "19/20")]


def test_search_rows_order_and_notes():
    k, W, S = 2, 4, 2
    records = [("a", "GCT" * 8), ("tiny", "GCTGC"), ("stops", "TAATAGTGA" * 3), ("b", "GCT" * 3)]
    def count_fn(r, f, j):
        return [9, 9 if j == 0 else 0]
    rows, (no_kmer, unsearched), n = search_rows(records, k, W, S, count_fn, 2, errors=1, with_counts=True)
    # "b": frames of 3 and 2 residues, w = 2 or 1 <= k E: no window has a threshold above 0
    assert "tiny" in no_kmer and "b" in unsearched and "a" not in no_kmer + unsearched
    a_rows = [r for r in rows if r[0] == "a"]
    assert a_rows[0] == ("a", 0, "+1", 1, 24, "9/3") and a_rows[1] == ("a", 1, "+1", 1, 12, "9/3")
    assert [r[2] for r in a_rows] == sorted((r[2] for r in a_rows), key=["+1", "+2", "+3", "-1", "-2", "-3"].index)
    assert n == sum(1 for name, s in records for f in range(6) for _, w in window_ranges(s, f, k, W, S) if w > k)


@pytest.mark.parametrize("k,W,S", [(6, 40, 10), (1, 1, 1), (12, 12, 5), (5, 7, 7)])
def test_windows_bound(k, W, S):
    from tetrex_amd import capi
    rng = np.random.default_rng(3)
    lengths = list(range(0, 3 * (W + S + 2) + 3)) + [int(x) for x in rng.integers(0, 5000, size=50)]
    rec = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    assert capi.translate_windows_bound(rec, k, W, S) == window_count(lengths, k, W, S)
    assert capi.translate_windows_bound(rec[:1], k, W, S) == 0
    for one in (3 * k - 1, 3 * k, 3 * W + 2, 3 * (W + 1)):
        assert capi.translate_windows_bound(np.array([5, 5 + one], dtype=np.uint64), k, W, S) == window_count([one], k, W, S)


def test_windows_bound_refusals():
    from tetrex_amd import capi
    rec = np.array([0, 100, 250], dtype=np.uint64)
    for k, W, S in [(0, 10, 5), (13, 20, 5), (6, 5, 1), (6, 40, 0), (6, 40, 41)]:
        with pytest.raises(capi.TxqError):
            capi.translate_windows_bound(rec, k, W, S)
    with pytest.raises(capi.TxqError):
        capi.translate_windows_bound(np.array([0, 100, 50], dtype=np.uint64), 6, 40, 10)


REFUSALS = [
    (["--frame-window", "40", "-e", "2"], "needs --translate"),
    (["--frame-step", "10", "--translate", "-e", "2"], "--frame-step"),
    (["--translate", "--frame-window", "40"], "-e E or --threshold F"),
    (["--translate", "--frame-window", "40", "-e", "2", "--threshold", "0.5"], "exclude each other"),
    (["--translate", "--frame-window", "40", "-e", "2", "--window", "60"], "--window"),
    (["--translate", "--frame-window", "40", "-e", "2", "--step", "10"], "--step"),
    (["--translate", "--frame-window", "40", "-e", "2", "--verify"], "frame windows are not verified"),
    (["--translate", "--frame-window", "40", "-e", "2", "--verify-frames"], "frame windows are not verified"),
    (["--translate", "--frame-window", "40", "-e", "2", "--verify-frames", "--align"], "frame windows are not verified"),
    (["--translate", "--frame-window", "40", "-e", "2", "--verify-frames", "--all-targets"], "frame windows are not verified"),
    (["--translate", "--frame-window", "0", "-e", "2"], "--frame-window must be"),
    (["--translate", "--frame-window", "-4", "-e", "2"], "--frame-window must be"),
    (["--translate", "--frame-window", "w", "-e", "2"], "--frame-window must be"),
    (["--translate", "--frame-window", "40", "--frame-step", "0", "-e", "2"], "--frame-step must be"),
    (["--translate", "--frame-window", "40", "--frame-step", "41", "-e", "2"], "--frame-step must be"),
    (["--translate", "--frame-window", "40", "--frame-step", "s", "-e", "2"], "--frame-step must be"),
    (["--window", "60", "-e", "1", "--translate"], "--frame-window"),  # the old refusal now names the way
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
