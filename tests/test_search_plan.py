"""The host planning of `tetrex search` (tetrex_amd/csrc/host/search_plan.hpp) without a GPU: tests/native/search_plan_dump.cpp,
built with the address and undefined-behaviour sanitizers, prints what the header computes — the windows of a record, the
thresholds, the runs of hit windows, the window batches and the record batches — and this file holds it to the Python
restatements the GPU tests hold the command to (tests/search_window_ref.py, tests/frame_window_ref.py).  The cuts have no
restatement: they are checked for what a cut must be — contiguous, complete, within both limits unless a single item is
larger, and greedy."""
import os
import subprocess

import pytest

import frame_window_ref
import search_window_ref
from conftest import ROOT
from search_window_ref import windows_of, threshold_of

K = 6
WS = [(60, 1), (60, 60), (60, 15), (6, 1), (6, 6), (7, 3), (150, 50), (16, 16)]  # the pairs of tests/test_search_window_cpu.py


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("search_plan") / "search_plan_dump")
    # (-Wno-unknown-pragmas: the kernels' plan headers, which the header includes, carry unroll pragmas for the device compiler)
    subprocess.run(["g++", "-std=c++20", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(ROOT, "tests", "native", "search_plan_dump.cpp")], check=True, timeout=600)

    def run(*args, stdin=""):
        r = subprocess.run([exe] + [str(a) for a in args], input=stdin, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-3000:])
        return [line.split() for line in r.stdout.splitlines()]
    return run


def cxx_windows(dump, k, W, S, Lmax):
    """{L: [(begin, len)]} for L = 0 .. Lmax"""
    return {int(f[0]): [tuple(int(x) for x in w.split(":")) for w in f[1:]] for f in dump("windows", k, W, S, Lmax)}


@pytest.mark.parametrize("W,S", WS)
def test_window_layout(dump, W, S):
    Lmax = 3 * W + 2 * S + 2
    got = cxx_windows(dump, K, W, S, Lmax)
    assert sorted(got) == list(range(Lmax + 1))
    for L in range(Lmax + 1):
        assert got[L] == windows_of(L, K, W, S), (L, W, S)


def test_thresholds(dump):
    nmax = 120
    lines = dump("thresholds", K, nmax)
    assert len(lines) == 6 * (nmax + 1)
    seen = set()
    for kind, x, n, t in lines:
        n, t = int(n), int(t)
        if kind == "e":
            assert t == threshold_of(n, K, errors=int(x)), (x, n)
        else:
            assert kind == "f" and t == threshold_of(n, K, fraction=float(x)), (x, n)
        seen.add((kind, x))
    assert seen == {("e", "0"), ("e", "1"), ("e", "2"), ("f", "0.01"), ("f", "0.5"), ("f", "1.0")}


def cxx_runs(dump, per_bin):
    """per_bin: {bin: {window: count}} of one record or frame -> {bin: [(first, last, best, count)]}, the runs in the order given"""
    hits = [(j, u, per_bin[u][j]) for u in sorted(per_bin) for j in sorted(per_bin[u])]  # by bin, then window
    out = {}
    for u, first, last, best, count in dump("runs", stdin="".join("%d %d %d\n" % h for h in hits)):
        out.setdefault(int(u), []).append((int(first), int(last), int(best), int(count)))
    return out


WINDOW_MERGES = [  # (L, W, S, {bin: {window: count}}): the cases of test_search_window_cpu.py test_run_merge, and more
    (135, 60, 15, {0: {}}),
    (135, 60, 15, {0: {0: 50}}),
    (135, 60, 15, {0: {5: 50}}),
    (135, 60, 15, {0: {j: 50 for j in range(6)}}),
    (135, 60, 15, {0: {0: 50, 1: 51, 3: 49, 4: 55}}),
    (135, 60, 15, {0: {1: 40, 2: 44, 3: 44}}),
    (70, 60, 15, {0: {0: 30, 1: 30}}),
    (20, 60, 15, {0: {0: 9}}),
    (200, 60, 15, {0: {4: 41, 2: 41, 3: 40}}),
    (30, 60, 15, {0: {0: 25}}),
    # tied counts at the front, in the middle and at the back of a run; every window tied
    (200, 60, 15, {0: {0: 7, 1: 7, 2: 3}, 1: {3: 1, 4: 9, 5: 9}, 2: {6: 2, 7: 2, 8: 2, 9: 2}}),
    # runs that touch but belong to different bins: windows 0-1 of bin 0, 2-3 of bin 1, 4 of bin 2 — and 0-4 of bin 3
    (200, 60, 15, {0: {0: 5, 1: 6}, 1: {2: 6, 3: 5}, 2: {4: 8}, 3: {0: 1, 1: 1, 2: 2, 3: 1, 4: 2}}),
    # a bin's last window next to the following bin's first in value: bin 0 ends at window 3, bin 1 begins at window 4
    (200, 60, 15, {0: {3: 5}, 1: {4: 5}, 5: {5: 5}}),
]


@pytest.mark.parametrize("L,W,S,per_bin", WINDOW_MERGES, ids=[str(i) for i in range(len(WINDOW_MERGES))])
def test_window_run_merge(dump, L, W, S, per_bin):
    wins = cxx_windows(dump, K, W, S, L)[L]
    runs = cxx_runs(dump, per_bin)
    for u, hit_counts in per_bin.items():
        rows = [(wins[first][0] + 1, wins[last][0] + wins[last][1], "%d/%d" % (count, wins[best][1] - K + 1))
                for first, last, best, count in runs.get(u, [])]
        assert rows == search_window_ref.merge_rows(wins, K, hit_counts, True), (u, runs.get(u))
        assert all(hit_counts[best] == count for _, _, best, count in runs.get(u, []))
    assert set(runs) == {u for u, h in per_bin.items() if h}


FRAME_MERGES = [  # (L, frame, ws, {bin: {window: count}}), k = 6, W = 40, S = 10: test_frame_window_cpu.py test_run_merge_and_coordinates
    (302, 1, [35] * 7, {0: {}}),
    (302, 1, [35] * 7, {0: {0: 30}}),
    (302, 1, [35] * 7, {0: {1: 30, 2: 33, 3: 33, 5: 31}}),
    (302, 4, [35] * 7, {0: {0: 30}}),
    (302, 4, [35] * 7, {0: {6: 30}}),
    (302, 0, [35, 20, 35, 35, 35, 35, 35], {0: {0: 18, 1: 19}}),
    (302, 5, [35, 20, 35, 35, 35, 35, 35], {0: {0: 19, 1: 19}, 1: {2: 4, 3: 4}, 2: {3: 1, 4: 2, 5: 2, 6: 1}}),  # ties; bins that touch
]


@pytest.mark.parametrize("L,f,ws,per_bin", FRAME_MERGES, ids=[str(i) for i in range(len(FRAME_MERGES))])
def test_frame_window_run_merge(dump, L, f, ws, per_bin):
    W, S = 40, 10
    R = frame_window_ref.frame_len(L, f % 3)
    wins = cxx_windows(dump, K, W, S, R)[R]
    assert wins == frame_window_ref.frame_windows(L, f, K, W, S) and len(wins) == len(ws)
    runs = cxx_runs(dump, per_bin)
    for u, hit_counts in per_bin.items():
        rows = [frame_window_ref.residues_on_record(L, f, wins[first][0], wins[last][0] + wins[last][1]) + ("%d/%d" % (count, ws[best]),)
                for first, last, best, count in runs.get(u, [])]
        assert rows == frame_window_ref.merge_rows(L, f, wins, ws, hit_counts, True), (u, runs.get(u))


def check_cuts(cut, n_items, fits, what):
    """cut: the boundaries; fits(a, b): the items [a, b) respect the limits"""
    assert cut[0] == 0 and cut[-1] == n_items, what                       # everything, in order ...
    assert all(a < b for a, b in zip(cut, cut[1:])) or n_items == 0, what  # ... exactly once, in contiguous batches with no empty one
    for a, b in zip(cut, cut[1:]):
        assert fits(a, b) or b - a == 1, (what, a, b)                      # both limits, unless a single item is larger
        assert b == n_items or not fits(a, b + 1), (what, a, b)            # greedy: the next item would not have fitted


def sliding_windows():
    """begins and lens as `tetrex search --window` makes them: records back to back, window j of a record of L letters owns the
    values [base + a, base + a + len - k + 1); one record is a single window wider than any bound used below"""
    begins, lens, base = [], [], 0
    for L, W, S in [(150, 20, 7), (100, 200, 50), (5, 20, 7), (60, 20, 20), (27, 20, 1), (6, 20, 7), (90, 20, 7)]:
        for a, n in windows_of(L, K, W, S):
            begins.append(base + a)
            lens.append(n - K + 1)
        base += max(L - K + 1, 0)
    return begins, lens


@pytest.mark.parametrize("max_values,max_windows", [(64, 7), (64, 1000), (10 ** 6, 7), (15, 3), (64, 1), (10 ** 6, 10 ** 6)])
def test_window_batches(dump, max_values, max_windows):
    begins, lens = sliding_windows()
    assert max(lens) == 95 and len(begins) == 44
    out = dump("cut_windows", max_values, max_windows, stdin="".join("%d %d\n" % x for x in zip(begins, lens)))
    cut = [int(x) for x in out[0][1:]]
    span = lambda a, b: begins[b - 1] + lens[b - 1] - begins[a]
    check_cuts(cut, len(begins), lambda a, b: b <= len(begins) and b - a <= max_windows and span(a, b) <= max_values, (max_values, max_windows))
    assert out[1] == ["most", str(max(span(a, b) for a, b in zip(cut, cut[1:]))), str(max(b - a for a, b in zip(cut, cut[1:])))]
    if (max_values, max_windows) == (64, 7):
        assert len(cut) - 1 >= -(-len(begins) // max_windows) == 7  # many batches ...
        assert any(b - a == 1 and span(a, b) > max_values for a, b in zip(cut, cut[1:]))  # ... and the wide window is alone in one


@pytest.mark.parametrize("max_values,max_records", [(64, 0), (64, 3), (10 ** 6, 1), (10 ** 6, 0), (30, 2)])
def test_record_batches(dump, max_values, max_records):
    lengths = [10, 0, 0, 30, 24, 1, 100, 0, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 64, 1, 0, 63, 2, 0]  # empty records; one above the bound
    bounds = list(lengths)  # (any bound will do; the command's is txq_translate_bound of the record)
    offsets = [0]
    for L in lengths:
        offsets.append(offsets[-1] + L)
    out = dump("cut_records", max_values, max_records, stdin=" ".join(map(str, offsets)) + "\n" + " ".join(map(str, bounds)) + "\n")
    cut = [int(x) for x in out[0][1:]]
    fits = lambda a, b: b <= len(lengths) and sum(bounds[a:b]) <= max_values and (max_records == 0 or b - a <= max_records)
    check_cuts(cut, len(lengths), fits, (max_values, max_records))
    batches = list(zip(cut, cut[1:]))
    assert out[1] == ["most", str(max(sum(bounds[a:b]) for a, b in batches)), str(max(offsets[b] - offsets[a] for a, b in batches)),
                      str(max(b - a for a, b in batches))]
    if max_values == 64:
        assert (6, 7) in batches and len(batches) >= 5  # the record above the bound is a batch of its own


def test_no_items_no_batches(dump):
    assert dump("cut_windows", 64, 7) == [["cut", "0"], ["most", "0", "0"]]
    assert dump("cut_records", 64, 3, stdin="0\n\n") == [["cut", "0"], ["most", "0", "0", "0"]]
