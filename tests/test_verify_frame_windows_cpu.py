"""`tetrex search --translate --frame-window --verify-frame-windows` without a GPU: the threshold lemma by brute
force, the refusals the command makes while it parses its options, and the letters walk of txq_frame_window_letters_device
(csrc/txq_frame_windows_plan.hpp) run on the CPU under sanitizers by tests/native/frame_window_letters_sim.cpp."""
import os
import subprocess

import numpy as np
import pytest

import edit_ref as E
import verify_frame_windows_ref as R
from conftest import ROOT

TETREX = os.path.join(ROOT, "bin", "tetrex")
AMINO = "ACDEFGHIKLMNPQRSTVWY"


def _window(rng, n, s):
    """n residues with exactly s stops"""
    w = list(rng.choice(list(AMINO), size=n))
    for at in rng.choice(n, size=s, replace=False):
        w[int(at)] = "*"
    return w


def _edited(rng, window, edits, stops_first):
    """a target made from the window by at most `edits` edits; stops_first: the edits go to the stops before anything else (a
    stop matches nothing, so a target within reach has to spend an edit on each)"""
    t = list(window)
    left = edits
    if stops_first:
        for at in [i for i, c in enumerate(t) if c == "*"][::-1]:
            if left == 0:
                break
            if rng.integers(0, 2):
                t[at] = AMINO[int(rng.integers(0, len(AMINO)))]
            else:
                del t[at]
            left -= 1
    for _ in range(int(rng.integers(0, left + 1))):
        kind, at = int(rng.integers(0, 3)), int(rng.integers(0, len(t)))
        if kind == 0:
            t[at] = AMINO[int(rng.integers(0, len(AMINO)))]
        elif kind == 1:
            t.insert(at, AMINO[int(rng.integers(0, len(AMINO)))])
        elif len(t) > 1:
            del t[at]
    return "".join(t)


@pytest.mark.parametrize("k", [3, 4, 5, 6])
def test_threshold_lemma_by_brute_force(k):
    """A window of w stop-free k-mers and s stops within E edits of a target shares at least w - k (E - s) of those k-mers with
    it, and a window with s > E is within E of nothing: the dynamic program decides what is within E, a set of the target's
    k-mers what is shared."""
    rng = np.random.default_rng(100 + k)
    within = {e: 0 for e in range(4)}
    for trial in range(600):
        errors = trial % 4
        s = int(rng.integers(0, errors + 2))
        n = int(rng.integers(3 * k, 8 * k))
        window = "".join(_window(rng, n, s))
        target = "X" * 3 + _edited(rng, window, errors, trial % 5 != 0) + "X" * 3
        d, _ = E.distance(window, target, R.PEPTIDE_CODES)
        stop_free = [window[c:c + k] for c in range(n - k + 1) if "*" not in window[c:c + k]]
        w = len(stop_free)
        t = R.stop_threshold(w, s, k, errors)
        if s > errors:
            assert d > errors and t == R.NOT_SEARCHED, (window, target, d)
            assert E.distance(window, window, R.PEPTIDE_CODES)[0] >= s  # (not even itself)
            continue
        if d > errors:
            continue
        within[errors] += 1
        kmers = {target[i:i + k] for i in range(len(target) - k + 1)}
        shared = sum(1 for x in stop_free if x in kmers)
        assert shared >= w - k * (errors - s), (window, target, d, shared, w, s)
        if t != R.NOT_SEARCHED:
            assert shared >= t
    assert all(v >= 40 for v in within.values()), within


def test_the_threshold_by_hand():
    assert R.stop_threshold(35, 0, 6, 2) == 23 and R.stop_threshold(29, 1, 6, 2) == 23 and R.stop_threshold(23, 2, 6, 2) == 23
    assert R.stop_threshold(23, 3, 6, 2) == R.NOT_SEARCHED and R.stop_threshold(12, 0, 6, 2) == R.NOT_SEARCHED
    assert R.stop_threshold(13, 0, 6, 2) == 1 and R.stop_threshold(0, 2, 6, 2) == R.NOT_SEARCHED and R.stop_threshold(1, 2, 6, 2) == 1
    # a full window with at most E stops is always searched where the command accepts W: w >= W - k + 1 - k s
    for k in (3, 6):
        for errors in range(4):
            W = k * errors + k  # the smallest workable --frame-window
            for s in range(errors + 1):
                assert R.stop_threshold(max(W - k + 1 - k * s, 0), s, k, errors) >= 1


def test_the_restatement_on_a_small_record():
    # frame +1 of ATGTAAGCT... : M * A ...; one stop in the first window of 4 residues
    seq = "ATGTAAGCTGCTGCTGCTAAA"  # M * A A A A K
    frames, foff, woff, begins, lens, stops, ws, thr = R.window_letters([seq], 3, 4, 2, 1)
    assert frames[int(foff[0]):int(foff[1])] == "M*AAAAK"
    assert [int(x) for x in woff[:2]] == [0, 3] and list(begins[:3]) == [0, 2, 3] and list(lens[:3]) == [4, 4, 4]  # windows 0, 2 and the tail 3
    assert list(stops[:3]) == [1, 0, 0] and list(ws[:3]) == [0, 2, 2]
    assert list(thr[:3]) == [R.NOT_SEARCHED, R.NOT_SEARCHED, R.NOT_SEARCHED]  # w - k (E - s): 0 - 0, 2 - 3, 2 - 3
    assert list(R.window_letters([seq], 3, 4, 2, 0)[7][:3]) == [R.NOT_SEARCHED, 2, 2]


def test_letters_walk_under_sanitizers(tmp_path):
    """frame lookup, window_at, clipped loads, head and tail masks and the popcount against a byte-by-byte count, records of
    every length 0 .. 120 nt, the buffer at every alignment and ending exactly at frames_bytes"""
    exe = str(tmp_path / "frame_window_letters_sim")
    subprocess.run(["g++", "-std=c++20", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "native", "frame_window_letters_sim.cpp"),
                    os.path.join(ROOT, "tetrex_amd", "csrc", "host", "encoder.cpp")], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    words = r.stdout.split()
    assert r.stdout.startswith("frame_window_letters_sim ok: ") and int(words[2]) >= 100 and int(words[4]) > 100000 and int(words[6]) > 10000, r.stdout
    assert int(words[8]) > int(words[4]) and int(words[10]) > 1000, r.stdout


REFUSALS = [
    (["--verify-frame-windows", "-e", "1"], "--translate"),
    (["--translate", "--verify-frame-windows", "-e", "1"], "--frame-window"),
    (["--translate", "--frame-window", "40", "--verify-frame-windows"], "-e E"),
    (["--translate", "--frame-window", "40", "--threshold", "0.5", "--verify-frame-windows"], "--threshold"),
    (["--translate", "--frame-window", "40", "-e", "1", "--verify-frame-windows", "--window", "60"], "--window"),
    (["--translate", "--verify-frame-windows", "-e", "1", "--window", "60"], "--verify-frame-windows cannot be combined with --window"),
    (["--translate", "--frame-window", "40", "-e", "1", "--verify-frame-windows", "--step", "5"], "--step"),
    (["--translate", "--frame-window", "40", "-e", "1", "--verify-frame-windows", "--verify"], "--verify:"),
    (["--translate", "--frame-window", "40", "-e", "1", "--verify-frame-windows", "--verify-frames"], "--verify-frames"),
    (["--translate", "--frame-window", "40", "-e", "1", "--verify-frame-windows", "--verify-windows"], "--verify-windows"),
    (["--translate", "--frame-window", "40", "-e", "1", "--verify-frame-windows", "--align"], "--align"),
    (["--translate", "--frame-window", "40", "-e", "1", "--verify-frame-windows", "--all-targets"], "--all-targets"),
    (["--translate", "--verify-frame-windows", "-e", "1", "--verify-frames"], "--verify-frame-windows cannot be combined with --verify-frames"),
    (["--translate", "--frame-window", "40", "-e", "2", "--verify"], "--verify-frame-windows"),  # the old refusals point to the new flag
    (["--translate", "--frame-window", "40", "-e", "2", "--verify-windows"], "--verify-frame-windows"),
    (["--translate", "--frame-window", "0", "-e", "1", "--verify-frame-windows"], "--frame-window must be"),
    (["--translate", "--frame-window", "40", "--frame-step", "41", "-e", "1", "--verify-frame-windows"], "--frame-step must be"),
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
    r = subprocess.run([TETREX, "search", "--translate", "--frame-window", "40", "--frame-step", "10", "-e", "2", "--verify-frame-windows", "--counts",
                        str(tmp_path / "none.ibf"), str(tmp_path / "none.fa")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Parser Error" not in r.stderr and "Index not valid" in r.stderr, r.stderr
