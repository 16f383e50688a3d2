"""Approximate matching by edit distance on the CPU: txh_edit_search (host/edit_distance.hpp, multiword
Myers) against the dynamic program restated in tests/edit_ref.py, all three fields of every pair; and the option checks of
`tetrex search --verify`, which are made before the index is read and so need no GPU."""
import os
import subprocess

import numpy as np
import pytest

import edit_cases
import edit_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TETREX = os.path.join(ROOT, "bin", "tetrex")

LENGTHS = list(range(1, 131)) + [511, 512, 513, 700]


@pytest.fixture(scope="module")
def host():
    from tetrex_amd import host as h
    return h


def test_reference_on_cases_worked_by_hand():
    codes = E.letter_codes("ACGT")
    assert E.distance("ACGT", "TTACGTTT", codes) == (0, 6)
    assert E.distance("ACGT", "TTACTTT", codes) == (1, 5)   # ACT for ACGT; "AC" alone would cost 2
    assert E.distance("ACGT", "", codes) == (4, 0)
    assert E.distance("AC#T", "AC#T", codes) == (1, 4)      # '#' matches nothing, not even itself
    assert E.distance("acgt", "ACGT", codes) == (0, 4)
    out = E.search(["ACGT"], ["", "GGAC", "GTGG", "ACGT"], [0, 3, 4, 4], [(0, 0, 1), (0, 0, 2), (0, 1, 0), (0, 2, 9)], codes)
    # "AC" at the end of one record and "GT" at the start of the next are no match: distance 2 in each, the lower record wins
    assert out.tolist() == [[E.NONE] * 3, [2, 1, 4], [0, 3, 4], [E.NONE] * 3]


@pytest.mark.parametrize("alphabet", list(edit_cases.ALPHABETS))
def test_host_equals_reference(host, alphabet):
    patterns, records, groups, pairs, codes = edit_cases.build(LENGTHS, alphabet, seed=len(alphabet), long_bytes=1200)
    want = E.search(patterns, records, groups, pairs, codes)
    for threads in (1, 3):
        got = host.edit_search([p.tobytes() for p in patterns], [r.tobytes() for r in records], groups, pairs, codes, threads=threads)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (alphabet, threads, [(pairs[i], got[i].tolist(), want[i].tolist()) for i in bad[:5]])
    found = want[:, 0] != E.NONE
    assert found.sum() > len(pairs) // 3 and (~found).sum() > len(pairs) // 10
    if alphabet == "dna":  # ties: the same least distance at several ends, and in several records
        recs = [E.as_bytes(r) for r in records]
        ties = 0
        for i in np.flatnonzero(found)[::7][:60]:
            p, g, _ = pairs[i]
            rows = [E.last_rows(E.as_bytes(patterns[p])[None, :], recs[r], codes)[0] for r in range(groups[g], groups[g + 1])]
            ties += sum(int((row == want[i, 0]).sum()) for row in rows) > 1
        assert ties >= 10


def test_host_long_record(host):
    """records of a few thousand bytes (the kernel's chunks are shorter) on both alphabets, m on either side of 64 and 512"""
    for alphabet in edit_cases.ALPHABETS:
        patterns, records, groups, pairs, codes = edit_cases.build([7, 64, 65, 512, 513], alphabet, seed=5, long_bytes=6000)
        assert max(r.size for r in records) > 3000
        want = E.search(patterns, records, groups, pairs, codes)
        got = host.edit_search([p.tobytes() for p in patterns], [r.tobytes() for r in records], groups, pairs, codes, threads=2)
        assert np.array_equal(got, want), alphabet


def test_host_refusals(host):
    codes = E.letter_codes("ACGT")
    for patterns, pairs in ((["ACGT", ""], [(1, 0, 1)]), (["ACGT"], [(1, 0, 1)]), (["ACGT"], [(0, 2, 1)])):
        with pytest.raises(host.HostError):
            host.edit_search(patterns, ["ACGT", "AC"], [0, 1, 2], pairs, codes)
    assert host.edit_search(["ACGT"], ["ACGT", "AC"], [0, 1, 2], [(0, 1, 2)], codes).tolist() == [[2, 1, 2]]


def _run(*args):
    r = subprocess.run([TETREX, *args], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("flags,words", [(["--verify"], ["--verify", "-e"]),
                                         (["--verify", "--threshold", "0.5"], ["--verify", "--threshold"]),
                                         (["--verify", "-e", "2", "--translate"], ["--verify", "--translate"])], ids=str)
def test_cli_refuses_verify_without_its_conditions(tmp_path, flags, words):
    """--verify needs -e and excludes --threshold and --translate: a parser error that names --verify, before the index is
    read (the index named here does not exist), with a non-zero exit"""
    q = tmp_path / "q.fa"
    q.write_text(">a\nACDEFGHIK\n")
    rc, so, se = _run("search", *flags, str(tmp_path / "missing.ibf"), str(q))
    lines = [l for l in se.splitlines() if l.startswith("[Search Parser Error]")]
    assert len(lines) == 1 and "Unknown option" not in se and "Index not valid" not in se and so == "", se
    for w in words:
        assert w in lines[0], se
    assert rc != 0
