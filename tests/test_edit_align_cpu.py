"""Alignments on the CPU: tetrex_amd.host.edit_align (txh_edit_align, host/edit_distance.hpp — the banded host
twin of the kernel) against the full matrix and the three-rule walk of tests/edit_align_ref.py, on generated cases with
patterns of up to 40 letters; the run identities of include/txq.h for every case; the layout of an answer."""
import numpy as np
import pytest

import edit_align_ref as A
import edit_cases
import edit_ref as E

FILL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def host():
    from tetrex_amd import host as h
    return h


def _cases(alphabet, seed):
    """patterns, records, groups and (pattern, group) combinations: per pattern a group whose target lies behind records of
    no bytes; copies with 0..3 edits inside a record, at its very start (the window is clipped) and at its very end; random
    patterns; patterns with nothing in common with their record (d = m: all 'I', an empty match)"""
    letters = edit_cases.ALPHABETS[alphabet]
    rng = np.random.default_rng(seed)
    patterns, records, groups, combos = [], [], [0], []
    for m in [1, 2, 3, 5, 8, 13, 21, 33, 40] * 3:
        for kind in ("inside", "start", "end", "random", "far"):
            p = edit_cases.random_text(rng, letters, m, junk=0.05)
            copy = edit_cases.edited(rng, letters, p, int(rng.integers(0, 4)))
            left, right = (edit_cases.random_text(rng, letters, int(rng.integers(1, 30))) for _ in range(2))
            if kind == "inside":
                target = np.concatenate([left, copy, right])
            elif kind == "start":
                target = np.concatenate([copy, right])
            elif kind == "end":
                target = np.concatenate([left, copy])
            elif kind == "random":
                target = edit_cases.random_text(rng, letters, int(rng.integers(0, 50)))
            else:
                p = np.frombuffer(b"#" * m, dtype=np.uint8)  # no class: matches nothing, itself included
                target = np.concatenate([left, np.frombuffer(b"#" * 3, dtype=np.uint8)])
            records += [np.zeros(0, np.uint8)] * int(rng.integers(0, 3)) + [target, edit_cases.random_text(rng, letters, 4)]
            groups.append(len(records))
            combos.append((len(patterns), len(groups) - 2))
            patterns.append(p)
    return [p.tobytes() for p in patterns], [r.tobytes() for r in records], groups, combos, E.letter_codes(letters)


@pytest.mark.parametrize("alphabet", list(edit_cases.ALPHABETS))
def test_host_twin_matches_the_full_matrix(host, alphabet):
    patterns, records, groups, combos, codes = _cases(alphabet, seed=7 + len(alphabet))
    free = host.edit_search(patterns, records, groups, [(p, g, 1000) for p, g in combos], codes)
    assert (free == E.search(patterns, records, groups, [(p, g, 1000) for p, g in combos], codes)).all()
    pairs = [(p, g, cap) for (p, g), d in zip(combos, free[:, 0].tolist()) for cap in (0, d, d + 1)]
    results = host.edit_search(patterns, records, groups, pairs, codes)
    max_errors = int(free[:, 0].max())
    assert max_errors == 40 and (results[:, 0] == E.NONE).sum() > len(combos) // 2
    starts, runs = host.edit_align(patterns, records, groups, pairs, results, codes, max_errors)
    want_starts, want_runs = A.align_pairs(patterns, records, pairs, results, codes)
    bad = [i for i in range(len(pairs)) if starts[i] != want_starts[i] or runs[i] != want_runs[i]]
    assert not bad, [(pairs[i], results[i].tolist(), int(starts[i]), runs[i], int(want_starts[i]), want_runs[i]) for i in bad[:4]]
    seen = set()
    for (p, _, _), (d, r, j), start, rr in zip(pairs, results.tolist(), starts.tolist(), runs):
        if d == E.NONE:
            assert start == E.NONE and rr == []
            continue
        A.check_identities(len(patterns[p]), d, j, start, rr)
        seen.update(c for c, _ in rr)
        if d == len(patterns[p]) and set(patterns[p]) == {ord("#")}:
            assert rr == [("I", d)] and start == j  # an empty match: no target letter taken
    assert seen == set("=XID")
    assert any(s == 0 and d not in (0, E.NONE) for s, d in zip(starts.tolist(), results[:, 0].tolist()))  # a clipped window
    assert any(j == len(records[r]) and d < len(patterns[p]) for (p, _, _), (d, r, j) in zip(pairs, results.tolist()) if d != E.NONE)


def test_answer_layout_and_what_is_not_aligned(host):
    codes = E.letter_codes("ACGT")
    patterns, records, groups = ["ACGTACGT", "ACGAACGT", "TTTT"], ["", "GGACGTACGTGG", "ACGTTACGT"], [0, 2, 3]
    pairs = [(0, 0, 2), (1, 0, 2), (2, 0, 1), (0, 1, 2), (1, 1, 0)]
    results = host.edit_search(patterns, records, groups, pairs, codes)
    assert results.tolist() == [[0, 1, 10], [1, 1, 10], [E.NONE] * 3, [1, 2, 9], [E.NONE] * 3]
    raw = host.edit_align(patterns, records, groups, pairs, results, codes, 2, raw=True)
    assert raw.shape == (5, 7)
    assert raw[0].tolist() == [2, 1, 8 << 2 | 0, 0, 0, 0, 0]
    assert raw[1].tolist() == [2, 3, 3 << 2 | 0, 1 << 2 | 1, 4 << 2 | 0, 0, 0]
    assert raw[2].tolist() == [E.NONE, 0, 0, 0, 0, 0, 0] and raw[4].tolist() == raw[2].tolist()
    # ACGTTACGT: the walk back prefers the diagonal, so of the two T it is the first that is skipped
    assert raw[3].tolist() == [0, 3, 3 << 2 | 0, 1 << 2 | 3, 5 << 2 | 0, 0, 0]
    assert A.align(patterns[0], records[2], codes) == (1, 9, 0, [("=", 3), ("D", 1), ("=", 5)])
    # the refusal marker of a search call is passed on; d above max_errors, and triples that are no cell of the matrix, are
    # marked and nothing else of their words is written
    odd = np.array([[E.NONE, A.NOT_ALIGNED, A.NOT_ALIGNED], [1, 1, 10], [0, 7, 10], [0, 2, 10], [0, 1, 13], [9, 1, 10], [0, 1, 9],
                    [3, 1, 10], [0, 1, 10]], dtype=np.uint32)
    pairs = [(0, 0, 2)] * 7 + [(1, 0, 5), (0, 0, 2)]
    raw = host.edit_align(patterns, records, groups, pairs, odd, codes, 2, raw=True)
    assert raw[0].tolist() == [E.NONE, A.NOT_ALIGNED, 0, 0, 0, 0, 0]
    for i in range(1, 8):  # D[8][10] is 0, not 1; record 7 does not exist; record 2 is outside the group; j beyond the record; ...
        assert raw[i].tolist() == [A.NOT_ALIGNED] + [FILL] * 6, i
    assert raw[8].tolist() == [2, 1, 8 << 2, 0, 0, 0, 0]
    raw = host.edit_align(patterns, records, groups, [(1, 0, 2)], [[1, 1, 10]], codes, 0, raw=True)
    assert raw.tolist() == [[A.NOT_ALIGNED, FILL, FILL]]  # d = 1 > max_errors = 0
