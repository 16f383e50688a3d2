"""Every target of a pair on the CPU: txh_edit_targets (host/edit_distance.hpp) against the dynamic program
restated in tests/edit_ref.py, record by record, against txh_edit_search with every record a group of its own, and the
consistency rule — the least hit of a pair is what txh_edit_search answers on the real group."""
import numpy as np
import pytest

import edit_cases
import edit_ref as E
import edit_targets_ref as T

LENGTHS = [1, 2, 63, 64, 65, 130, 513]


@pytest.fixture(scope="module")
def host():
    from tetrex_amd import host as h
    return h


@pytest.fixture(scope="module", params=list(edit_cases.ALPHABETS))
def case(request):
    patterns, records, groups, pairs, codes = edit_cases.build(LENGTHS, request.param, seed=11 + len(request.param), long_bytes=1200)
    return [p.tobytes() for p in patterns], [r.tobytes() for r in records], groups, pairs, codes


def _same(got, want):
    assert got.shape == want.shape, (got.shape, want.shape, got[:4].tolist(), want[:4].tolist())
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, [(got[i].tolist(), want[i].tolist()) for i in bad[:5]]


def test_host_targets_equal_reference_per_record(host, case):
    patterns, records, groups, pairs, codes = case
    single_groups, single, owner = T.expand(groups, pairs)
    want = T.hits_of(E.search(patterns, records, single_groups, single, codes), owner)
    for threads in (1, 3):
        got, total = host.edit_targets(patterns, records, groups, pairs, codes, threads=threads)
        assert total == want.shape[0]
        _same(got, want)
    # the same from the search that was there before, every record a group of its own
    _same(T.hits_of(host.edit_search(patterns, records, single_groups, single, codes), owner), want)
    # conditions that keep this from passing on nothing
    counts = T.per_pair_counts(want, len(pairs))
    assert (counts >= 1).sum() >= len(pairs) / 3 and (counts >= 2).sum() >= len(pairs) / 5 and (counts == 0).sum() >= len(pairs) / 10
    empty = {r for r, rec in enumerate(records) if len(rec) == 0}
    assert any(int(r) in empty and j == 0 for _, _, r, j in want.tolist())  # m <= e: an empty record is the hit (m, r, 0)


def test_least_hit_is_the_search_answer(host, case):
    patterns, records, groups, pairs, codes = case
    got, _ = host.edit_targets(patterns, records, groups, pairs, codes)
    want = host.edit_search(patterns, records, groups, pairs, codes)
    assert np.array_equal(T.least(got, len(pairs)), want)
    assert (want[:, 0] == E.NONE).sum() >= len(pairs) // 10


def test_capacity_and_refusals(host):
    codes = E.letter_codes("ACGT")
    patterns, records, groups = ["ACGT", "AC"], ["ACGT", "", "TTACTT", "GG"], [0, 3, 4, 4]
    pairs = [(0, 0, 1), (1, 0, 2), (0, 1, 4), (0, 2, 9)]
    full, total = host.edit_targets(patterns, records, groups, pairs, codes)
    assert full.tolist() == [[0, 0, 0, 4], [0, 1, 2, 5], [1, 0, 0, 2], [1, 2, 1, 0], [1, 0, 2, 4], [2, 3, 3, 1]] and total == 6
    for capacity in (0, 1, 5, 6, 9):
        got, total = host.edit_targets(patterns, records, groups, pairs, codes, capacity=capacity)
        assert total == 6 and got.tolist() == full[:capacity].tolist()
    for bad_patterns, bad_pairs in ((["ACGT", ""], [(1, 0, 1)]), (["ACGT"], [(1, 0, 1)]), (["ACGT"], [(0, 3, 1)])):
        with pytest.raises(host.HostError):
            host.edit_targets(bad_patterns, records, groups, bad_pairs, codes)
    got, total = host.edit_targets(["A" * 5000], ["A" * 4999, "C" * 10, "A" * 5001], [0, 3], [(0, 0, 1)], codes)  # no limit on m
    assert got.tolist() == [[0, 1, 0, 4999], [0, 0, 2, 5000]] and total == 2
