"""The similarity rearrangement of `tetrex index --layout sized --rearrange` on the CPU: the interval and chain rules
(tetrex_amd/csrc/host/layout.hpp through include/txh.h) against their numpy restatement (rearrange_ref.py), the layout over
a given order, and what the rule saves on a library of families."""
import numpy as np
import pytest

import rearrange_ref as RR
from sized_hibf_ref import estimate, paths, registers, total_bits, union_table


@pytest.fixture(scope="module")
def host():
    from tetrex_amd import host as h
    return h


def _random_counts(rng, B, kind):
    if kind == "lognormal":
        return np.round(rng.lognormal(6, 1.5, size=B))
    if kind == "equal":
        return np.full(B, 500.0)
    if kind == "zeros":
        c = np.round(rng.lognormal(5, 1, size=B))
        c[rng.random(B) < 0.3] = 0
        return c
    if kind == "all zero":
        return np.zeros(B)
    return np.round(rng.lognormal(4, 0.2, size=B) / 10) * 10  # many equal counts


@pytest.mark.parametrize("kind", ["lognormal", "equal", "zeros", "all zero", "ties"])
@pytest.mark.parametrize("ratio", [0.25, 0.5, 1.0])
def test_intervals_equal_the_restatement(host, kind, ratio):
    rng = np.random.default_rng(7)
    for B in (1, 2, 3, 10, 257, 1000):
        counts = _random_counts(rng, B, kind)
        order = RR.sorted_order(counts)
        assert order == [int(b) for b in host.layout_order(counts)]
        for max_len in (None, 1, 2, 5, 64):
            want = RR.intervals(counts, order, ratio, max_len or RR.MAX_LEN)
            got = host.rearrange_intervals(counts, ratio, max_len)
            assert [int(s) for s in got] == want, (kind, ratio, B, max_len)
            ends = want[1:] + [B]
            assert want[0] == 0 and all(1 <= e - s <= (max_len or RR.MAX_LEN) for s, e in zip(want, ends))
    # the cut by max_len happens: equal counts would all share one interval
    assert [int(s) for s in host.rearrange_intervals(np.full(10, 3.0), ratio, 4)] == [0, 4, 8]
    assert [int(s) for s in host.rearrange_intervals(np.full(10, 3.0), ratio)] == [0]


def test_intervals_follow_the_ratio(host):
    counts = np.array([100.0, 60.0, 50.0, 49.0, 30.0, 24.0, 0.0, 0.0])
    assert [int(s) for s in host.rearrange_intervals(counts, 0.5)] == [0, 3, 5, 6]  # 50 >= 50; 49 starts; 24 < 24.5; 0 < 12
    assert [int(s) for s in host.rearrange_intervals(counts, 1.0)] == [0, 1, 2, 3, 4, 5, 6]  # only equal counts share
    assert [int(s) for s in host.rearrange_intervals(counts, 0.25)] == [0, 5, 6]


@pytest.mark.parametrize("bad", [0.0, -0.5, 1.5, float("nan")])
def test_bad_ratios_and_lengths_are_refused(host, bad):
    with pytest.raises(host.HostError):
        host.rearrange_intervals(np.full(5, 2.0), bad)
    with pytest.raises(host.HostError):
        host.rearrange_intervals(np.full(5, 2.0), 0.5, host.REARRANGE_MAX_LEN + 1)
    with pytest.raises(host.HostError):
        host.rearrange_intervals(np.array([1.0, -1.0]), 0.5)


def _symmetric(rng, c, kind):
    n = c.size
    if kind == "random":
        u = rng.uniform(0.5, 2.0, size=(n, n)) * np.maximum(c[:, None], c[None, :])
    elif kind == "integers":  # many equal J
        u = np.maximum(c[:, None], c[None, :]) + rng.integers(0, 3, size=(n, n)) * 10.0
    else:  # zeros among the unions
        u = rng.uniform(0.5, 2.0, size=(n, n)) * np.maximum(c[:, None], c[None, :])
        u[rng.random((n, n)) < 0.3] = 0.0
    u = np.triu(u) + np.triu(u, 1).T
    u[np.arange(n), np.arange(n)] = c
    return u


@pytest.mark.parametrize("kind", ["random", "integers", "zeros"])
def test_chain_equals_the_restatement(host, kind):
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 4, 17, 100, 300):
        for counts_kind in ("lognormal", "equal", "zeros"):
            c = np.sort(_random_counts(rng, n, counts_kind))[::-1].copy()
            u = _symmetric(rng, c, kind)
            got = [int(p) for p in host.rearrange_chain(c, u)]
            assert got == RR.chain(c, u), (kind, n, counts_kind)
            assert sorted(got) == list(range(n)) and got[0] == 0
            if n <= 2:
                assert got == list(range(n))


def test_chain_ties_go_to_the_smaller_position(host):
    # equal rows: every candidate has the same J at every step, so the chain is the identity
    n = 9
    c = np.full(n, 100.0)
    u = np.full((n, n), 150.0)
    assert [int(p) for p in host.rearrange_chain(c, u)] == list(range(n)) == RR.chain(c, u)
    # two groups of equal bins: from 0 the chain takes its own group in ascending position, then the other one
    group = [0, 1, 0, 1, 0, 1, 0]
    u = np.array([[100.0 if group[i] == group[j] else 200.0 for j in range(7)] for i in range(7)])
    c = np.full(7, 100.0)
    assert [int(p) for p in host.rearrange_chain(c, u)] == [0, 2, 4, 6, 1, 3, 5] == RR.chain(c, u)
    # all unions zero: J = 0 everywhere
    assert [int(p) for p in host.rearrange_chain(np.zeros(5), np.zeros((5, 5)))] == list(range(5))


def _disjoint_unions(host, counts, tmax, order):
    B = len(counts)
    W = host.union_window(B, tmax)
    cum = np.concatenate([[0.0], np.cumsum(np.asarray(counts, dtype=np.float64)[np.asarray(order, dtype=np.int64)])])
    U = np.zeros((B, W))
    for L in range(1, W + 1):
        s = np.arange(B - L + 1)
        U[s, L - 1] = cum[s + L] - cum[s]
    return U


def _same_layout(a, b):
    assert a["tmax"] == b["tmax"] and a["window"] == b["window"]
    assert np.array_equal(a["order"], b["order"]) and len(a["ibfs"]) == len(b["ibfs"])
    for f, g in zip(a["ibfs"], b["ibfs"]):
        assert f["bins"] == g["bins"] and f["bin_size"] == g["bin_size"]
        assert np.array_equal(f["next_ibf_id"], g["next_ibf_id"]) and np.array_equal(f["tb_to_user_bin"], g["tb_to_user_bin"])


@pytest.mark.parametrize("tmax", [64, 128])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1000, 2500])
def test_layout_over_the_sorted_order_is_the_layout(host, B, tmax):
    rng = np.random.default_rng(B)
    for counts in (np.round(rng.lognormal(6, 1.5, size=B)), np.full(B, 500.0)):
        order = host.layout_order(counts)
        U = _disjoint_unions(host, counts, tmax, order)
        _same_layout(host.hibf_layout(counts, U, tmax=tmax), host.hibf_layout(counts, U, tmax=tmax, order=order))


def _depth_first_bins(ibfs):
    """User bins in the order a depth-first walk of the tree meets them (a split bin once)."""
    out = []

    def walk(i):
        last = None
        for t, ub in enumerate(ibfs[i]["tb_to_user_bin"]):
            ub = int(ub)
            if ub == 0xFFFFFFFFFFFFFFFF:
                walk(int(ibfs[i]["next_ibf_id"][t]))
                last = None
            elif ub != last:
                out.append(ub)
                last = ub
    walk(0)
    return out


@pytest.mark.parametrize("tmax", [64, 128])
@pytest.mark.parametrize("B", [3, 65, 1000])
def test_layout_over_a_rearranged_order(host, B, tmax):
    rng = np.random.default_rng(B + tmax)
    counts = np.round(rng.lognormal(6, 1.5, size=B))
    counts[::9] = 0
    order = RR.sorted_order(counts)
    starts = RR.intervals(counts, order, 0.5, 50)
    final = list(order)
    for s, e in zip(starts, starts[1:] + [B]):  # any permutation inside the intervals
        final[s:e] = [order[s + p] for p in rng.permutation(e - s)]
    U = _disjoint_unions(host, counts, tmax, final)
    lay = host.hibf_layout(counts, U, tmax=tmax, order=final)
    assert [int(b) for b in lay["order"]] == final
    p = paths(lay["ibfs"])
    assert sorted(p) == list(range(B))
    assert _depth_first_bins(lay["ibfs"]) == final


def test_an_order_that_is_no_permutation_is_refused(host):
    counts = np.full(100, 10.0)
    order = list(range(100))
    U = _disjoint_unions(host, counts, 64, order)
    host.hibf_layout(counts, U, tmax=64, order=order)
    for bad in (order[:50] + order[:50], order[:99] + [100], order[:99] + [0], order[:99]):
        with pytest.raises(host.HostError):
            host.hibf_layout(counts, U, tmax=64, order=bad)


def family_library(rng, families, members, core, own):
    """Registers of families * members bins: every bin holds its family's core (core * U(0.7, 1.3) random values) and
    own * U(0.5, 1.5) values of its own.  Returns (registers, family of each bin)."""
    regs = np.zeros((families * members, 4096), dtype=np.uint8)
    fam = []
    for f in range(families):
        rc = registers(rng.integers(0, 1 << 63, size=int(core * rng.uniform(0.7, 1.3)), dtype=np.uint64))
        for m in range(members):
            mine = rng.integers(0, 1 << 63, size=int(own * rng.uniform(0.5, 1.5)), dtype=np.uint64)
            regs[f * members + m] = np.maximum(rc, registers(mine))
            fam.append(f)
    return regs, fam


def test_rearrangement_saves_bits_on_a_library_of_families(host):
    """256 bins, 32 families of 8, core 20 000 +- 30 %, 5 000 +- 50 % own values each; t_max 64 (window 16), ratio 0.5."""
    regs, fam = family_library(np.random.default_rng(1), 32, 8, 20_000, 5_000)
    B, tmax = len(fam), 64
    counts = np.array([estimate(r) for r in regs])
    W = host.union_window(B, tmax)
    assert W == 16
    sorted_ = RR.sorted_order(counts)
    before = host.hibf_layout(counts, union_table(regs, sorted_, W), tmax=tmax)
    table = RR.pair_unions(regs, range(B))
    final, starts = RR.rearranged_order(counts, regs, 0.5, pairs=lambda _, ids: table[np.ix_(ids, ids)])
    # the host's rule on the same tables gives the same order
    got = list(sorted_)
    hs = [int(s) for s in host.rearrange_intervals(counts, 0.5)]
    assert hs == starts
    for s, e in zip(hs, hs[1:] + [B]):
        ids = sorted_[s:e]
        got[s:e] = [ids[int(p)] for p in host.rearrange_chain(counts[ids], table[np.ix_(ids, ids)])]
    assert got == final and sorted(final) == list(range(B))
    after = host.hibf_layout(counts, union_table(regs, final, W), tmax=tmax, order=final)
    assert _depth_first_bins(after["ibfs"]) == final

    def neighbours(order):
        return sum(fam[order[i]] == fam[order[i + 1]] for i in range(B - 1))

    b0, b1 = total_bits(before["ibfs"]), total_bits(after["ibfs"])
    print("family library: %d bits sorted, %d bits rearranged, ratio %.3f; same-family neighbours %d -> %d of %d"
          % (b0, b1, b1 / b0, neighbours(sorted_), neighbours(final), B - 1))
    assert b1 < b0
    assert 2 * neighbours(final) >= B - 1
