"""The size-aware HIBF layout on the CPU (tetrex_amd/csrc/host/layout.hpp through include/txh.h txh_hibf_layout): the numpy
HyperLogLog restatement against known cardinalities, the layout's structural invariants, and what it saves against the
uniform two-level tree on a skewed library."""
import numpy as np
import pytest

from sized_hibf_ref import MERGED, estimate, paths, registers, total_bits, uniform_bits


@pytest.fixture(scope="module")
def host():
    from tetrex_amd import host as h
    return h


@pytest.mark.parametrize("n", [1, 10, 100, 500, 1000])
def test_hll_linear_counting_range(n):
    e = estimate(registers(np.arange(n, dtype=np.uint64) * np.uint64(7919)))
    assert abs(e - n) <= 0.02 * n, (n, e)


@pytest.mark.parametrize("n", [100_000, 300_000, 1_000_000])
def test_hll_large_cardinalities(n):
    v = np.random.default_rng(n).permutation(np.arange(n, dtype=np.uint64) + np.uint64(1 << 33))
    e = estimate(registers(np.concatenate([v, v[: n // 3]])))  # repeated values count once
    assert abs(e - n) <= 0.05 * n, (n, e)


def test_hll_union_is_the_max_of_registers():
    a, b = np.arange(0, 60_000, dtype=np.uint64), np.arange(40_000, 100_000, dtype=np.uint64)
    u = np.maximum(registers(a), registers(b))
    assert np.array_equal(u, registers(np.concatenate([a, b])))
    assert abs(estimate(u) - 100_000) <= 5_000
    assert estimate(registers(np.zeros(0, dtype=np.uint64))) == 0.0


def _disjoint_unions(host, counts, tmax):
    """Union estimates of disjoint bins: the sums of the counts over each run in layout order."""
    B = len(counts)
    order = host.layout_order(counts).astype(np.int64)
    W = host.union_window(B, tmax)
    cum = np.concatenate([[0.0], np.cumsum(np.asarray(counts, dtype=np.float64)[order])])
    U = np.zeros((B, W))
    for L in range(1, W + 1):
        s = np.arange(B - L + 1)
        U[s, L - 1] = cum[s + L] - cum[s]
    return U


def _check(host, counts, tmax=None):
    counts = np.asarray(counts, dtype=np.float64)
    B = counts.size
    tm = tmax or host.default_tmax(B)
    U = _disjoint_unions(host, counts, tm)
    lay = host.hibf_layout(counts, U, tmax=tm)
    ibfs = lay["ibfs"]
    assert np.array_equal(lay["order"], host.layout_order(counts))
    pos = np.empty(B, dtype=np.int64)
    pos[lay["order"].astype(np.int64)] = np.arange(B)
    for f in ibfs:
        assert f["bins"] <= tm and len(f["tb_to_user_bin"]) == f["bins"] and f["bin_size"] >= 1
        for t in range(f["bins"]):  # every technical bin used: a user bin or a merged bin with a child
            u = int(f["tb_to_user_bin"][t])
            assert u == MERGED or u < B
    p = paths(ibfs)  # each user bin: one run of technical bins in one IBF; each child one parent
    assert sorted(p) == list(range(B))
    for ub, steps in p.items():
        for (i, t, parts) in steps[:-1]:
            assert parts == 1 and int(ibfs[i]["tb_to_user_bin"][t]) == MERGED
    # a merged bin's child covers exactly a run of the layout order, and IBF i has T = min(tmax, 64 * ceil(n / 64))
    under = {i: [] for i in range(len(ibfs))}
    for ub, steps in p.items():
        for (i, _, _) in steps:
            under[i].append(pos[ub])
    for i, ps in under.items():
        ps = sorted(ps)
        assert ps == list(range(ps[0], ps[0] + len(ps))), i
        assert ibfs[i]["bins"] == min(tm, 64 * ((len(ps) + 63) // 64)), i
    again = host.hibf_layout(counts, U, tmax=tm)
    assert np.array_equal(again["order"], lay["order"]) and len(again["ibfs"]) == len(ibfs)
    for f, g in zip(ibfs, again["ibfs"]):
        assert f["bin_size"] == g["bin_size"]
        assert np.array_equal(f["next_ibf_id"], g["next_ibf_id"]) and np.array_equal(f["tb_to_user_bin"], g["tb_to_user_bin"])
    return lay, p


@pytest.mark.parametrize("B", [1, 63, 64, 65, 1000, 5000])
def test_layout_invariants_on_lognormal_sizes(host, B):
    counts = np.round(np.random.default_rng(B).lognormal(6, 1.5, size=B))
    _check(host, counts)


@pytest.mark.parametrize("B", [1, 64, 65, 1000])
def test_layout_invariants_on_equal_sizes(host, B):
    _check(host, np.full(B, 500.0))


def test_empty_bins_get_a_technical_bin(host):
    counts = np.random.default_rng(3).lognormal(5, 1, size=300).round()
    counts[::7] = 0
    _, p = _check(host, counts)
    assert all(b in p for b in range(0, 300, 7))


def test_one_giant_bin_is_split_and_tiny_bins_are_merged(host):
    counts = np.full(1000, 50.0)
    counts[417] = 2_000_000.0
    lay, p = _check(host, counts)
    assert p[417][-1][2] > 1 and len(p[417]) == 1  # split, in the root
    merged = sum(1 for ub in p if len(p[ub]) > 1)
    assert merged >= 900  # the tiny bins sit below merged bins
    # one giant bin and many tiny ones under a small t_max: three levels and more
    deep = _check(host, np.concatenate([[1e6], np.full(4999, 20.0)]), tmax=64)[1]
    assert max(len(s) for s in deep.values()) >= 3


def test_bad_inputs_are_refused(host):
    counts = np.full(100, 10.0)
    U = _disjoint_unions(host, counts, 64)
    with pytest.raises(host.HostError):
        host.hibf_layout(counts, U, tmax=100)  # not a multiple of 64
    with pytest.raises(host.HostError):
        host.hibf_layout(counts, U[:, :3], tmax=64)  # wrong window
    bad = counts.copy()
    bad[3] = -1
    with pytest.raises(host.HostError):
        host.hibf_layout(bad, U, tmax=64)


def test_sized_layout_spends_at_most_half_the_uniform_bits_on_a_skewed_library(host):
    """256 bins, 8 of them 100x the size of the others (declared library): the uniform tree sizes every child bin like the
    largest one."""
    counts = np.full(256, 2000.0)
    counts[[3, 40, 77, 101, 150, 199, 230, 255]] = 200_000.0
    lay, _ = _check(host, counts)
    sized, uniform = total_bits(lay["ibfs"]), uniform_bits(list(counts))
    assert sized <= 0.5 * uniform, (sized, uniform)
