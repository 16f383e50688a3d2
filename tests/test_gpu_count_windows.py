"""GPU parity of the sliding window count (include/txq.h txq_count_windows, `tetrex search --window`): the windows written
out as duplicated disjoint queries go through the numpy restatement of tests/search_ref.py, and every hit mask and every
count of Index.count_windows must equal it bit for bit — on flat IBFs (the sliding kernel), column shards and regular,
layout-shaped and split-heavy HIBFs (the windows as independent queries).  The window sets are those of
tests/native/count_windows_sim.cpp, 5000 windows of 64 values at step 1 (many unit boundaries) and 12 windows of 10 000
values at step 1000 (a window far longer than one pass of the workgroup); then more units than the kernel has workgroups
and more windows than an HIBF level has waves, where a workgroup's second item starts on what its first one left in LDS."""
import numpy as np
import pytest

from helpers import random_words, oracle_ibf_from_words, regular_hibf, layout_hibf, split_heavy_hibf, splitmix64
from search_ref import TreeRef, flat_search, csr
from test_gpu_search import thresholds_for

pytestmark = pytest.mark.gpu

ROWS = 1031
FLAT = [(5, 1), (64, 2), (1000, 3), (9000, 5)]  # (9000: two column tiles, the second partial)


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


def sliding(length, step, n):
    return np.arange(n, dtype=np.uint64) * np.uint64(step), np.full(n, length, dtype=np.uint32)


def sim_window_sets():
    """the window sets of tests/native/count_windows_sim.cpp, as (begins, lens)"""
    sets = []
    for length in (0, 1, 63, 64, 65, 300):
        for step in (1, 7, length, length + 5):
            for n in (0, 1, 37, 130):
                sets.append(sliding(length, step, n))
    b, e, bs, ls = 0, 80, [], []  # a length that shrinks, then grows
    for j in range(50):
        bs.append(b), ls.append(e - b)
        b, e = (b + 3, e + 1) if j < 25 else (b + 1, e + 6)
    sets.append((np.array(bs, dtype=np.uint64), np.array(ls, dtype=np.uint32)))
    for total in (101, 149, 150, 151):  # the end-aligned tail window
        bs = list(range(0, total - 50 + 1, 25))
        if bs[-1] + 50 < total:
            bs.append(total - 50)
        sets.append((np.array(bs, dtype=np.uint64), np.full(len(bs), 50, dtype=np.uint32)))
    sets.append((np.array([(j // 3) * 9 for j in range(40)], dtype=np.uint64), np.full(40, 70, dtype=np.uint32)))  # repeated
    bs = [(j // 2) * 30 + (25 if j % 2 else 0) for j in range(41)]  # gaps, an empty window in each
    sets.append((np.array(bs, dtype=np.uint64), np.array([0 if j % 2 else 20 for j in range(41)], dtype=np.uint32)))
    return sets


def joined(sets):
    """Several window sets as ONE sliding sequence over one value array: each set moved behind the end of the one before
    (so that set boundaries are further non-overlapping steps).  Empty sets vanish; they are run on their own."""
    bs, ls, base = [], [], 0
    for b, n in sets:
        if b.size == 0:
            continue
        bs.append(b + np.uint64(base))
        ls.append(n)
        base += int((b + n.astype(np.uint64)).max())
    return np.concatenate(bs), np.concatenate(ls)


def sim_small():
    """a cut of the simulator's sets for the widest index: one set of every kind, about 25 000 values in all"""
    sets = [sliding(65, 7, 130), sliding(300, 1, 37), sliding(64, 64, 37), sliding(63, 68, 37), sliding(1, 1, 37), sliding(0, 5, 37)]
    return joined(sets + sim_window_sets()[-7:])  # ... and the shrinking, tail, repeated and gap sets


WINDOW_SETS = {
    "sim": lambda: joined(sim_window_sets()),
    "sim_small": sim_small,
    "empty": lambda: sliding(64, 1, 0),
    "one": lambda: sliding(64, 1, 1),
    "many": lambda: sliding(64, 1, 5000),
    "long": lambda: sliding(10000, 1000, 12),
}


def mid_unit_resets():
    """270 000 windows of 16 values: 1000 times 263 windows at step 4, then 4 at step 16 (each begins at the end of the one
    before) and 3 at step 20 (gaps): the windows that do not slide fall on every position of a unit of 16"""
    return joined([sliding(16, 4, 263), sliding(16, 16, 4), sliding(16, 20, 3)] * 1000)


SCALE_SETS = {  # more units than count_windows_kernel has workgroups (test_flat_more_units_than_workgroups)
    "units_of_one": lambda: sliding(24, 3, 20000),
    "mid_unit_resets": mid_unit_resets,
}


def restated(bins, name):
    """The numpy restatement takes 0.14 ms per value of the written-out windows on the 9000-bin index (45 s for the
    simulator's sets, 41 s for the 5000 windows): there it answers the cut sim_small, and the larger sets are held to what
    txq_count itself — code this feature does not touch, which tests/test_gpu_search.py holds to the restatement — says of the
    written-out windows, which is the definition of the result (include/txq.h).  The narrower indexes are restated in full."""
    return bins <= 1000 or name in ("sim_small", "empty", "one")


def expanded(values, begins, lens):
    """the windows as duplicated disjoint queries: (values, offsets) of txq_count"""
    return csr([values[int(b):int(b) + int(n)] for b, n in zip(begins, lens)])


def window_thresholds(lens, shift=0):
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.asarray(lens, dtype=np.uint64))
    return thresholds_for(off, shift)


_flat_cache = {}


def flat_case(oracle, capi, bins, h, name):
    """index words, windows and the expected answer, computed once per (index, window set) and left unchanged"""
    key = (bins, h, name)
    if key not in _flat_cache:
        words = random_words(bins, ROWS, 0.5, bins + h)
        begins, lens = {**WINDOW_SETS, **SCALE_SETS}[name]()
        n_values = int((begins + lens.astype(np.uint64)).max()) if begins.size else 10
        values = splitmix64(bins * 31 + len(name), n_values + 3)  # (three values behind the last window)
        thr = window_thresholds(lens, shift=bins % 5)
        ev, eo = expanded(values, begins, lens)
        if begins.size == 0:  # (no windows: the restatement has nothing to reshape; the answer is two arrays of no rows)
            want_hits, want_counts = np.zeros((0, (bins + 63) // 64), dtype=np.uint64), np.zeros((0, (bins + 63) // 64 * 64), dtype=np.int64)
        elif restated(bins, name):
            want_hits, want_counts = flat_search(oracle_ibf_from_words(oracle, bins, ROWS, h, words), bins, ev, eo, thr)
        else:
            ix = capi.Index.upload_ibf(bins, ROWS, h, words)
            want_hits, want_counts = ix.count(ev, eo, thr, counts=True)
            ix.free()
        for a in (words, values, begins, lens, thr, want_hits, want_counts):
            a.setflags(write=False)
        _flat_cache[key] = (words, values, begins, lens, thr, want_hits, want_counts)
    return _flat_cache[key]


@pytest.mark.parametrize("name", list(WINDOW_SETS))
@pytest.mark.parametrize("bins,h", FLAT)
def test_flat_windows_match_restatement(capi, oracle, bins, h, name):
    words, values, begins, lens, thr, want_hits, want_counts = flat_case(oracle, capi, bins, h, name)
    ix = capi.Index.upload_ibf(bins, ROWS, h, words)
    hits, counts = ix.count_windows(values, begins, lens, thr, counts=True)
    assert hits.shape == (begins.size, ix.shard_words) and counts.shape == (begins.size, 64 * ix.shard_words)
    assert np.array_equal(counts, want_counts), (bins, h, name)
    assert np.array_equal(hits, want_hits), (bins, h, name)
    assert np.array_equal(ix.count_windows(values, begins, lens, thr), hits)  # without counts: the same hits
    if begins.size and restated(bins, name):  # ... and what txq_count itself says of the written-out windows
        ev, eo = expanded(values, begins, lens)
        h2, c2 = ix.count(ev, eo, thr, counts=True)
        assert np.array_equal(h2, hits) and np.array_equal(c2, counts)
    if name == "many":  # (non-vacuity: real thresholds are reached and missed)
        assert hits[thr == 1].any() and not hits[thr == 65].any() and counts.max() > 1
    ix.free()


@pytest.mark.parametrize("bins,h,name", [(1000, 3, "sim"), (1000, 3, "many"), (9000, 5, "sim_small"), (9000, 5, "many")])
def test_unit_and_waves_knobs_give_identical_arrays(capi, oracle, monkeypatch, bins, h, name):
    words, values, begins, lens, thr, want_hits, want_counts = flat_case(oracle, capi, bins, h, name)
    ix = capi.Index.upload_ibf(bins, ROWS, h, words)
    for unit, waves in (("1", "1"), ("3", "1"), ("64", "1"), ("1", "4"), ("3", "4"), ("16", "4"), ("64", "4")):
        monkeypatch.setenv("TXQ_COUNT_WINDOWS_UNIT", unit)
        monkeypatch.setenv("TXQ_COUNT_WINDOWS_WAVES", waves)
        hits, counts = ix.count_windows(values, begins, lens, thr, counts=True)
        assert np.array_equal(counts, want_counts), (unit, waves)
        assert np.array_equal(hits, want_hits), (unit, waves)
    ix.free()


COUNT_WINDOWS_GRID = 4096 * 4  # txq_count.hip count_windows_flat: grid = min(cw_units(n, U) * n_tiles, kCountGrid * 4)
COUNT_WINDOWS_UNIT = 16        # txq_count_windows_plan.hpp kCountWindowsUnitDefault


@pytest.mark.parametrize("bins,h,name,unit,waves", [(64, 2, "units_of_one", 1, 1), (64, 2, "units_of_one", 1, 4), (40, 2, "mid_unit_resets", None, None)])
def test_flat_more_units_than_workgroups(capi, oracle, monkeypatch, bins, h, name, unit, waves):
    """More units than the 16 384 workgroups of count_windows_kernel: a workgroup's second unit begins on the LDS counters
    its first one left behind (they are never cleared when read), so its first window must reset them.  20 000 units of one
    window, with one wave and with four; and 16 875 units of the default 16 windows, with windows that begin at or behind the
    end of the one before (cw_step: reset) on every position inside a unit."""
    for knob, value in (("TXQ_COUNT_WINDOWS_UNIT", unit), ("TXQ_COUNT_WINDOWS_WAVES", waves)):
        if value is None:
            monkeypatch.delenv(knob, raising=False)
        else:
            monkeypatch.setenv(knob, str(value))
    words, values, begins, lens, thr, want_hits, want_counts = flat_case(oracle, capi, bins, h, name)
    U = unit or COUNT_WINDOWS_UNIT
    n_units, n_tiles = -(-begins.size // U), 1  # txq_count_windows_plan.hpp cw_units; one column tile up to 8192 bins
    assert n_units * n_tiles > COUNT_WINDOWS_GRID, (n_units, n_tiles)  # count_windows_kernel: work < n_units * n_tiles, work += gridDim.x
    if name == "mid_unit_resets":
        ends = begins + lens.astype(np.uint64)
        at = np.flatnonzero(begins[1:] >= ends[:-1]) + 1  # windows that share nothing with the one before
        assert set((at % U).tolist()) == set(range(U)) and (at % U != 0).sum() > 5000
    assert want_hits.any() and not (want_hits == np.uint64((1 << bins) - 1)).all() and want_counts.max() > 1
    ix = capi.Index.upload_ibf(bins, ROWS, h, words)
    hits, counts = ix.count_windows(values, begins, lens, thr, counts=True)
    assert np.array_equal(counts, want_counts), (bins, h, name)
    assert np.array_equal(hits, want_hits), (bins, h, name)
    assert np.array_equal(ix.count_windows(values, begins, lens, thr), hits)  # without counts: the same hits
    ix.free()
    if name == "mid_unit_resets":
        del _flat_cache[bins, h, name]  # (140 MB of expected counts that no other test asks for)


@pytest.mark.parametrize("bins,h,name", [(1000, 3, "sim"), (9000, 5, "sim_small"), (9000, 5, "long")])
def test_flat_column_shards_join(capi, oracle, bins, h, name):
    words, values, begins, lens, thr, want_hits, want_counts = flat_case(oracle, capi, bins, h, name)
    for R in (2, 3):
        got_h, got_c = [], []
        for r in range(R):
            ix = capi.Index.upload_ibf(bins, ROWS, h, words, shard_rank=r, n_shards=R)
            hits, counts = ix.count_windows(values, begins, lens, thr, counts=True)
            w0, W = int(ix.info.shard_word0), ix.shard_words
            assert np.array_equal(hits, want_hits[:, w0:w0 + W]), (R, r)
            assert np.array_equal(counts, want_counts[:, 64 * w0:64 * (w0 + W)]), (R, r)
            got_h.append(hits)
            got_c.append(counts)
            ix.free()
        assert np.array_equal(np.concatenate(got_h, axis=1), want_hits)
        assert np.array_equal(np.concatenate(got_c, axis=1), want_counts)


def make_tree(oracle, name):
    rng = np.random.default_rng(3)
    if name == "regular":
        return regular_hibf(oracle, 1024, 16, 60, lambda b: rng.integers(0, 1 << 20, size=60, dtype=np.uint64), h=2)
    if name == "layout":
        return layout_hibf(oracle, 5, user_bins=900, tmax=64, n_values=30)
    return split_heavy_hibf(oracle, 7)[:3]


def tree_windows(values, seed, n_values=600):
    """windows of 20 to 40 values sliding at step 5 over a concatenation of user bins' own values"""
    rng = np.random.default_rng(seed)
    parts, total = [], 0
    while total < n_values:  # (bins of a few values each: more of them)
        parts.append(np.asarray(values[int(rng.integers(0, len(values)))], dtype=np.uint64))
        total += parts[-1].size
    v = np.concatenate(parts)
    begins = np.arange(0, v.size - 40, 5, dtype=np.uint64)
    ends = np.maximum.accumulate(begins + rng.integers(20, 41, size=begins.size).astype(np.uint64))  # (ends do not decrease)
    return v, begins, (ends - begins).astype(np.uint32)


@pytest.mark.parametrize("tree", ["regular", "layout", "split_heavy"])
def test_hibf_windows_match_restatement(capi, oracle, tree):
    ox, descs, values = make_tree(oracle, tree)
    user_bins = len(values)
    ref = TreeRef(oracle, user_bins, descs)
    v, begins, lens = tree_windows(values, len(tree))
    assert lens.min() >= 20 and lens.max() <= 45 and begins.size > 20
    ev, eo = expanded(v, begins, lens)
    ix = capi.Index.upload_hibf(user_bins, descs)
    any_hit = False
    for shift in range(5):
        thr = window_thresholds(lens, shift)
        want_hits, want_counts = ref.search(ev, eo, thr)
        hits, counts = ix.count_windows(v, begins, lens, thr, counts=True)
        assert np.array_equal(hits, want_hits), (tree, shift)
        assert np.array_equal(counts, want_counts), (tree, shift)
        assert np.array_equal(ix.count_windows(v, begins, lens, thr), hits)
        any_hit |= bool(want_hits[thr > 1].any())
    assert any_hit  # (windows over a bin's own values reach real thresholds)
    ix.free()
    if tree == "layout":  # column shards of the tree concatenate to the unsharded answer
        for R in (2, 3):
            hs, cs = [], []
            for r in range(R):
                sh = capi.Index.upload_hibf(user_bins, descs, shard_rank=r, n_shards=R)
                a, b = sh.count_windows(v, begins, lens, thr, counts=True)
                hs.append(a)
                cs.append(b)
                sh.free()
            assert np.array_equal(np.concatenate(hs, axis=1), want_hits), R
            assert np.array_equal(np.concatenate(cs, axis=1), want_counts), R


def test_hibf_more_windows_than_waves(capi, oracle):
    """5000 windows on the 900-bin layout tree: the windows reach count_hibf as queries with their own lengths (CountOut::lens),
    level 0 has more than 4096 (window, root) items on 4096 waves, and a deeper level more than 4096 pairs."""
    ox, descs, values = make_tree(oracle, "layout")
    user_bins = len(values)
    ref = TreeRef(oracle, user_bins, descs)
    v, begins, lens = tree_windows(values, 17, n_values=25_100)
    assert begins.size > 5000 > 4096  # txq_count.hip count_hibf: grid = lvl ? kCountGrid : min(nq, kCountGrid), kCountGrid = 4096
    ev, eo = expanded(v, begins, lens)
    thr = window_thresholds(lens, 2)
    want_hits, want_counts = ref.search(ev, eo, thr)
    assert ref.level_pairs[0] == begins.size and max(ref.level_pairs[1:]) > 4096, ref.level_pairs
    assert want_hits[thr > 1].any() and not want_hits[thr > lens].any()
    ix = capi.Index.upload_hibf(user_bins, descs)
    hits, counts = ix.count_windows(v, begins, lens, thr, counts=True)
    assert np.array_equal(hits, want_hits)
    assert np.array_equal(counts, want_counts)
    assert np.array_equal(ix.count_windows(v, begins, lens, thr), hits)
    ix.free()


def test_refusals(capi, oracle):
    """What the raw library refuses, before anything is launched: every call returns -1 and leaves the result buffers alone."""
    L = capi.lib()
    u64p, u32p = capi.u64p, capi.u32p
    words = random_words(64, ROWS, 0.5, 1)
    ix = capi.Index.upload_ibf(64, ROWS, 2, words)
    values = splitmix64(1, 100)
    thr = np.ones(3, dtype=np.uint32)

    def call(begins, lens, n_values=100, v=values, t=thr, with_hits=True):
        b = np.array(begins if begins is not None else [], dtype=np.uint64)
        n = np.array(lens if lens is not None else [], dtype=np.uint32)
        hits = np.full((3, ix.shard_words), 0xABCD, dtype=np.uint64)
        rc = L.txq_count_windows(ix._h, v.ctypes.data_as(u64p) if v is not None else None, n_values, b.ctypes.data_as(u64p) if begins is not None else None,
                                 n.ctypes.data_as(u32p) if lens is not None else None, 3, t.ctypes.data_as(u32p) if t is not None else None,
                                 hits.ctypes.data_as(u64p) if with_hits else None, None)
        capi.synchronize()
        assert (hits == 0xABCD).all() or rc == 0
        return rc

    assert call([0, 10, 20], [30, 30, 30]) == 0
    assert call([0, 20, 10], [30, 40, 60]) == -1       # descending begin
    assert call([0, 10, 20], [30, 30, 15]) == -1       # descending begin + len
    assert call([0, 10, 80], [30, 30, 21]) == -1       # a window past n_values
    assert call([0, 10, 20], [30, 30, 30], n_values=49) == -1
    assert call([0, 10, 101], [30, 30, 0]) == -1
    assert call([0, 10, 20], [30, 30, 30], v=None) == -1
    assert call(None, [30, 30, 30]) == -1
    assert call([0, 10, 20], None) == -1
    assert call([0, 10, 20], [30, 30, 30], t=None) == -1
    assert call([0, 10, 20], [30, 30, 30], with_hits=False) == -1
    assert L.txq_count_windows(None, None, 0, None, None, 0, None, None, None) == -1
    assert L.txq_count_windows_device(ix._h, None, None, None, 1, None, None, None, None) == -1
    with pytest.raises(capi.TxqError) as e:            # the wrapper's own check
        ix.count_windows(values, [0, 10, 80], [30, 30, 21], thr)
    assert e.value.code == -1
    ix.free()
    ox, descs, tv = layout_hibf(oracle, 5, user_bins=900, tmax=64, n_values=30)
    sub = capi.Index.upload_hibf(900, descs, shard_rank=0, n_shards=2, subtrees=True)
    assert sub.info.join_or == 1
    with pytest.raises(capi.TxqError) as e:
        sub.count_windows(values, [0, 10, 20], [30, 30, 30], thr)
    assert e.value.code == -1
    sub.free()
