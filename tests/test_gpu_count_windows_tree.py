"""GPU parity of the sliding window count on an HIBF (include/txq.h txq_count_windows; csrc/txq_count.hip
count_windows_tree_kernel): hits and counts of Index.count_windows equal the numpy restatement of the written-out
windows bit for bit for every unit size and for TXQ_COUNT_WINDOWS_TREE=0, and txq_count_windows_trace equals the restated item
walk (tests/count_windows_tree_ref.py) exactly — visits, values added, values subtracted, items.  Four trees: a regular one
whose root and children differ in their hash counts, a layout-shaped one with one-word rows, the split-heavy one (256-wide
IBFs, runs of up to 200 parts, 4 levels) and a random one.  Windows of 20 to 40 values at step 5 over bins' own values;
thresholds max(1, len // 2 - 3 * shift) for shift 0, 2 and 4 (4: many false descents), and a run with thresholds 0 and above the
length.  Then the simulator's hard window sets, more items than the kernel has waves (a wave's second item starts on used
counters and mask words), column shards, and translated windows.  Every restatement is computed once and left unchanged."""
import numpy as np
import pytest

from count_windows_tree_ref import descend, walk, unit_of
from helpers import regular_hibf, layout_hibf, split_heavy_hibf, random_hibf
from search_ref import TreeRef
from test_gpu_count_windows import expanded, joined, sim_window_sets, tree_windows

pytestmark = pytest.mark.gpu

TREES = ["regular_mixed", "layout", "split_heavy", "random"]
THRESHOLDS = ["shift0", "shift2", "shift4", "edges"]
UNITS = [1, 2, 3, 16, 64]  # (64: clipped to 32 on a tree)
COUNT_GRID = 4096          # txq_count_plan.hpp kCountGrid: the waves of a level


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


_trees, _cases = {}, {}


def make_tree(oracle, name):
    """(descs, values per user bin, user bins, TreeRef), built once"""
    if name not in _trees:
        rng = np.random.default_rng(3)
        if name == "regular_mixed":
            ox, descs, values = regular_hibf(oracle, 1024, 16, 60, lambda b: rng.integers(0, 1 << 20, size=60, dtype=np.uint64), h=2, mixed=True)
            assert descs[0]["hash_funs"] != descs[1]["hash_funs"]
        elif name == "layout":
            ox, descs, values = layout_hibf(oracle, 5, user_bins=900, tmax=64, n_values=30)
            assert max(d["bins"] for d in descs) <= 64  # one-word rows
        elif name == "split_heavy":
            ox, descs, values = split_heavy_hibf(oracle, 7)[:3]
            assert max(d["bins"] for d in descs) == 256
        else:
            ox, descs, values = random_hibf(oracle, 11, user_bins=300, tmax=128)
        _trees[name] = (descs, values, len(values), TreeRef(oracle, len(values), descs))
    return _trees[name]


def thresholds(lens, kind):
    n = lens.astype(np.int64)
    if kind == "edges":  # some 0 (every bin), some above the length (none)
        t = n // 2
        j = np.arange(n.size)
        t[j % 7 == 3] = 0
        t[j % 5 == 1] = n[j % 5 == 1] + 1
        return t.astype(np.uint32)
    return np.maximum(1, n // 2 - 3 * int(kind[-1])).astype(np.uint32)


def restated(oracle, tree, kind, windows=None, key=None):
    """values, windows, thresholds and the restatement's hits, counts and levels: computed once per case and left unchanged"""
    key = key or (tree, kind)
    if key not in _cases:
        descs, values, user_bins, ref = make_tree(oracle, tree)
        if windows is None:
            v, begins, lens = tree_windows(values, len(tree), n_values=3000)
            assert v.size >= 3000 and lens.min() >= 20 and lens.max() <= 45 and begins.size >= 592
        else:
            begins, lens = windows
            rng = np.random.default_rng(len(tree))  # half of the values are bins' own: windows that descend
            n_values = int((begins + lens.astype(np.uint64)).max())
            own = np.concatenate([np.asarray(values[int(b)], dtype=np.uint64) for b in rng.integers(0, len(values), size=n_values // 10 + 1)])
            v = np.where(rng.random(n_values) < 0.5, np.resize(own, n_values), rng.integers(0, 1 << 20, size=n_values, dtype=np.uint64))
        thr = thresholds(lens, kind)
        ev, eo = expanded(v, begins, lens)
        want_hits, want_counts, levels = descend(ref, ev, eo, thr)
        for a in (v, begins, lens, thr, want_hits, want_counts):
            a.setflags(write=False)
        _cases[key] = (v, begins, lens, thr, want_hits, want_counts, levels)
    return _cases[key]


def set_knobs(monkeypatch, unit=None, tree=None):
    for knob, value in (("TXQ_COUNT_WINDOWS_UNIT", unit), ("TXQ_COUNT_WINDOWS_TREE", tree)):
        if value is None:
            monkeypatch.delenv(knob, raising=False)
        else:
            monkeypatch.setenv(knob, str(value))


@pytest.mark.parametrize("kind", THRESHOLDS)
@pytest.mark.parametrize("tree", TREES)
def test_parity_for_every_knob(capi, oracle, monkeypatch, tree, kind):
    descs, values, user_bins, ref = make_tree(oracle, tree)
    v, begins, lens, thr, want_hits, want_counts, levels = restated(oracle, tree, kind)
    # non-vacuity, from the restatement alone: an item below the root, a hit at a threshold above 1, a miss
    assert len(levels) > 1 and walk(levels, begins, lens, 16)["level_items"][1] > 0
    assert want_hits[thr > 1].any() and not want_hits[thr > lens].any() and (want_hits[(thr > 1) & (thr <= lens)] == 0).any()
    if kind == "shift4":  # steps that slide from a visited window to a later one across a window that did not visit the IBF
        for U in (3, 16, 32):
            assert walk(levels, begins, lens, U)["skipped"] >= 10, (tree, U)
    ix = capi.Index.upload_hibf(user_bins, descs)
    for unit, route in [(u, 1) for u in UNITS] + [(None, 1), (None, None), (None, 0), (3, 0)]:  # (None: the default of either knob)
        set_knobs(monkeypatch, unit, route)
        hits, counts = ix.count_windows(v, begins, lens, thr, counts=True)
        assert np.array_equal(counts, want_counts), (tree, kind, unit, route)
        assert np.array_equal(hits, want_hits), (tree, kind, unit, route)
        assert np.array_equal(ix.count_windows(v, begins, lens, thr), hits), (tree, kind, unit, route)  # counts=None: the same hits
    ix.free()


@pytest.mark.parametrize("tree", TREES)
def test_trace_equals_restated_walk(capi, oracle, monkeypatch, tree):
    descs, values, user_bins, ref = make_tree(oracle, tree)
    ix = capi.Index.upload_hibf(user_bins, descs)
    assert ix.count_windows_trace() == (0, 0, 0, 0)  # before the first call
    for kind in ("shift0", "shift4"):
        v, begins, lens, thr, want_hits, want_counts, levels = restated(oracle, tree, kind)
        total = int(lens.astype(np.int64).sum())
        for unit in UNITS + [None]:
            set_knobs(monkeypatch, unit, 1)
            w = walk(levels, begins, lens, unit_of(unit or 16))
            assert np.array_equal(ix.count_windows(v, begins, lens, thr), want_hits)
            trace = ix.count_windows_trace()
            assert trace == (w["visits"], w["added"], w["subtracted"], w["items"]), (tree, kind, unit)
            if kind == "shift0" and unit in (16, None):  # a condition that sliding happens (the CPU gives 0.37 to 0.40), no performance figure
                assert trace[1] + trace[2] < 0.5 * sum(int(lens[qs].astype(np.int64).sum()) for lv in levels for qs in lv.values())
                assert trace[0] >= begins.size and total > 0
        set_knobs(monkeypatch, 3, 0)  # the windows as independent queries: every visit an item, counted in full
        visits = sum(len(qs) for lv in levels for qs in lv.values())
        sum_len = sum(int(lens[qs].astype(np.int64).sum()) for lv in levels for qs in lv.values())
        assert np.array_equal(ix.count_windows(v, begins, lens, thr), want_hits)
        assert ix.count_windows_trace() == (visits, sum_len, 0, visits), (tree, kind)
    assert ix.count_windows(v, [], [], []).shape == (0, ix.shard_words) and ix.count_windows_trace() == (0, 0, 0, 0)  # a call of no windows
    ix.free()


def test_hard_window_sets(capi, oracle, monkeypatch):
    """empty, repeated, shrinking, touching and gapped windows: the simulator's sets as one sliding sequence, on the layout tree"""
    descs, values, user_bins, ref = make_tree(oracle, "layout")
    v, begins, lens, thr, want_hits, want_counts, levels = restated(oracle, "layout", "edges", windows=joined(sim_window_sets()), key="hard")
    assert (lens == 0).any() and (begins[1:] == begins[:-1]).any() and want_hits[thr > 1].any() and len(levels) > 1
    ix = capi.Index.upload_hibf(user_bins, descs)
    for unit, route in [(1, 1), (3, 1), (16, 1), (64, 1), (None, None), (None, 0)]:
        set_knobs(monkeypatch, unit, route)
        hits, counts = ix.count_windows(v, begins, lens, thr, counts=True)
        assert np.array_equal(counts, want_counts), (unit, route)
        assert np.array_equal(hits, want_hits), (unit, route)
        if route == 1:
            w = walk(levels, begins, lens, unit_of(unit))
            assert ix.count_windows_trace() == (w["visits"], w["added"], w["subtracted"], w["items"]), unit
    ix.free()


def test_more_items_than_waves(capi, oracle, monkeypatch):
    """8200 windows on the layout tree at U = 1 and U = 2: more than 4096 level-0 items on 4096 waves, and at U = 1 more than
    4096 items on a deeper level, so a wave's second item starts on the counters and mask words its first one used."""
    descs, values, user_bins, ref = make_tree(oracle, "layout")
    v, begins, lens = tree_windows(values, 17, n_values=41_100)
    key = "many"
    if key not in _cases:
        thr = thresholds(lens, "shift2")
        ev, eo = expanded(v, begins, lens)
        _cases[key] = (v, begins, lens, thr) + descend(ref, ev, eo, thr)
    v, begins, lens, thr, want_hits, want_counts, levels = _cases[key]
    assert begins.size >= 8200 and -(-begins.size // 2) > COUNT_GRID
    assert max(walk(levels, begins, lens, 1)["level_items"][1:]) > COUNT_GRID
    assert want_hits[thr > 1].any() and (want_hits == 0).any()
    ix = capi.Index.upload_hibf(user_bins, descs)
    for unit in (1, 2):
        set_knobs(monkeypatch, unit, 1)
        hits, counts = ix.count_windows(v, begins, lens, thr, counts=True)
        assert np.array_equal(counts, want_counts), unit
        assert np.array_equal(hits, want_hits), unit
        w = walk(levels, begins, lens, unit)
        assert ix.count_windows_trace() == (w["visits"], w["added"], w["subtracted"], w["items"]), unit
    ix.free()
    del _cases[key]


def test_column_shards_join(capi, oracle, monkeypatch):
    descs, values, user_bins, ref = make_tree(oracle, "layout")
    v, begins, lens, thr, want_hits, want_counts, levels = restated(oracle, "layout", "shift2")
    for unit in (3, None):
        set_knobs(monkeypatch, unit, 1)
        for R in (2, 3):
            hs, cs = [], []
            for r in range(R):
                sh = capi.Index.upload_hibf(user_bins, descs, shard_rank=r, n_shards=R)
                a, b = sh.count_windows(v, begins, lens, thr, counts=True)
                hs.append(a)
                cs.append(b)
                sh.free()
            assert np.array_equal(np.concatenate(hs, axis=1), want_hits), (unit, R)
            assert np.array_equal(np.concatenate(cs, axis=1), want_counts), (unit, R)
    sub = capi.Index.upload_hibf(user_bins, descs, shard_rank=0, n_shards=2, subtrees=True)  # sub-tree shards stay refused
    with pytest.raises(capi.TxqError) as e:
        sub.count_windows(v, begins, lens, thr)
    assert e.value.code == -1
    sub.free()


def test_translated_windows_on_a_tree(capi, oracle, monkeypatch):
    """capi.translate_windows output goes to count_windows on a tree: the sliding route and the independent one, identical arrays"""
    from tetrex_amd import host
    descs, values, user_bins, ref = make_tree(oracle, "layout")
    rng = np.random.default_rng(21)
    records = ["".join(rng.choice(list("ACGT"), size=int(n))) for n in (900, 0, 451, 2000, 77)]
    v, offsets, win_offsets, begins, lens = capi.translate_windows(records, 4, host.peptide_codes(0), 40, 10)
    assert begins.size > 500
    thr = np.maximum(1, lens // 4).astype(np.uint32)
    ix = capi.Index.upload_hibf(user_bins, descs)
    set_knobs(monkeypatch, None, 0)
    want_hits, want_counts = ix.count_windows(v, begins, lens, thr, counts=True)
    assert want_counts.max() > 0 and (want_hits == 0).any()
    set_knobs(monkeypatch, None, None)  # the default of both knobs
    hits, counts = ix.count_windows(v, begins, lens, thr, counts=True)
    assert np.array_equal(hits, want_hits) and np.array_equal(counts, want_counts)
    for unit in (None, 3):
        set_knobs(monkeypatch, unit, 1)
        hits, counts = ix.count_windows(v, begins, lens, thr, counts=True)
        assert np.array_equal(hits, want_hits) and np.array_equal(counts, want_counts), unit
        t = ix.count_windows_trace()
        assert t[3] < t[0] and t[2] > 0  # (fewer items than visits, values subtracted: it slid)
    ix.free()
