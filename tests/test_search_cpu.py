"""The threshold-membership restatement (tests/search_ref.py) on hand-made two- and three-level trees: what it must mean
before any kernel is compared with it."""
import numpy as np
import pytest

from helpers import MERGED, splitmix64
from search_ref import TreeRef, count_on, csr, unpack

# IBF -> technical bins: ("u", user bin) or ("m", child IBF).  User bin 0 is split in two in the root, 3 in three in IBF 1.
THREE_LEVELS = [
    [("u", 0), ("u", 0), ("m", 1), ("u", 1), ("m", 2)],
    [("u", 2), ("m", 3), ("u", 3), ("u", 3), ("u", 3)],
    [("u", 4), ("u", 5)],
    [("u", 6), ("u", 7)],
]
TWO_LEVELS = [
    [("m", 1), ("u", 0), ("u", 0), ("u", 0), ("m", 2)],
    [("u", 1), ("u", 2), ("u", 2)],
    [("u", 3), ("u", 4)],
]


def build(O, spec, per_bin=40, rows=2048, h=2, skip_merged=()):
    """The tree of `spec` in the oracle and as descriptors.  Each user bin's values go into its technical bins (a split bin's
    values are dealt over its parts) and into every merged bin above it, except the merged bins listed in skip_merged
    ((ibf, technical bin) pairs), which are left without them."""
    user_bins = 1 + max(x for ibf in spec for kind, x in ibf if kind == "u")
    values = [splitmix64(100 + u, per_bin) >> np.uint64(40) for u in range(user_bins)]
    parent = {}
    for i, ibf in enumerate(spec):
        for tb, (kind, x) in enumerate(ibf):
            if kind == "m":
                parent[x] = (i, tb)
    ox = O.Index.hibf(user_bins, dna=False, k=4)
    descs = []
    for i, ibf in enumerate(spec):
        nxt = np.array([x if k == "m" else 0 for k, x in ibf], dtype=np.uint64)
        tbu = np.array([MERGED if k == "m" else x for k, x in ibf], dtype=np.uint64)
        assert ox.add_ibf(len(ibf), rows, h, nxt, tbu) == i
        descs.append(dict(bins=len(ibf), bin_size=rows, hash_funs=h, next_ibf_id=nxt, tb_to_user=tbu))
    for i, ibf in enumerate(spec):
        for u in {x for k, x in ibf if k == "u"}:
            parts = [tb for tb, (k, x) in enumerate(ibf) if k == "u" and x == u]
            for tb, chunk in zip(parts, np.array_split(values[u], len(parts))):
                ox.hibf_emplace(i, chunk, tb)
            at = i
            while at in parent:
                p, ptb = parent[at]
                if (p, ptb) not in skip_merged:
                    ox.hibf_emplace(p, values[u], ptb)
                at = p
    for i, d in enumerate(descs):
        d["words"] = ox.hibf_words(i)
    return ox, descs, values


@pytest.mark.parametrize("spec", [TWO_LEVELS, THREE_LEVELS], ids=["two_levels", "three_levels"])
def test_split_run_is_summed(oracle, spec):
    ox, descs, values = build(oracle, spec)
    ref = TreeRef(oracle, len(values), descs)
    split = [(i, u) for i, ibf in enumerate(spec) for u in {x for k, x in ibf if k == "u"}
             if sum(1 for k, x in ibf if k == "u" and x == u) > 1]
    assert split
    for i, u in split:
        v, off = csr([values[u]])
        n = len(values[u])
        hits, counts = ref.search(v, off, [n])
        parts = [tb for tb, (k, x) in enumerate(spec[i]) if k == "u" and x == u]
        per_part = count_on(ref.ox[i], v, off)[0, parts]
        assert per_part.max() < n  # no part alone reaches the threshold ...
        assert counts[0, u] == per_part.sum() >= n  # ... their sum does
        assert unpack(hits)[0, u] == 1


def test_merged_bin_below_threshold_is_not_descended(oracle):
    # user bin 6 lives in IBF 3 under root -> IBF 1 -> IBF 3; the root's merged bin towards IBF 1 is left without its values
    ox, descs, values = build(oracle, THREE_LEVELS, skip_merged={(0, 2)})
    ref = TreeRef(oracle, len(values), descs)
    v, off = csr([values[6]])
    n = len(values[6])
    assert count_on(ref.ox[0], v, off)[0, 2] < n // 2
    assert count_on(ref.ox[3], v, off)[0, 0] >= n  # the leaf alone would report it
    hits, counts = ref.search(v, off, [n // 2])
    assert counts[0, 6] == 0 and unpack(hits)[0, 6] == 0
    assert counts[0, 2] == 0 and counts[0, 3] == 0  # nothing of IBF 1 either
    # the intact tree reports it
    ox, descs, values = build(oracle, THREE_LEVELS)
    hits, counts = TreeRef(oracle, len(values), descs).search(v, off, [n // 2])
    assert counts[0, 6] >= n and unpack(hits)[0, 6] == 1


@pytest.mark.parametrize("spec", [TWO_LEVELS, THREE_LEVELS], ids=["two_levels", "three_levels"])
def test_threshold_zero_selects_every_bin(oracle, spec):
    ox, descs, values = build(oracle, spec)
    ub = len(values)
    ref = TreeRef(oracle, ub, descs)
    v, off = csr([values[0], [], splitmix64(7, 30) >> np.uint64(40)])
    hits, _ = ref.search(v, off, [0, 0, 0])
    bits = unpack(hits)
    assert bits[:, :ub].all() and not bits[:, ub:].any()


@pytest.mark.parametrize("spec", [TWO_LEVELS, THREE_LEVELS], ids=["two_levels", "three_levels"])
def test_one_value_threshold_one_is_hibf_query(oracle, spec):
    ox, descs, values = build(oracle, spec)
    ref = TreeRef(oracle, len(values), descs)
    probe = np.concatenate([np.concatenate(values), splitmix64(9, 200) >> np.uint64(40)])
    v, off = csr([[x] for x in probe])
    hits, counts = ref.search(v, off, np.ones(probe.size, dtype=np.uint32))
    want = ox.probe(probe)
    assert np.array_equal(hits, want)
    assert np.array_equal(unpack(hits).astype(bool), counts >= 1)


def test_user_bin_in_several_runs(oracle):
    """A user bin whose parts are not adjacent (layout-shaped trees deal parts in any order) forms several runs: each run is
    walked on its own, as Hibf::descend does; the bin is a hit when any run passes, and its count is the largest run sum."""
    spec = [[("u", 0), ("u", 1), ("u", 0), ("m", 1)], [("u", 2), ("u", 3)]]
    ox, descs, values = build(oracle, spec)
    ref = TreeRef(oracle, len(values), descs)
    v, off = csr([values[0]])
    per_part = count_on(ref.ox[0], v, off)[0, [0, 2]]
    hits, counts = ref.search(v, off, [per_part.max()])
    assert counts[0, 0] == per_part.max() and unpack(hits)[0, 0] == 1
    hits, counts = ref.search(v, off, [per_part.max() + 1])  # the parts' sum would pass, but they are no run
    assert per_part.sum() >= per_part.max() + 1 and unpack(hits)[0, 0] == 0
    one = np.concatenate(values)
    kv, koff = csr([[x] for x in one])
    assert np.array_equal(ref.search(kv, koff, np.ones(one.size, dtype=np.uint32))[0], ox.probe(one))
