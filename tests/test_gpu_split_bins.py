"""Split user bins with MANY parts in layout order (csrc/txq_records.hpp VSplit): a fused step (csrc/txq_exec.hip PathRows) sees a
split bin only through its representative's chunk and learns of the other parts from the IBF's side matrix, whose entries for
one chunk are as many consecutive bits as the chunk has parts — 199 for a user bin split 200 ways, as seqan::hibf's layouts
with tmax = 256 produce.  Every mask must equal the CPU oracle's, on every way a session can take; the planted k-mers of each
heavy bin lie only in parts at late side bits (tests/helpers.py split_heavy_hibf), so a step that reads too few side words
drops the bin.  The sub-tree shards' roots (txq_index_upload_subtrees) clear the columns of other shards' technical bins: those
must not become parts of user bin 0."""
import numpy as np
import pytest

from helpers import MERGED, kmer_values, split_heavy_hibf

pytestmark = pytest.mark.gpu

DENSE = {"TETREX_DENSE_MIN": "2", "TETREX_DENSE_SPARSE_BELOW": "2", "TETREX_DENSE_EVIDENCE": "dense"}
WAYS = {  # (every way but the last with TXQ_KMER_TABLE_MB=0: the index's table of all k-mers' masks would take the steps over)
    "default": {},
    "dense": DENSE,
    "tracked": dict(DENSE, TETREX_DENSE_TRACKED="1"),
    "untracked": dict(DENSE, TETREX_DENSE_TRACKED="0"),
    "enumerated": {"TETREX_DENSE": "0"},
    "level-kernels": {"TXQ_HIBF_LAYOUT_FUSED": "0"},
    "user-order": {"TXQ_HIBF_LAYOUT_ORDER": "0"},
    "kmer-table": {"TXQ_KMER_TABLE_MB": "512", "TXQ_KMER_TABLE_MIN": "1"},  # (last: once built, the table stays with the index)
}
KNOBS = sorted({n for env in WAYS.values() for n in env} | {"TXQ_KMER_TABLE_MB"})


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


def _set_way(monkeypatch, way):
    for n in KNOBS:
        monkeypatch.delenv(n, raising=False)
    monkeypatch.setenv("TXQ_KMER_TABLE_MB", "0")
    for n, v in WAYS[way].items():
        monkeypatch.setenv(n, v)


def _variants(motifs):
    """(query, literal): the literals, and `.`, class and {m,n} forms of them (each still matches its literal)."""
    out = []
    for m in motifs:
        out += [(m, m), (m[0] + "." + m[2:], m), (m[:2] + "[" + "".join(sorted(set(m[2] + "AK"))) + "]" + m[3:], m), (m[:3] + ".{0,2}" + m[3:], m)]
    return out


def _has(mask, ub):
    return (int(mask[ub >> 6]) >> (ub & 63)) & 1


@pytest.mark.parametrize("k", [4, 6])
@pytest.mark.parametrize("narrow", [False, True], ids=["16-byte-chunks", "8-byte-chunks"])
def test_heavy_split_bins_on_every_way(capi, oracle, monkeypatch, narrow, k):
    ox, descs, values, planted = split_heavy_hibf(oracle, 3, k=k, narrow=narrow)
    ub = ox.bins
    qs, lits = zip(*_variants(sorted(planted)))
    wants = []
    for q in qs:
        want, quirks = ox.expected_mask(q)
        assert quirks == 0, q  # (no motif is exempted)
        wants.append(want)
    ix = capi.Index.upload_hibf(ub, descs)
    assert ix.supports_dense() == 2  # the tree is taken in layout order
    qs = list(qs)
    results = {}
    for way in WAYS:
        _set_way(monkeypatch, way)
        got, status, stats = ix.query_masks(qs, False, k)
        results[way] = got
        hits = 0
        for q, g, st, want in zip(qs, got, status, wants):
            assert st == 0, (way, q)
            assert np.array_equal(g, want), (way, q, np.nonzero(np.unpackbits((g ^ want).view(np.uint8), bitorder="little"))[0][:8])
        for lit, g in zip(lits, got):
            hits += sum(_has(g, u) for u in planted[lit])
        assert hits == 4 * len(planted), way  # every planted bin answers its literal and each variant of it (cannot pass vacuously)
        if way in ("dense", "tracked", "untracked"):
            assert stats["dense_ops"] > 0, way
        if way == "tracked":
            assert stats["tracked_queries"] > 0
        if way == "untracked":
            assert stats["tracked_queries"] == 0
    for way, got in results.items():
        assert np.array_equal(got, results["user-order"]), way
    kmers = np.array([v for m in planted for v in kmer_values(m, k)] + [int(v) for v in values[0][:4]], dtype=np.uint64)
    assert np.array_equal(ix.probe(kmers), ox.probe(kmers))
    ix.free()


def _subtree_root_hibf(O, seed, children=380, leaf_bins=8, n_values=6, k=4):
    """A root of `children` merged bins (one-word leaves of single user bins) and, above all of them, user bin 0 and a few more
    user bins of its own: a sub-tree shard keeps its own merged bins and clears the others (txq_index_upload_subtrees), so the
    root of shard 0 has >= 128 cleared technical bins below user bin 0's.  Motif `motif` is planted in user bin 0 and in leaf
    bins spread over the shards.  Returns (oracle index, descs, motif, user bins holding it)."""
    rng = np.random.default_rng(seed)
    motif = "WMKHCQ"
    planted_kmers = kmer_values(motif, k)
    own = 4  # the root's own user bins: 0 and three more, in its last technical bins
    user_bins = own + children * leaf_bins
    holders = [0] + [own + c * leaf_bins + (c % leaf_bins) for c in (3, 100, 201, 302, 377)]

    def content(u):
        v = rng.integers(0, 1 << (5 * k), size=n_values, dtype=np.uint64)
        return np.concatenate([v, np.array(planted_kmers, dtype=np.uint64)]) if u in holders else v
    leaf = [[content(own + c * leaf_bins + b) for b in range(leaf_bins)] for c in range(children)]
    root_tbs = [np.concatenate(leaf[c]) for c in range(children)] + [content(u) for u in range(own)]
    ox = O.Index.hibf(user_bins, dna=False, k=k)
    descs = [dict(bins=children + own, bin_size=2048, hash_funs=2, words=None,
                  next_ibf_id=np.array(list(range(1, children + 1)) + [0] * own, dtype=np.uint64),
                  tb_to_user=np.array([MERGED] * children + list(range(own)), dtype=np.uint64))]
    descs += [dict(bins=leaf_bins, bin_size=256, hash_funs=2, words=None, next_ibf_id=np.zeros(leaf_bins, dtype=np.uint64),
                   tb_to_user=np.arange(own + c * leaf_bins, own + (c + 1) * leaf_bins, dtype=np.uint64)) for c in range(children)]
    for i, d in enumerate(descs):
        j = ox.add_ibf(d["bins"], d["bin_size"], d["hash_funs"], d["next_ibf_id"], d["tb_to_user"])
        for tb in range(d["bins"]):
            ox.hibf_emplace(j, root_tbs[tb] if i == 0 else leaf[i - 1][tb], tb)
    for i, d in enumerate(descs):
        d["words"] = ox.hibf_words(i)
    return ox, descs, motif, holders


@pytest.mark.parametrize("R", [2, 3])
def test_sub_tree_shards_do_not_merge_cleared_root_bins_into_user_bin_0(capi, oracle, monkeypatch, R):
    ox, descs, motif, holders = _subtree_root_hibf(oracle, 11)
    ub = ox.bins
    assert descs[0]["bins"] >= 192 and int(descs[0]["tb_to_user"][-4]) == 0
    qs = [q for q, _ in _variants([motif])] + ["LMA(E|Q)GLYN", "A.CD", "K[RK]DE"]
    wants = []
    for q in qs:
        want, quirks = ox.expected_mask(q)
        assert quirks == 0, q
        wants.append(want)
    assert all(_has(wants[0], u) for u in holders)
    one = capi.Index.upload_hibf(ub, descs)
    shards = [capi.Index.upload_hibf(ub, descs, shard_rank=r, n_shards=R, subtrees=True) for r in range(R)]
    for s_ in shards:
        assert s_.info.join_or == 1 and s_.supports_dense() == 2
    for way in ("default", "user-order", "dense", "tracked"):
        _set_way(monkeypatch, way)
        ref, _, _ = one.query_masks(qs, False, 4)
        full, status, _ = capi.query_masks_sharded(shards, qs, False, 4)
        for q, g, r_, st, want in zip(qs, full, ref, status, wants):
            assert st == 0, (way, q)
            assert np.array_equal(g, want), (way, q, np.nonzero(np.unpackbits((g ^ want).view(np.uint8), bitorder="little"))[0][:8])
            assert np.array_equal(r_, want), (way, "unsharded", q)
        assert sum(_has(g, u) for g in full[:4] for u in holders) >= 4 * len(holders), way
    # plain probes: the OR of the shards is membership_for of the whole tree; only shard 0 holds user bin 0's part (the root's own
    # user bins go to shard 0), and no other shard reports user bin 0 through a cleared technical bin
    kmers = np.array(kmer_values(motif, 4) + [int(x) for x in np.random.default_rng(5).integers(0, 1 << 20, size=400)], dtype=np.uint64)
    want = ox.probe(kmers)
    got = np.zeros_like(want)
    for r, s_ in enumerate(shards):
        p = s_.probe(kmers)
        got |= p
        if r:
            assert not (p[:, 0] & np.uint64(1)).any(), r
    assert np.array_equal(got, want)
    assert (want[:, 0] & np.uint64(1)).any()
    for s_ in shards + [one]:
        s_.free()
