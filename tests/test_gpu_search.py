"""GPU parity of threshold membership (include/txq.h txq_count, `tetrex search`): every hit mask and every count against the
numpy restatement of tests/search_ref.py, on flat IBFs, column shards and regular, layout-shaped and split-heavy HIBFs; then
the command line on indexes that `tetrex index` builds from generated FASTA."""
import os
import subprocess

import numpy as np
import pytest

from helpers import random_words, oracle_ibf_from_words, regular_hibf, layout_hibf, split_heavy_hibf, splitmix64
from search_ref import TreeRef, flat_search, csr, unpack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TETREX = os.path.join(ROOT, "bin", "tetrex")


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


def thresholds_for(offsets, shift=0):
    """thresholds 0, 1, n/2, n and n + 1, in turn over the queries"""
    lens = np.diff(np.asarray(offsets, dtype=np.int64))
    pick = [lambda n: 0, lambda n: 1, lambda n: n // 2, lambda n: n, lambda n: n + 1]
    return np.array([pick[(q + shift) % 5](int(n)) for q, n in enumerate(lens)], dtype=np.uint32)


def mixed_batch(seed, lengths, value_bits=64):
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(lengths))
    qs = [splitmix64(seed * 1000 + i, lengths[i]) >> np.uint64(64 - value_bits) for i in order]
    return csr(qs)


def check_flat(capi, oracle, bins, h, lengths, seed, rows=1031, density=0.5, shards=(1,)):
    words = random_words(bins, rows, density, seed)
    ox = oracle_ibf_from_words(oracle, bins, rows, h, words)
    values, offsets = mixed_batch(seed, lengths)
    for shift in range(2):
        thr = thresholds_for(offsets, shift)
        want_hits, want_counts = flat_search(ox, bins, values, offsets, thr)
        for R in shards:
            got_h, got_c = [], []
            for r in range(R):
                ix = capi.Index.upload_ibf(bins, rows, h, words, shard_rank=r, n_shards=R)
                hits, counts = ix.count(values, offsets, thr, counts=True)
                w0, W = int(ix.info.shard_word0), ix.shard_words
                assert np.array_equal(hits, want_hits[:, w0:w0 + W]), (bins, h, R, r)
                assert np.array_equal(counts, want_counts[:, 64 * w0:64 * (w0 + W)]), (bins, h, R, r)
                assert np.array_equal(ix.count(values, offsets, thr), hits)  # without counts: the same hits
                got_h.append(hits)
                got_c.append(counts)
                ix.free()
            assert np.array_equal(np.concatenate(got_h, axis=1), want_hits)
            assert np.array_equal(np.concatenate(got_c, axis=1), want_counts)


BATCH = [0, 1, 63, 64, 65, 10000, 0, 7, 300, 1, 129, 2048, 64]


@pytest.mark.parametrize("bins,h", [(5, 1), (64, 2), (1000, 3), (1024, 4), (9000, 5), (1024, 3), (64, 5), (9000, 1)])
def test_flat_counts_match_restatement(capi, oracle, bins, h):
    check_flat(capi, oracle, bins, h, BATCH, seed=bins + h)


@pytest.mark.parametrize("lengths", [[0], [1], [63], [64], [65], [10000], [0, 0, 5, 0]], ids=str)
def test_flat_single_queries(capi, oracle, lengths):
    check_flat(capi, oracle, 1000, 3, lengths, seed=len(lengths) * 7 + sum(lengths))


def test_flat_column_shards_join(capi, oracle):
    check_flat(capi, oracle, 1000, 3, BATCH, seed=11, shards=(2, 3))
    check_flat(capi, oracle, 9000, 2, [65, 3000, 1, 0], seed=12, shards=(3,))


def test_flat_long_query_spreads_over_waves(capi, oracle):
    """10^6 values in one query (and a short one on either side) on a narrow IBF: the query is cut over many workgroups
    whose partial counts are added; every count must still be exact."""
    bins, rows, h = 40, 4099, 2
    words = random_words(bins, rows, 0.4, 5)
    ox = oracle_ibf_from_words(oracle, bins, rows, h, words)
    values, offsets = csr([splitmix64(1, 3), splitmix64(2, 1_000_000), splitmix64(3, 70)])
    for thr in ([1, 160_000, 2], [0, 1_000_001, 70]):
        want_hits, want_counts = flat_search(ox, bins, values, offsets, thr)
        ix = capi.Index.upload_ibf(bins, rows, h, words)
        hits, counts = ix.count(values, offsets, np.array(thr, dtype=np.uint32), counts=True)
        assert np.array_equal(counts, want_counts)
        assert np.array_equal(hits, want_hits)
        ix.free()
    assert want_counts[1].max() > 100_000  # (the sum of the partial counts of about 2000 workgroups)


def test_one_value_threshold_one_is_probe_flat(capi, oracle):
    for bins, h in ((64, 2), (1024, 3), (9000, 4)):
        words = random_words(bins, 2053, 0.45, bins)
        ix = capi.Index.upload_ibf(bins, 2053, h, words)
        kmers = splitmix64(bins, 5000)
        values, offsets = csr([[k] for k in kmers])
        assert np.array_equal(ix.count(values, offsets, np.ones(kmers.size, dtype=np.uint32)), ix.probe(kmers))
        ix.free()


def trees(oracle):
    rng = np.random.default_rng(3)
    yield "regular", regular_hibf(oracle, 1024, 16, 60, lambda b: rng.integers(0, 1 << 20, size=60, dtype=np.uint64), h=2)
    yield "regular_mixed", regular_hibf(oracle, 300, 5, 40, lambda b: rng.integers(0, 1 << 20, size=40, dtype=np.uint64), h=2, mixed=True)
    yield "layout", layout_hibf(oracle, 5, user_bins=900, tmax=64, n_values=30)
    yield "layout_4_levels", layout_hibf(oracle, 6, user_bins=400, tmax=16, n_values=30, direct=3)
    yield "split_heavy", split_heavy_hibf(oracle, 7)[:3]


def tree_batch(values, seed):
    """queries cut from user bins (all of a bin's values, or a part plus noise), a few random ones, an empty one"""
    rng = np.random.default_rng(seed)
    qs = []
    for _ in range(40):
        v = values[int(rng.integers(0, len(values)))]
        take = v if rng.random() < 0.5 else v[: max(1, len(v) // 2)]
        noise = rng.integers(0, 1 << 20, size=int(rng.integers(0, 6)), dtype=np.uint64)
        qs.append(np.concatenate([take, noise]))
    qs += [np.zeros(0, dtype=np.uint64), rng.integers(0, 1 << 20, size=70, dtype=np.uint64)]
    return csr(qs)


def test_hibf_counts_match_restatement(capi, oracle):
    for name, (ox, descs, values) in trees(oracle):
        user_bins = len(values)
        ref = TreeRef(oracle, user_bins, descs)
        ix = capi.Index.upload_hibf(user_bins, descs)
        v, off = tree_batch(values, len(name))
        for shift in range(5):
            thr = thresholds_for(off, shift)
            want_hits, want_counts = ref.search(v, off, thr)
            hits, counts = ix.count(v, off, thr, counts=True)
            assert np.array_equal(hits, want_hits), (name, shift)
            assert np.array_equal(counts, want_counts), (name, shift)
        # one value, threshold 1: the probe's masks
        k = np.concatenate([np.concatenate(values)[:3000], splitmix64(1, 500) >> np.uint64(44)])
        kv, koff = csr([[x] for x in k])
        assert np.array_equal(ix.count(kv, koff, np.ones(k.size, dtype=np.uint32)), ix.probe(k)), name
        assert np.array_equal(ix.probe(k), ox.probe(k)), name
        ix.free()


def test_hibf_column_shards_join(capi, oracle):
    rng = np.random.default_rng(4)
    for name, (ox, descs, values) in [("regular", regular_hibf(oracle, 1024, 16, 60, lambda b: rng.integers(0, 1 << 20, size=60, dtype=np.uint64), h=2)),
                                      ("layout", layout_hibf(oracle, 8, user_bins=700, tmax=64, n_values=30))]:
        ub = len(values)
        v, off = tree_batch(values, 9)
        thr = thresholds_for(off, 1)
        want_hits, want_counts = TreeRef(oracle, ub, descs).search(v, off, thr)
        for R in (2, 3):
            hs, cs = [], []
            for r in range(R):
                ix = capi.Index.upload_hibf(ub, descs, shard_rank=r, n_shards=R)
                hits, counts = ix.count(v, off, thr, counts=True)
                hs.append(hits)
                cs.append(counts)
                ix.free()
            assert np.array_equal(np.concatenate(hs, axis=1), want_hits), (name, R)
            assert np.array_equal(np.concatenate(cs, axis=1), want_counts), (name, R)


def test_refusals(capi, oracle):
    ox, descs, values = layout_hibf(oracle, 5, user_bins=900, tmax=64, n_values=30)
    sub = capi.Index.upload_hibf(900, descs, shard_rank=0, n_shards=2, subtrees=True)
    assert sub.info.join_or == 1
    v, off = csr([values[0], values[1]])
    with pytest.raises(capi.TxqError) as e:
        sub.count(v, off, [1, 1])
    assert e.value.code == -1
    sub.free()
    ix = capi.Index.upload_hibf(900, descs)
    # what the library refuses, called directly: offsets that are not ascending, more than 2^32-1 values, null pointers
    L = capi.lib()
    thr = np.ones(2, dtype=np.uint32)
    hits = np.zeros((2, ix.shard_words), dtype=np.uint64)
    u64p, u32p = capi.u64p, capi.u32p
    for bad in (np.array([0, 40, 30], dtype=np.uint64), np.array([0, 1, 1 << 32], dtype=np.uint64)):
        rc = L.txq_count(ix._h, v.ctypes.data_as(u64p), bad.ctypes.data_as(u64p), 2, thr.ctypes.data_as(u32p),
                         hits.ctypes.data_as(u64p), None)
        assert rc == -1, bad
    assert L.txq_count(ix._h, None, None, 1, None, None, None) == -1
    assert L.txq_count_device(ix._h, None, None, 1, None, None, None, None) == -1
    # offsets past the end of the values: the C signature carries no value count, so the Python wrapper checks this one
    with pytest.raises(capi.TxqError) as e:
        ix.count(v, np.array([0, 30, 61], dtype=np.uint64), [1, 1])
    assert e.value.code == -1
    hits = ix.count(v, off, [len(values[0]), 1])
    assert unpack(hits)[0, 0] == 1
    ix.free()


def test_hibf_wider_than_8192_bins_is_refused(capi):
    """On an HIBF one IBF's counters must fit the LDS of a workgroup: 8192 technical bins at most (include/txq.h)."""
    root_bins = 8200
    nxt = np.zeros(root_bins, dtype=np.uint64)
    nxt[0] = 1
    tbu = np.concatenate([[np.uint64(0xFFFFFFFFFFFFFFFF)], np.arange(root_bins - 1, dtype=np.uint64)])
    descs = [dict(bins=root_bins, bin_size=64, hash_funs=2, words=np.zeros(64 * 129, dtype=np.uint64), next_ibf_id=nxt, tb_to_user=tbu),
             dict(bins=2, bin_size=64, hash_funs=2, words=np.zeros(64, dtype=np.uint64), next_ibf_id=np.zeros(2, dtype=np.uint64),
                  tb_to_user=np.array([root_bins - 1, root_bins], dtype=np.uint64))]
    ix = capi.Index.upload_hibf(root_bins + 1, descs)
    v, off = csr([splitmix64(1, 10)])
    with pytest.raises(capi.TxqError) as e:
        ix.count(v, off, [1])
    assert e.value.code == -1
    ix.free()


def test_hibf_long_query(capi, oracle):
    """A query of 2 x 10^5 values on an HIBF (one wave per (query, IBF) pair counts it all): exact counts on every level."""
    ox, descs, values = layout_hibf(oracle, 5, user_bins=900, tmax=64, n_values=30)
    ref = TreeRef(oracle, 900, descs)
    long = np.concatenate([np.tile(values[7], 4000), splitmix64(5, 80_000) >> np.uint64(44)])
    v, off = csr([values[3], long, values[8]])
    for thr in ([1, 120_000, 30], [0, 1, 31]):
        want_hits, want_counts = ref.search(v, off, thr)
        hits, counts = ix_count(capi, descs, v, off, thr)
        assert np.array_equal(hits, want_hits), thr
        assert np.array_equal(counts, want_counts), thr
    assert unpack(want_hits)[1, 7] == 1 and want_counts[1, 7] >= 120_000


def ix_count(capi, descs, v, off, thr):
    ix = capi.Index.upload_hibf(900, descs)
    try:
        return ix.count(v, off, np.array(thr, dtype=np.uint32), counts=True)
    finally:
        ix.free()


# ---- the command line ---------------------------------------------------------------------------------------------------

AMINO = "ACDEFGHIKLMNPQRSTVWY"
ALPHABETS = {  # name: (residues, k, index flags, dna, reduction, query length)
    "peptide": (AMINO, 6, [], False, 0, 60),
    "murphy": (AMINO, 5, ["-r", "murphy"], False, 1, 60),
    "dna": ("ACGT", 16, ["-n"], True, 0, 150),
}
LAYOUTS = {"flat": ["-i"], "default": [], "sized": ["--layout", "sized"]}
EDITS = 2


def _run(*args):
    r = subprocess.run([TETREX, *args], capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


def _edit(seq, e, residues, rng):
    s = list(seq)
    for _ in range(e):
        kind = int(rng.integers(0, 3))
        at = int(rng.integers(1, len(s) - 1))
        if kind == 0:
            s[at] = residues[(residues.index(s[at]) + 1 + int(rng.integers(0, len(residues) - 1))) % len(residues)]
        elif kind == 1:
            s.insert(at, residues[int(rng.integers(0, len(residues)))])
        else:
            del s[at]
    return "".join(s)


@pytest.fixture(scope="module")
def cli_setup(tmp_path_factory):
    """For each alphabet: 70 bins of generated FASTA (gzip for some), its three indexes, and a query file of records cut
    from the bins with up to EDITS substitutions and indels (plus a record too short for one k-mer)."""
    import gzip
    root = tmp_path_factory.mktemp("search_cli")
    out = {}
    for name, (res, k, flags, dna, red, qlen) in ALPHABETS.items():
        rng = np.random.default_rng(len(name))
        d = root / name
        d.mkdir()
        files, seqs = [], []
        for b in range(70):
            recs = ["".join(rng.choice(list(res), size=int(rng.integers(150, 400) * (3 if dna else 1)))) for _ in range(2)]
            seqs.append(recs)
            text = "".join(">b%d_%d\n%s\n" % (b, i, r) for i, r in enumerate(recs))
            p = d / ("bin%02d.fa" % b + (".gz" if b % 3 == 0 else ""))
            if b % 3 == 0:
                with gzip.open(p, "wt") as f:
                    f.write(text)
            else:
                p.write_text(text)
            files.append(str(p))
        queries = []
        for q in range(40):
            b = int(rng.integers(0, 70))
            rec = seqs[b][int(rng.integers(0, 2))]
            at = int(rng.integers(0, len(rec) - qlen))
            queries.append(("q%d_b%d" % (q, b), b, _edit(rec[at:at + qlen], int(rng.integers(0, EDITS + 1)), res, rng)))
        queries.append(("tiny", -1, res[: k - 1]))
        qf = d / "queries.fa"
        qf.write_text("".join(">%s some comment\n%s\n" % (n, s) for n, _, s in queries))
        indexes = {}
        for lay, lflags in LAYOUTS.items():
            rc, so, se = _run("index", "-k", str(k), *flags, *lflags, str(d / lay), *files)
            assert rc == 0 and os.path.exists(d / (lay + ".ibf")), se
            indexes[lay] = str(d / (lay + ".ibf"))
        out[name] = dict(files=[os.path.abspath(f) for f in files], queries=queries, qfile=str(qf), indexes=indexes, k=k, dna=dna, red=red)
    return out


def _expected(oracle, setup, layout, thresholds_of):
    """rows (name, bin path, count, n) the restatement gives for the query file on one index"""
    from tetrex_amd import host
    ix = host.IndexFile.load(setup["indexes"][layout])
    d = ix.describe()
    qs = [(n, host.record_values_array(s, setup["k"], dna=setup["dna"], reduction=setup["red"])) for n, _, s in setup["queries"]]
    qs = [(n, v) for n, v in qs if v.size]
    values, offsets = csr([v for _, v in qs])
    thr = np.array([thresholds_of(v.size) for _, v in qs], dtype=np.uint32)
    if d["is_hibf"]:
        descs = []
        for i, f in enumerate(d["ibfs"]):
            nxt, tbu = ix.maps(i)
            descs.append(dict(bins=f["bins"], bin_size=f["bin_size"], hash_funs=f["hash_funs"], words=ix.words(i), next_ibf_id=nxt, tb_to_user=tbu))
        hits, counts = TreeRef(oracle, d["bins"], descs).search(values, offsets, thr)
    else:
        f = d["ibfs"][0]
        hits, counts = flat_search(oracle_ibf_from_words(oracle, f["bins"], f["bin_size"], f["hash_funs"], ix.words(0)), f["bins"], values, offsets, thr)
    bits = unpack(hits)
    rows = []
    for q, (n, v) in enumerate(qs):
        for u in np.flatnonzero(bits[q]):
            rows.append((n, d["paths"][u], int(counts[q, u]), int(v.size)))
    return rows


@pytest.mark.parametrize("alphabet", list(ALPHABETS))
def test_cli_search(oracle, cli_setup, tmp_path, alphabet):
    import math
    setup = cli_setup[alphabet]
    k = setup["k"]
    for layout, path in setup["indexes"].items():
        rc, so, se = _run("search", "-e", str(EDITS), "--counts", "-v", path, setup["qfile"])
        assert rc == 0, se
        assert "tiny: no k-mer" in se and "Search time:" in se
        got = [tuple(line.split("\t")) for line in so.splitlines()]
        want = _expected(oracle, setup, layout, lambda n: max(n - k * EDITS, 0))
        assert got == [(n, p, "%d/%d" % (c, m)) for n, p, c, m in want], (alphabet, layout)
        # the q-gram lemma: every query is reported in the bin it was cut from
        reported = {(n, p) for n, p, _ in got}
        for n, b, _ in setup["queries"]:
            if b >= 0:
                assert (n, setup["files"][b]) in reported, (alphabet, layout, n)
        # --threshold, -o
        dest = tmp_path / ("%s_%s.tsv" % (alphabet, layout))
        rc, so, se = _run("search", "--threshold", "0.6", "-o", str(dest), path, setup["qfile"])
        assert rc == 0 and so == "", se
        got = [tuple(line.split("\t")) for line in dest.read_text().splitlines()]
        want = _expected(oracle, setup, layout, lambda n: math.ceil(0.6 * n))
        assert got == [(n, p) for n, p, _, _ in want], (alphabet, layout)
    # a large -e gives threshold 0: every bin, with a note
    rc, so, se = _run("search", "-e", "1000", setup["indexes"]["default"], setup["qfile"])
    assert rc == 0 and "threshold 0, every bin is reported" in se
    assert len(so.splitlines()) == 70 * (len(setup["queries"]) - 1)


@pytest.mark.parametrize("flags", [["-e", "1", "--threshold", "0.5"], ["--threshold", "0"], ["--threshold", "1.5"], ["--threshold", "x"],
                                   ["-e", "-1"], ["-e", "two"], ["--bogus"]], ids=str)
def test_cli_search_refuses_bad_options(tmp_path, flags):
    q = tmp_path / "q.fa"
    q.write_text(">a\nACDEFGHIK\n")
    rc, so, se = _run("search", *flags, str(tmp_path / "missing.ibf"), str(q))
    assert "[Search Parser Error]" in se and "Index not valid" not in se and so == "", se
    assert rc != 0
