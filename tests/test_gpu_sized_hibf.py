"""Size-aware HIBFs built on the GPU (`tetrex index --layout sized`; csrc/txq_build.hip, host/layout.hpp): the sketch and union
kernels against their numpy restatement bit for bit, the built trees against an independent rebuild in the CPU oracle, no false
negatives, the false-positive rate the sizing promises, query parity with the oracle on trees with split bins, merged bins and
three levels (every way test_gpu_layout_order.py runs a tree), and the CLI end to end."""
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from motifs import random_prosite_motifs
from sized_hibf_ref import MERGED, part_of, paths, registers, union_table

pytestmark = pytest.mark.gpu
TETREX = os.path.join(ROOT, "bin", "tetrex")
AA = "ACDEFGHIKLMNPQRSTVWY"


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


def _seq(rng, n, alphabet=AA):
    return "".join(rng.choice(list(alphabet), size=n))


def _library(d, name, seed, n_bins, giant_records, dna=False, empty_every=0):
    """One giant bin (bin 1), eight medium bins, tiny bins; every `empty_every`-th bin holds only a record shorter than k."""
    rng = np.random.default_rng(seed)
    alphabet = "ACGT" if dna else AA
    files, recs = [], []
    for b in range(n_bins):
        if b == 1:
            seqs = [_seq(rng, 200, alphabet) for _ in range(giant_records)]
        elif b % max(1, n_bins // 8) == 3:
            seqs = [_seq(rng, 120, alphabet) for _ in range(8)]
        elif empty_every and b % empty_every == 7:
            seqs = [_seq(rng, 3, alphabet)]
        else:
            seqs = [_seq(rng, int(rng.integers(30, 70)), alphabet)]
        p = d / ("%s%04d.fa" % (name, b))
        p.write_text("".join(">r%d_%d\n%s\n" % (b, i, s) for i, s in enumerate(seqs)))
        files.append(str(p))
        recs.append(seqs)
    return files, recs


def _values(recs, k, dna=False, reduction=0):
    from tetrex_amd import host
    out = []
    for seqs in recs:
        vs = [host.record_values_array(s, k, dna, reduction, True) for s in seqs if len(s) >= k]
        out.append(np.concatenate(vs).astype(np.uint64) if vs else np.zeros(0, dtype=np.uint64))
    return out


def _tree(ix):
    d = ix.describe()
    ibfs = []
    for i, f in enumerate(d["ibfs"]):
        nxt, tbu = ix.maps(i)
        ibfs.append(dict(bins=f["bins"], bin_size=f["bin_size"], hash_funs=f["hash_funs"], words=ix.words(i),
                         next_ibf_id=nxt, tb_to_user=tbu, tb_to_user_bin=tbu))
    return d, ibfs


def _rebuild(oracle, ibfs, values, dna, k, reduction=0):
    """The tree's bits from its maps alone: every value of user bin b in each merged bin on b's path and in the part of
    its leaf run that the part rule picks (oracle hibf_emplace)."""
    ox = oracle.Index.hibf(len(values), dna=dna, k=k, reduction=reduction)
    for f in ibfs:
        ox.add_ibf(f["bins"], f["bin_size"], f["hash_funs"], f["next_ibf_id"], f["tb_to_user"])
    for ub, steps in paths(ibfs).items():
        v = values[ub]
        if not v.size:
            continue
        for (i, t, parts) in steps[:-1]:
            ox.hibf_emplace(i, v, t)
        i, t, parts = steps[-1]
        which = part_of(v, parts)
        for p in np.unique(which):
            ox.hibf_emplace(i, v[which == p], t + int(p))
    return ox


def _shape(ibfs):
    p = paths(ibfs)
    split = sum(1 for s in p.values() if s[-1][2] > 1)
    merged = sum(1 for f in ibfs for u in f["tb_to_user"] if int(u) == MERGED)
    return split, merged, max(len(s) for s in p.values())


# ---- kernels against numpy --------------------------------------------------------------------------------------------


def test_sketch_registers_and_union_table_equal_the_numpy_restatement(capi):
    from tetrex_amd import host
    rng = np.random.default_rng(11)
    bins = [np.zeros(0, dtype=np.uint64), np.array([12345], dtype=np.uint64),
            rng.integers(0, 1 << 30, size=1_200_000, dtype=np.uint64)]
    bins += [rng.integers(0, 1 << int(rng.integers(8, 30)), size=int(rng.integers(1, 60_000)), dtype=np.uint64) for _ in range(21)]
    bins.append(np.repeat(np.arange(500, dtype=np.uint64), 7))  # repeated values
    regs = capi.sketch(bins)
    for b, v in enumerate(bins):
        assert np.array_equal(regs[b], registers(v)), b
    counts = capi.union_estimates(regs, np.arange(len(bins), dtype=np.uint32), 1)[:, 0]
    order = host.layout_order(counts)
    W = len(bins)  # the full window
    got = capi.union_estimates(regs, order.astype(np.uint32), W)
    want = union_table(regs, order, W)
    assert np.array_equal(got, want)
    assert counts[0] == 0.0 and abs(counts[1] - 1.0) < 0.01 and abs(counts[2] - 1_200_000) < 0.05 * 1_200_000


# ---- built trees ------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def pep(tmp_path_factory):
    """1100 peptide bins, one giant, t_max 64: W = 72 > 64, so merged runs longer than an IBF's 64 technical bins give a
    third level."""
    d = tmp_path_factory.mktemp("pep")
    files, recs = _library(d, "p", 5, 1100, 300, empty_every=97)
    return files, recs


def _build(files, k, dna=False, reduction=0, tmax=None):
    from tetrex_amd import host
    return host.IndexFile.build(files, k=k, dna=dna, reduction=reduction, layout="sized", tmax=tmax)


@pytest.mark.parametrize("k", [6, 4])
def test_peptide_tree_rebuilds_and_answers_every_kmer(capi, oracle, pep, k):
    files, recs = pep
    ix = _build(files, k, tmax=64)
    d, ibfs = _tree(ix)
    split, merged, depth = _shape(ibfs)
    assert d["is_hibf"] and split >= 1 and merged >= 10 and depth >= (3 if k == 6 else 2), (split, merged, depth)
    values = _values(recs, k)
    ox = _rebuild(oracle, ibfs, values, False, k)
    for i in range(len(ibfs)):
        assert np.array_equal(ox.hibf_words(i), ibfs[i]["words"]), i
    # no false negatives: every k-mer of bin b reports b, on the device and in the oracle
    dx = capi.Index.upload_hibf(len(files), ibfs)
    for b in range(0, len(files), 7) if k == 4 else range(len(files)):
        if not values[b].size:
            continue
        for masks in (dx.probe(values[b]), ox.probe(values[b])):
            assert np.all((masks[:, b // 64] >> np.uint64(b % 64)) & np.uint64(1)), b
    # false positives: 2^16 k-mers that lie in no bin
    if k == 6:
        present = np.unique(np.concatenate(values))
        rng = np.random.default_rng(99)
        from tetrex_amd import host
        cand = np.unique(host.record_values_array(_seq(rng, 90_000), k, False, 0, True).astype(np.uint64))
        absent = cand[~np.isin(cand, present)][: 1 << 16]
        assert absent.size == 1 << 16
        masks = dx.probe(absent)
        bits = np.unpackbits(masks.view(np.uint8), axis=1, bitorder="little")[:, : len(files)]
        rate = bits.mean(axis=0)
        print("sized tree FPR: mean %.4f max %.4f (bin %d)" % (rate.mean(), rate.max(), int(rate.argmax())))
        assert rate.mean() <= 1.25 * 0.05 and rate.max() <= 2 * 0.05, (rate.mean(), rate.max())
    dx.free()


def _planted(recs, rng, n):
    """PROSITE-style motifs cut from the library's own records: residues, wildcards and classes."""
    out = []
    while len(out) < n:
        seqs = recs[int(rng.integers(0, len(recs)))]
        s = seqs[int(rng.integers(0, len(seqs)))]
        if len(s) < 12:
            continue
        a = int(rng.integers(0, len(s) - 11))
        parts = []
        for c in s[a:a + int(rng.integers(8, 12))]:
            r = rng.random()
            parts.append("." if r < 0.08 else "[%s]" % "".join(sorted(set(c + AA[int(rng.integers(0, 20))]))) if r < 0.25 else c)
        out.append("".join(parts))
    return out


WAYS = ("layout", "layout-levels", "layout-blocks", "layout-tracked", "user-order", "table", "two-shards")


@pytest.mark.parametrize("k", [6, 4])
def test_peptide_queries_on_sized_trees_equal_the_oracle(capi, oracle, pep, monkeypatch, tmp_path, k):
    files, recs = pep
    rc = subprocess.run([TETREX, "index", "--layout", "sized", "--tmax", "64", "-k", str(k), str(tmp_path / "ix"), *files],
                        capture_output=True, text=True, timeout=600)
    assert rc.returncode == 0 and os.path.exists(tmp_path / "ix.ibf"), rc.stderr
    from tetrex_amd import host
    ix = host.IndexFile.load(str(tmp_path / "ix.ibf"))
    d, ibfs = _tree(ix)
    split, merged, depth = _shape(ibfs)
    assert split >= 1 and merged >= 10 and depth >= (3 if k == 6 else 2), (split, merged, depth)
    ox = _rebuild(oracle, ibfs, _values(recs, k), False, k)
    rng = np.random.default_rng(k)
    qs = random_prosite_motifs(150, 40 + k) + _planted(recs, rng, 50)
    assert len(qs) == 200
    wants = [ox.query(q, with_stats=True) for q in qs]
    monkeypatch.setenv("TETREX_DENSE_EVIDENCE", "dense")
    ub = len(files)
    results = {}
    for way in WAYS:
        for var in ("TETREX_DENSE_MIN", "TETREX_DENSE_SPARSE_BELOW", "TETREX_DENSE_TRACKED", "TXQ_HIBF_LAYOUT_ORDER",
                    "TXQ_HIBF_LAYOUT_FUSED"):
            monkeypatch.delenv(var, raising=False)
        monkeypatch.setenv("TXQ_KMER_TABLE_MB", "512" if way == "table" else "0")
        monkeypatch.setenv("TXQ_KMER_TABLE_MIN", "1")
        if way == "layout-levels":
            monkeypatch.setenv("TXQ_HIBF_LAYOUT_FUSED", "0")
        if way in ("layout-blocks", "layout-tracked", "table"):
            monkeypatch.setenv("TETREX_DENSE_MIN", "2")
            monkeypatch.setenv("TETREX_DENSE_SPARSE_BELOW", "2")
        if way == "layout-tracked":
            monkeypatch.setenv("TETREX_DENSE_TRACKED", "1")
        if way == "user-order":
            monkeypatch.setenv("TXQ_HIBF_LAYOUT_ORDER", "0")
        if way == "two-shards":
            shards = [capi.Index.upload_hibf(ub, ibfs, shard_rank=r, n_shards=2, subtrees=True) for r in range(2)]
            got, status, _ = capi.query_masks_sharded(shards, qs, False, k)
            for s in shards:
                s.free()
        else:
            dx = capi.Index.upload_hibf(ub, ibfs)
            got, status, _ = dx.query_masks(qs, False, k)
            dx.free()
        hits = compared = 0
        for q, g, st, (want, ost) in zip(qs, got, status, wants):
            assert st == 0, q
            if not ost["quirk_merges"]:
                compared += 1
                assert np.array_equal(g, want), (q, way)
                hits += int(want.any())
        assert compared >= 150 and hits >= 40, (way, compared, hits)
        results[way] = got
    for way, got in results.items():
        assert np.array_equal(got, results["user-order"]), way


@pytest.mark.parametrize("case", ["dna-k16", "murphy-k6"])
def test_dna_and_reduced_alphabet_trees(capi, oracle, tmp_path, case):
    dna = case.startswith("dna")
    k, reduction = (16, 0) if dna else (6, 1)
    files, recs = _library(tmp_path, "l", 8, 150, 200, dna=dna)
    ix = _build(files, k, dna=dna, reduction=reduction)
    d, ibfs = _tree(ix)
    split, merged, _ = _shape(ibfs)
    assert split >= 1 and merged >= 1, (split, merged)
    values = _values(recs, k, dna, reduction)
    ox = _rebuild(oracle, ibfs, values, dna, k, reduction)
    for i in range(len(ibfs)):
        assert np.array_equal(ox.hibf_words(i), ibfs[i]["words"]), i
    dx = capi.Index.upload_hibf(len(files), ibfs)
    rng = np.random.default_rng(3)
    if dna:
        qs = [recs[b][0][a:a + 22] for b in range(0, 150, 9) for a in (5,)] + ["ACGT.{0,4}" + recs[1][3][10:28], "GATTACA.{2}TTAGC"]
    else:
        qs = _planted(recs, rng, 30)
    got, status, _ = dx.query_masks(qs, dna, k, reduction)
    hits = 0
    for q, g, st in zip(qs, got, status):
        want, ost = ox.query(q, with_stats=True)
        assert st == 0, q
        if not ost["quirk_merges"]:
            assert np.array_equal(g, want), q
            hits += int(want.any())
    assert hits >= 10
    dx.free()


# ---- CLI --------------------------------------------------------------------------------------------------------------


def _run(*args, cwd=None):
    r = subprocess.run([TETREX, *args], capture_output=True, text=True, cwd=cwd, timeout=600)
    return r.returncode, r.stdout, r.stderr


def test_cli_sized_index_verifies_like_a_flat_index(tmp_path):
    files, recs = _library(tmp_path, "c", 21, 300, 120)
    for name, flags in (("flat", ["-i"]), ("sized", ["--layout", "sized"]), ("again", ["--layout", "sized"])):
        rc, so, se = _run("index", "-k", "5", *flags, str(tmp_path / name), *files)
        assert rc == 0 and "across 300 bins." in se, se
    assert open(tmp_path / "sized.ibf", "rb").read() == open(tmp_path / "again.ibf", "rb").read()
    rc, so, se = _run("inspect", str(tmp_path / "sized.ibf"))
    assert rc == 0 and "INDEX TYPE: HIBF" in so and so.count("\t- ") == 300
    motifs = _planted(recs, np.random.default_rng(5), 12)
    for q in motifs[:4]:
        out = {}
        for name in ("flat", "sized"):
            rc, so, se = _run("query", "-v", str(tmp_path / (name + ".ibf")), q)
            assert rc == 0, se
            out[name] = sorted(so.splitlines())
        assert out["flat"] == out["sized"] and out["flat"], q
    (tmp_path / "motifs.tsv").write_text("".join("M%d\t%s\n" % (i, m) for i, m in enumerate(motifs)))
    res = {}
    for name in ("flat", "sized"):
        od = tmp_path / ("out_" + name)
        od.mkdir()
        rc, so, se = _run("query", "-f", str(tmp_path / (name + ".ibf")), str(tmp_path / "motifs.tsv"), cwd=str(od))
        assert rc == 0, se
        res[name] = {os.path.basename(p): open(p).read() for p in sorted(glob.glob(str(od / "*.tsv")))}
    assert res["flat"] == res["sized"] and sum(1 for v in res["flat"].values() if v) >= 8


@pytest.mark.parametrize("flags", [["--layout", "sized", "-i"], ["--layout", "uniform", "-i"], ["--layout", "sized", "--tmax", "100"],
                                   ["--layout", "sized", "--tmax", "0"], ["--tmax", "64"], ["--layout", "wide"]])
def test_cli_refuses_bad_layout_options(tmp_path, flags):
    files, _ = _library(tmp_path, "r", 1, 10, 2)
    rc, so, se = _run("index", *flags, str(tmp_path / "bad"), *files)
    assert "[Indexing Parser Error]" in se and not os.path.exists(tmp_path / "bad.ibf"), se
