"""`tetrex index --layout sized --rearrange` on the GPU (csrc/txq_build.hip pair_union_kernel, host/layout.hpp): the pairwise
union estimates against numpy bit for bit, a rearranged tree of a FASTA family library against an independent rebuild in the
CPU oracle and against the numpy restatement of the rule, the unchanged bytes of builds without the option, and the CLI."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import rearrange_ref as RR
from conftest import ROOT
from family_fasta import family_library
from motifs import random_prosite_motifs
from sized_hibf_ref import MERGED, estimate, part_of, paths, registers

pytestmark = pytest.mark.gpu
TETREX = os.path.join(ROOT, "bin", "tetrex")
AA = "ACDEFGHIKLMNPQRSTVWY"

# SHA-256 of the serialised index that the PARENT commit builds from family_library(seed 1), k = 6, layout "sized",
# t_max 64 (file names relative to the library's directory): recorded from a build of the parent's sources on an MI355X,
# not from the code under test.
PARENT_SIZED_SHA256 = "9f58909bde3d0cd5e7f933b2a2154fb18c0c5835f87ad2d8b424e9a511895c3f"


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


# ---- the kernel against numpy ------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def sketches(capi):
    rng = np.random.default_rng(23)
    bins = [np.zeros(0, dtype=np.uint64), np.array([12345], dtype=np.uint64),
            rng.integers(0, 1 << 40, size=1_000_000, dtype=np.uint64), np.zeros(0, dtype=np.uint64)]
    shared = rng.integers(0, 1 << 40, size=30_000, dtype=np.uint64)
    for b in range(36):
        own = rng.integers(0, 1 << int(rng.integers(8, 40)), size=int(rng.integers(1, 40_000)), dtype=np.uint64)
        bins.append(np.concatenate([shared[: int(rng.integers(0, shared.size))], own]) if b % 3 else own)
    regs = capi.sketch(bins)
    for b, v in enumerate(bins):
        assert np.array_equal(regs[b], registers(v)), b
    return regs


@pytest.mark.parametrize("n", [1, 2, 3, 65, 300])
def test_pair_unions_equal_the_numpy_estimate(capi, sketches, n):
    regs = sketches
    B = regs.shape[0]
    rng = np.random.default_rng(n)
    if n <= B:
        ids = rng.permutation(B)[:n]  # random order
        if n == 3:
            ids = np.array([2, 0, 1])  # the bin of 10^6 values, an empty bin, the one-value bin
    else:
        ids = np.concatenate([rng.permutation(B), rng.integers(0, B, size=n - B)])  # every bin, then repeats
    ids = ids.astype(np.uint32)
    got = capi.pair_unions(regs, ids)
    assert got.shape == (n, n) and got.dtype == np.float64
    # the restatement over the distinct pairs of bins, spread over the ids
    table = {}
    want = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            a, b = sorted((int(ids[i]), int(ids[j])))
            if (a, b) not in table:
                table[(a, b)] = estimate(np.maximum(regs[a], regs[b]))
            want[i, j] = table[(a, b)]
    assert np.array_equal(got, want)
    own = capi.union_estimates(regs, np.arange(B, dtype=np.uint32), 1)[:, 0]
    assert np.array_equal(np.diag(got), own[ids])
    if n == 65:
        assert np.array_equal(capi.pair_unions(regs, np.full(5, 7, dtype=np.uint32)), np.full((5, 5), own[7]))
        assert np.array_equal(RR.pair_unions(regs, ids[:9]), got[:9, :9])  # the restatement the order test relies on


def test_pair_unions_refusals(capi, sketches):
    L = capi.lib()
    L.txq_pair_unions_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    dr = capi.DeviceBuffer.from_numpy(sketches)
    di = capi.DeviceBuffer.from_numpy(np.zeros(4097, dtype=np.uint32))
    de = capi.DeviceBuffer(64 * 8)
    try:
        assert L.txq_pair_unions_device(None, None, 0, None, None) == 0  # n = 0: a no-op
        assert L.txq_pair_unions_device(dr.ptr, di.ptr, 0, de.ptr, None) == 0
        assert L.txq_pair_unions_device(None, di.ptr, 4, de.ptr, None) == -1
        assert L.txq_pair_unions_device(dr.ptr, None, 4, de.ptr, None) == -1
        assert L.txq_pair_unions_device(dr.ptr, di.ptr, 4, None, None) == -1
        assert L.txq_pair_unions_device(dr.ptr, di.ptr, 4097, de.ptr, None) == -1  # would not fit de: refused before a launch
        capi.synchronize()
    finally:
        for b in (dr, di, de):
            b.free()
    with pytest.raises(capi.TxqError) as e:
        capi.pair_unions(sketches, np.zeros(4097, dtype=np.uint32))
    assert e.value.code == -1
    assert capi.pair_unions(sketches, np.zeros(0, dtype=np.uint32)).shape == (0, 0)


# ---- a rearranged tree -------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def families(tmp_path_factory):
    d = tmp_path_factory.mktemp("families")
    names, recs, fam = family_library(str(d))
    return str(d), names, recs, fam


def _values(recs, k):
    from tetrex_amd import host
    out = []
    for seqs in recs:
        vs = [host.record_values_array(s, k, False, 0, True) for s in seqs if len(s) >= k]
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


def _rebuild(oracle, ibfs, values, k):
    """The tree's bits from its maps alone (as tests/test_gpu_sized_hibf.py rebuilds the plain sized tree)."""
    ox = oracle.Index.hibf(len(values), dna=False, k=k, reduction=0)
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


def _depth_first_bins(ibfs):
    out = []

    def walk(i):
        last = None
        for t, ub in enumerate(ibfs[i]["tb_to_user_bin"]):
            ub = int(ub)
            if ub == MERGED:
                walk(int(ibfs[i]["next_ibf_id"][t]))
                last = None
            elif ub != last:
                out.append(ub)
                last = ub
    walk(0)
    return out


def _build(names, **kw):
    from tetrex_amd import host
    return host.IndexFile.build(names, k=6, layout="sized", tmax=64, **kw)


def test_family_tree_rebuilds_answers_and_is_smaller(capi, oracle, families, monkeypatch):
    d, names, recs, fam = families
    monkeypatch.chdir(d)
    k, B = 6, len(names)
    ix = _build(names, rearrange=0.5)
    desc, ibfs = _tree(ix)
    assert desc["is_hibf"] and sum(1 for f in ibfs for u in f["tb_to_user"] if int(u) == MERGED) >= 10
    values = _values(recs, k)
    assert sum(1 for v in values if not v.size) == 4
    # the same words in every IBF as an independent rebuild from the maps
    ox = _rebuild(oracle, ibfs, values, k)
    for i in range(len(ibfs)):
        assert np.array_equal(ox.hibf_words(i), ibfs[i]["words"]), i
    # no false negatives, on the device and in the oracle
    dx = capi.Index.upload_hibf(B, ibfs)
    for b in range(B):
        if not values[b].size:
            continue
        for masks in (dx.probe(values[b]), ox.probe(values[b])):
            assert np.all((masks[:, b // 64] >> np.uint64(b % 64)) & np.uint64(1)), b
    # 100 PROSITE-style motifs: the oracle's masks
    qs = random_prosite_motifs(100, 46)
    got, status, _ = dx.query_masks(qs, False, k)
    compared = 0
    for q, g, st in zip(qs, got, status):
        want, ost = ox.query(q, with_stats=True)
        assert st == 0, q
        if not ost["quirk_merges"]:
            compared += 1
            assert np.array_equal(g, want), q
    assert compared >= 50, compared
    dx.free()
    # the order of the tree is the restatement's, computed from the device's sketches
    regs = capi.sketch(values)
    counts = np.array([estimate(r) for r in regs])
    assert np.array_equal(counts, capi.union_estimates(regs, np.arange(B, dtype=np.uint32), 1)[:, 0])
    want_order, starts = RR.rearranged_order(counts, regs, 0.5)
    order = _depth_first_bins(ibfs)
    assert order == want_order
    assert order != RR.sorted_order(counts) and max(e - s for s, e in zip(starts, starts[1:] + [B])) >= 3
    near = sum(fam[order[i]] >= 0 and fam[order[i]] == fam[order[i + 1]] for i in range(B - 1))
    # strictly smaller than the tree over the sorted order
    plain = _build(names)
    assert _depth_first_bins(_tree(plain)[1]) == RR.sorted_order(counts)
    a, b = len(plain.serialise()), len(ix.serialise())
    print("family library, %d files: %d bytes sorted, %d bytes rearranged, ratio %.3f; %d interval(s); same-family neighbours %d of %d"
          % (B, a, b, b / a, len(starts), near, B - 1))
    assert b < a


def test_builds_without_the_option_keep_the_parents_bytes(capi, families, monkeypatch):
    d, names, _, _ = families
    monkeypatch.chdir(d)
    images = [_build(names).serialise(), _build(names, rearrange=None).serialise(), _build(names, rearrange=0).serialise()]
    assert images[0] == images[1] == images[2]
    digest = hashlib.sha256(images[0]).hexdigest()
    print("sha256 of the sized index without --rearrange:", digest)
    assert digest == PARENT_SIZED_SHA256
    from tetrex_amd import host
    with pytest.raises(host.HostError):
        _build(names, rearrange=1.5)
    with pytest.raises(host.HostError):
        host.IndexFile.build(names, k=6, layout="uniform", rearrange=True)


# ---- CLI ---------------------------------------------------------------------------------------------------------------


def _run(*args, cwd=None):
    r = subprocess.run([TETREX, *args], capture_output=True, text=True, cwd=cwd, timeout=600)
    return r.returncode, r.stdout, r.stderr


def _seq(rng, n):
    return "".join(rng.choice(list(AA), size=n))


def _library(d, name, seed, n_bins, giant_records):
    """One giant bin (bin 1), eight medium bins, tiny bins (the recipe of tests/test_gpu_sized_hibf.py)."""
    rng = np.random.default_rng(seed)
    files, recs = [], []
    for b in range(n_bins):
        if b == 1:
            seqs = [_seq(rng, 200) for _ in range(giant_records)]
        elif b % max(1, n_bins // 8) == 3:
            seqs = [_seq(rng, 120) for _ in range(8)]
        else:
            seqs = [_seq(rng, int(rng.integers(30, 70)))]
        p = d / ("%s%04d.fa" % (name, b))
        p.write_text("".join(">r%d_%d\n%s\n" % (b, i, s) for i, s in enumerate(seqs)))
        files.append(str(p))
        recs.append(seqs)
    return files, recs


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


def test_cli_rearranged_indexes_answer_like_a_flat_index(tmp_path):
    files, recs = _library(tmp_path, "c", 21, 300, 120)
    builds = (("flat", ["-i"]), ("sized", ["--layout", "sized"]), ("half", ["--layout", "sized", "--rearrange"]),
              ("quarter", ["--layout", "sized", "--rearrange", "--rearrange-ratio", "0.25"]),
              ("again", ["--rearrange", "--layout", "sized"]))
    for name, flags in builds:
        rc, so, se = _run("index", "-k", "5", *flags, str(tmp_path / name), *files)
        assert rc == 0 and "across 300 bins." in se, se
    assert open(tmp_path / "half.ibf", "rb").read() == open(tmp_path / "again.ibf", "rb").read()
    rng = np.random.default_rng(5)
    motifs = _planted(recs, rng, 8)
    for q in motifs:
        out = {}
        for name in ("flat", "half", "quarter"):
            rc, so, se = _run("query", "-v", str(tmp_path / (name + ".ibf")), q)
            assert rc == 0, se
            out[name] = sorted(so.splitlines())
        assert out["flat"] == out["half"] == out["quarter"] and out["flat"], q
    # planted records: windows of the library's records with one substitution each, and one record of no bin
    picks = [(int(b), int(rng.integers(0, len(recs[b])))) for b in rng.integers(0, 300, size=40)]
    lines = []
    for i, (b, r) in enumerate(picks):
        s = recs[b][r]
        a = int(rng.integers(0, max(1, len(s) - 40)))
        w = list(s[a:a + 40])
        at = int(rng.integers(0, len(w)))
        w[at] = AA[(AA.index(w[at]) + 1) % 20]
        lines.append(">q%d\n%s\n" % (i, "".join(w)))
    lines.append(">nowhere\n%s\n" % _seq(rng, 60))
    (tmp_path / "q.fa").write_text("".join(lines))
    res = {}
    for name in ("flat", "half", "quarter"):
        rc, so, se = _run("search", "-e", "1", str(tmp_path / (name + ".ibf")), str(tmp_path / "q.fa"))
        assert rc == 0, se
        res[name] = sorted(so.splitlines())
    assert res["flat"] == res["half"] == res["quarter"]
    reported = {tuple(line.split("\t")[:2]) for line in res["half"]}
    for i, (b, _) in enumerate(picks):
        assert ("q%d" % i, files[b]) in reported, i
    assert not any(line.startswith("nowhere\t") for line in res["half"])


@pytest.mark.parametrize("flags", [["--rearrange"], ["--layout", "uniform", "--rearrange"], ["-i", "--rearrange"],
                                   ["--layout", "sized", "--rearrange-ratio", "0.5"],
                                   ["--layout", "sized", "--rearrange", "--rearrange-ratio", "0"],
                                   ["--layout", "sized", "--rearrange", "--rearrange-ratio", "1.5"],
                                   ["--layout", "sized", "--rearrange", "--rearrange-ratio", "-0.5"],
                                   ["--layout", "sized", "--rearrange", "--rearrange-ratio", "half"],
                                   ["--layout", "sized", "--rearrange", "--rearrange-ratio", "nan"]], ids=str)
def test_cli_refuses_bad_rearrange_options(tmp_path, flags):
    files, _ = _library(tmp_path, "r", 1, 10, 2)
    rc, so, se = _run("index", *flags, str(tmp_path / "bad"), *files)
    assert "[Indexing Parser Error]" in se and not os.path.exists(tmp_path / "bad.ibf"), se
