"""`tetrex search --window W [--step S]` on indexes that `tetrex index` builds from generated FASTA: for each
alphabet and layout the rows of the command against tests/search_window_ref.py over the oracle restatement of the index file
(so Bloom false positives are expected, not tolerated): exact equality of the row lists, with and without --counts.  The query
records are chimeras — a segment of bin A with 0 to 2 edits at the front, random letters, a segment of bin B at the end, the
segments 2 W long — and a record shorter than W, one shorter than k, one of exactly W and one whose length forces the
end-aligned tail window.

What the rows of a chimera must cover.  A window that lies inside a planted segment is within E = 2 edits of a substring of
the bin, so it is hit (q-gram lemma).  Segment A begins with the record, where window 0 begins, and the windows inside it are
S apart: their union is letters 1 .. at least len(A) - S + 1.  Segment B ends with the record, where the last window ends
(the tail window where need be), and holds every window that begins at or behind its first letter: their union is from at
most letter L - len(B) + S to L.  Both intervals are asserted on the expected rows; so is that the plain search of the same
file under the same -e has no row at all for at least half of the chimeras."""
import os
import subprocess

import numpy as np
import pytest

from helpers import oracle_ibf_from_words
from search_ref import TreeRef, flat_search, csr
from search_window_ref import windows_of, threshold_of, search_rows
from test_gpu_search import _edit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TETREX = os.path.join(ROOT, "bin", "tetrex")

AMINO = "ACDEFGHIKLMNPQRSTVWY"
ALPHABETS = {  # name: (residues, k, index flags, dna, reduction, W, S)
    "peptide": (AMINO, 6, [], False, 0, 60, 15),
    "murphy": (AMINO, 5, ["-r", "murphy"], False, 1, 60, 15),
    "dna": ("ACGT", 16, ["-n"], True, 0, 150, 50),
}
LAYOUTS = {"flat": ["-i"], "default": [], "sized": ["--layout", "sized"]}
EDITS = 2
BINS = 40
CHIMERAS = 10


def _run(*args, env=None):
    r = subprocess.run([TETREX, *args], capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    return r.returncode, r.stdout, r.stderr


@pytest.fixture(scope="module")
def setups(tmp_path_factory):
    root = tmp_path_factory.mktemp("search_window")
    out = {}
    for name, (res, k, flags, dna, red, W, S) in ALPHABETS.items():
        rng = np.random.default_rng(100 + len(name))
        d = root / name
        d.mkdir()
        letters = lambda n: "".join(rng.choice(list(res), size=n))
        files, seqs = [], []
        for b in range(BINS):
            recs = [letters(int(rng.integers(2 * W + 20, 2 * W + 200))) for _ in range(2)]
            seqs.append(recs)
            p = d / ("bin%02d.fa" % b)
            p.write_text("".join(">b%d_%d\n%s\n" % (b, i, r) for i, r in enumerate(recs)))
            files.append(str(p))

        def cut(b, n):
            rec = seqs[b][int(rng.integers(0, 2))]
            at = int(rng.integers(0, len(rec) - n + 1))
            return rec[at:at + n]
        queries = []  # (name, letters, None | (bin A, len A, bin B, len B))
        for q in range(CHIMERAS):
            a, b = (int(x) for x in rng.choice(BINS, size=2, replace=False))
            sa = _edit(cut(a, 2 * W), int(rng.integers(0, EDITS + 1)), res, rng)
            sb = _edit(cut(b, 2 * W), int(rng.integers(0, EDITS + 1)), res, rng)
            queries.append(("chimera%d_b%d_b%d" % (q, a, b), sa + letters(W + int(rng.integers(0, S))) + sb, (a, len(sa), b, len(sb))))
        queries.append(("short", cut(3, W - 7), None))
        queries.append(("tiny", res[: k - 1], None))
        queries.append(("exact", cut(5, W), None))
        queries.append(("tail", cut(7, W + S + 1), None))
        qf = d / "queries.fa"
        qf.write_text("".join(">%s some comment\n%s\n" % (n, s) for n, s, _ in queries))
        indexes = {}
        for lay, lflags in LAYOUTS.items():
            rc, so, se = _run("index", "-k", str(k), *flags, *lflags, str(d / lay), *files)
            assert rc == 0 and os.path.exists(d / (lay + ".ibf")), se
            indexes[lay] = str(d / (lay + ".ibf"))
        out[name] = dict(files=[os.path.abspath(f) for f in files], queries=queries, qfile=str(qf), indexes=indexes, k=k, dna=dna, red=red, W=W, S=S)
    return out


def _restatement(oracle, path):
    """search(values, offsets, thresholds) -> (hits, counts) of the index file, and its bin paths"""
    from tetrex_amd import host
    ix = host.IndexFile.load(path)
    d = ix.describe()
    if d["is_hibf"]:
        descs = []
        for i, f in enumerate(d["ibfs"]):
            nxt, tbu = ix.maps(i)
            descs.append(dict(bins=f["bins"], bin_size=f["bin_size"], hash_funs=f["hash_funs"], words=ix.words(i), next_ibf_id=nxt, tb_to_user=tbu))
        return TreeRef(oracle, d["bins"], descs).search, d["paths"]
    f = d["ibfs"][0]
    ox = oracle_ibf_from_words(oracle, f["bins"], f["bin_size"], f["hash_funs"], ix.words(0))
    return (lambda v, o, t: flat_search(ox, f["bins"], v, o, t)), d["paths"]


def _expected(oracle, setup, layout, errors=None, fraction=None):
    """(rows with counts, notes, windows searched, whole-record hits) the restatement gives for the query file on one index"""
    from tetrex_amd import host
    k, W, S = setup["k"], setup["W"], setup["S"]
    search, paths = _restatement(oracle, setup["indexes"][layout])
    vals = [host.record_values_array(s, k, dna=setup["dna"], reduction=setup["red"]) for _, s, _ in setup["queries"]]
    # every window of every record as a query of its own, answered in one call
    at, qs, thr = {}, [], []
    for r, (_, s, _) in enumerate(setup["queries"]):
        for b, n in windows_of(len(s), k, W, S):
            at[(r, b, n)] = len(qs)
            qs.append(vals[r][b:b + n - k + 1])
            assert qs[-1].size == n - k + 1  # letters map to values one to one
            thr.append(threshold_of(n - k + 1, k, errors, fraction))
    v, off = csr(qs)
    hits, counts = search(v, off, np.array(thr, dtype=np.uint32))
    records = [(n, s) for n, s, _ in setup["queries"]]
    rows, notes = search_rows(records, k, W, S, lambda r, b, n: counts[at[(r, b, n)]], len(paths), errors, fraction, with_counts=True)
    rows = [(n, paths[u]) + tuple(str(x) for x in rest) for n, u, *rest in rows]
    # the plain search of the same records: one query a record
    whole = [(n, x) for (n, _, _), x in zip(setup["queries"], vals) if x.size]
    wv, woff = csr([x for _, x in whole])
    wthr = np.array([threshold_of(x.size, k, errors, fraction) for _, x in whole], dtype=np.uint32)
    whits, _ = search(wv, woff, wthr)
    whole_hit = {n: bool(whits[i].any()) for i, (n, _) in enumerate(whole)}
    return rows, notes, sum(1 for t in thr if t > 0), whole_hit


@pytest.mark.parametrize("alphabet", list(ALPHABETS))
def test_cli_search_window(oracle, setups, tmp_path, alphabet):
    setup = setups[alphabet]
    k, W, S = setup["k"], setup["W"], setup["S"]
    for layout, path in setup["indexes"].items():
        want, (skipped, unsearched), n_searched, whole_hit = _expected(oracle, setup, layout, errors=EDITS)
        assert skipped == ["tiny"] and unsearched == []
        # non-vacuity, on the expected side: both segments of every chimera are found where they were planted ...
        for name, s, plant in setup["queries"]:
            if not plant:
                continue
            a, la, b, lb = plant
            L = len(s)
            rows_a = [(int(r[2]), int(r[3])) for r in want if r[0] == name and r[1] == setup["files"][a]]
            rows_b = [(int(r[2]), int(r[3])) for r in want if r[0] == name and r[1] == setup["files"][b]]
            assert any(x == 1 and y >= la - S + 1 for x, y in rows_a), (alphabet, layout, name, rows_a)
            assert any(x <= L - lb + S and y == L for x, y in rows_b), (alphabet, layout, name, rows_b)
        # ... and the plain search finds nothing at all for at least half of them
        chimeras = [n for n, _, p in setup["queries"] if p]
        assert sum(1 for n in chimeras if not whole_hit[n]) * 2 >= len(chimeras), (alphabet, layout)
        for n in ("short", "exact", "tail"):
            assert any(r[0] == n for r in want), n
        rc, so, se = _run("search", "--window", str(W), "--step", str(S), "-e", str(EDITS), "--counts", "-v", path, setup["qfile"])
        assert rc == 0, se
        assert "tiny: no k-mer" in se and "Search time:" in se
        got = [tuple(line.split("\t")) for line in so.splitlines()]
        assert got == want, (alphabet, layout)
        hit_windows = None
        for line in se.splitlines():
            if line.startswith("Windows: "):
                w = line.split()
                assert w[2:] == ["searched,", w[3], "hit,", w[5], "rows"] and int(w[1]) == n_searched and int(w[5]) == len(want), line
                hit_windows = int(w[3])
        assert hit_windows is not None and 0 < hit_windows <= n_searched
        # without --counts: the same rows less their last column; -o
        dest = tmp_path / ("%s_%s.tsv" % (alphabet, layout))
        rc, so2, se = _run("search", "--window", str(W), "--step", str(S), "-e", str(EDITS), "-o", str(dest), path, setup["qfile"])
        assert rc == 0 and so2 == "", se
        assert [tuple(line.split("\t")) for line in dest.read_text().splitlines()] == [r[:4] for r in want], (alphabet, layout)
        # batches of 7 windows (runs are merged across them, tails of values sent again): the same bytes
        rc, so3, se = _run("search", "--window", str(W), "--step", str(S), "-e", str(EDITS), "--counts", path, setup["qfile"],
                           env={"TETREX_SEARCH_BATCH_WINDOWS": "7"})
        assert rc == 0 and so3 == so, se
        rc, so4, se = _run("search", "--window", str(W), "--step", str(S), "-e", str(EDITS), "--counts", path, setup["qfile"],
                           env={"TETREX_SEARCH_BATCH_WINDOWS": "1", "TXQ_COUNT_WINDOWS_UNIT": "3"})
        assert rc == 0 and so4 == so, se


@pytest.mark.parametrize("alphabet", ["peptide", "dna"])
def test_cli_threshold_default_step_and_unsearched_windows(oracle, setups, alphabet):
    setup = dict(setups[alphabet])  # (the default step: W / 2)
    k, W = setup["k"], setup["W"]
    setup["S"] = max(1, W // 2)
    path = setup["indexes"]["flat"]
    want, _, _, _ = _expected(oracle, setup, "flat", fraction=0.7)
    rc, so, se = _run("search", "--window", str(W), "--threshold", "0.7", path, setup["qfile"])
    assert rc == 0, se
    assert [tuple(line.split("\t")) for line in so.splitlines()] == [r[:4] for r in want]
    assert want
    # -e so large that the short record's one window has threshold 0 while full windows keep one: a note, no row for it
    E = (W - 7 - k + 1) // k  # short has W - 7 letters: w = W - 7 - k + 1 <= k E
    assert W - k + 1 > k * E
    want, (skipped, unsearched), _, _ = _expected(oracle, setup, "flat", errors=E)
    assert unsearched == ["short"]
    rc, so, se = _run("search", "--window", str(W), "-e", str(E), "--counts", path, setup["qfile"])
    assert rc == 0, se
    assert [tuple(line.split("\t")) for line in so.splitlines()] == want
    assert se.count("short: a window with threshold 0 is not searched") == 1 and not any(r[0] == "short" for r in want)


def test_cli_refusals_that_need_the_index(setups, tmp_path):
    setup = setups["peptide"]
    path, k = setup["indexes"]["flat"], setup["k"]
    dest = tmp_path / "out.tsv"
    rc, so, se = _run("search", "--window", str(k - 1), "-e", "0", "-o", str(dest), path, setup["qfile"])
    assert rc != 0 and se.startswith("[Search Parser Error] --window must be") and "k = %d" % k in se and so == "" and not dest.exists()
    # W - k + 1 <= k E: every full window would have threshold 0; the smallest workable W is k E + k
    rc, so, se = _run("search", "--window", "17", "-e", "2", "-o", str(dest), path, setup["qfile"])
    assert rc != 0 and se.startswith("[Search Parser Error] ") and "smallest workable --window is 18" in se and so == "" and not dest.exists()
    rc, so, se = _run("search", "--window", "18", "-e", "2", "-o", str(dest), path, setup["qfile"])
    assert rc == 0 and dest.exists(), se
    # without --window nothing changes: the plain search of the chimeras still runs
    rc, so, se = _run("search", "-e", "2", path, setup["qfile"])
    assert rc == 0, se
