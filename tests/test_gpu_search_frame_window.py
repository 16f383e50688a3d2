"""`tetrex search --translate --frame-window W [--frame-step S]` on indexes that `tetrex index` builds from generated FASTA
(DESIGN.md §18): for each alphabet and layout the rows of the command against tests/frame_window_ref.py over the oracle
restatement of the index file (so Bloom false positives are expected, not tolerated): exact equality of the row lists, with
and without --counts.  The query records are contigs — random nucleotides, a segment of 2 W residues of bin A with 0 to 2
residue edits back-translated at a frame offset drawn per contig, random nucleotides, the reverse complement of such a segment
of bin B, random nucleotides — and a record shorter than 3 k, one whose best frame has exactly W residues, one that forces
the end-aligned tail window and one of W - 7 residues.

What the rows of a contig must cover.  A window that lies inside a planted segment is stop-free and within E = 2 edits of a
substring of the bin, so it is hit (q-gram lemma).  The windows of a frame begin S apart, so the windows inside the segment's
residues [s, e) are consecutive and their union holds at least [s + S - 1, e - S + 1): one row of the segment's bin and frame
covers those residues' nucleotides.  That is asserted on the expected rows; so is that plain `--translate -e 2` has no row at
all for at least half of the contigs (a planted segment is about a third of its frame's k-mers, so n_f - k E is out of reach)."""
import math
import os
import subprocess

import numpy as np
import pytest

import frame_window_ref as F
import translate_ref as T
from helpers import oracle_ibf_from_words
from search_ref import TreeRef, flat_search, csr
from search_window_ref import threshold_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TETREX = os.path.join(ROOT, "bin", "tetrex")

AMINO = "ACDEFGHIKLMNPQRSTVWY"
ALPHABETS = {"peptide": (6, [], 0), "murphy": (5, ["-r", "murphy"], 1)}  # name: (k, index flags, reduction)
LAYOUTS = {"flat": ["-i"], "default": [], "sized": ["--layout", "sized"]}
W, S, EDITS = 40, 10, 2
BINS = 24
CONTIGS = 10
CODONS_OF = {}
for _codon, _aa in T.CODON.items():
    CODONS_OF.setdefault(_aa, []).append(_codon)


def _run(*args, env=None):
    r = subprocess.run([TETREX, *args], capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    return r.returncode, r.stdout, r.stderr


def _nt(rng, n):
    return "".join(rng.choice(list("ACGT"), size=n))


def _edit(seq, e, rng):
    """e residue-level substitutions or indels (never a stop: the segment stays stop-free)"""
    s = list(seq)
    for _ in range(e):
        kind = int(rng.integers(0, 3))
        at = int(rng.integers(1, len(s) - 1))
        if kind == 0:
            s[at] = AMINO[(AMINO.index(s[at]) + 1 + int(rng.integers(0, len(AMINO) - 1))) % len(AMINO)]
        elif kind == 1:
            s.insert(at, AMINO[int(rng.integers(0, len(AMINO)))])
        else:
            del s[at]
    return "".join(s)


def _back(pep, rng):
    return "".join(CODONS_OF[a][int(rng.integers(0, len(CODONS_OF[a])))] for a in pep)


@pytest.fixture(scope="module")
def setups(tmp_path_factory):
    root = tmp_path_factory.mktemp("search_frame_window")
    out = {}
    for name, (k, flags, red) in ALPHABETS.items():
        rng = np.random.default_rng(200 + len(name))
        d = root / name
        d.mkdir()
        files, seqs = [], []
        for b in range(BINS):
            recs = ["".join(rng.choice(list(AMINO), size=int(rng.integers(2 * W + 20, 2 * W + 200)))) for _ in range(2)]
            seqs.append(recs)
            p = d / ("bin%02d.fa" % b)
            p.write_text("".join(">b%d_%d\n%s\n" % (b, i, r) for i, r in enumerate(recs)))
            files.append(str(p))

        def cut(b, n):
            rec = seqs[b][int(rng.integers(0, 2))]
            at = int(rng.integers(0, len(rec) - n + 1))
            return rec[at:at + n]
        queries = []  # (name, nucleotides, None | [(bin, frame, first residue, end residue) of the two planted segments])
        for q in range(CONTIGS):
            a, b = (int(x) for x in rng.choice(BINS, size=2, replace=False))
            pa = _edit(cut(a, 2 * W), int(rng.integers(0, EDITS + 1)), rng)
            pb = _edit(cut(b, 2 * W), int(rng.integers(0, EDITS + 1)), rng)
            o = int(rng.integers(0, 3))
            front = _nt(rng, 3 * int(rng.integers(20, 30)) + o)
            middle, behind = _nt(rng, int(rng.integers(60, 90))), _nt(rng, int(rng.integers(60, 90)))
            nt = front + _back(pa, rng) + middle + T.reverse_complement(_back(pb, rng)) + behind
            fb = 3 + len(behind) % 3
            plants = [(a, o, len(front) // 3, len(front) // 3 + len(pa)), (b, fb, len(behind) // 3, len(behind) // 3 + len(pb))]
            for _, f, s, e in plants:
                assert T.translate_frame(nt, f)[s:e] in (pa, pb)
            queries.append(("contig%d_b%d_b%d" % (q, a, b), nt, plants))
        queries.append(("tiny", _nt(rng, 3 * k - 1), None))
        queries.append(("exact", _back(cut(5, W), rng), None))
        queries.append(("tail", _back(cut(7, W + S + 1), rng) + "A", None))
        queries.append(("short", _back(cut(3, W - 7), rng), None))
        qf = d / "contigs.fa"
        qf.write_text("".join(">%s some comment\n%s\n" % (n, s) for n, s, _ in queries))
        indexes = {}
        for lay, lflags in LAYOUTS.items():
            rc, so, se = _run("index", "-k", str(k), *flags, *lflags, str(d / lay), *files)
            assert rc == 0 and os.path.exists(d / (lay + ".ibf")), se
            indexes[lay] = str(d / (lay + ".ibf"))
        out[name] = dict(files=[os.path.abspath(f) for f in files], queries=queries, qfile=str(qf), indexes=indexes, k=k, red=red, dir=d)
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


_expected_cache = {}


def _expected(oracle, setup, layout, step, errors=None, fraction=None):
    """(rows with counts, notes, windows searched) the restatement gives for the query file on one index, computed once"""
    key = (setup["qfile"], layout, step, errors, fraction)
    if key in _expected_cache:
        return _expected_cache[key]
    k, red = setup["k"], setup["red"]
    search, paths = _restatement(oracle, setup["indexes"][layout])
    # every window of every frame as a query of its own, answered in one call
    at, qs, thr = {}, [], []
    for r, (_, s, _) in enumerate(setup["queries"]):
        for f in range(6):
            values = T.frame_values(s, f, k, red)
            for j, (b, w) in enumerate(F.window_ranges(s, f, k, W, step)):
                assert b + w <= values.size
                at[(r, f, j)] = len(qs)
                qs.append(values[b:b + w])
                thr.append(threshold_of(w, k, errors, fraction) if w else 0)
    v, off = csr(qs)
    hits, counts = search(v, off, np.array(thr, dtype=np.uint32))
    records = [(n, s) for n, s, _ in setup["queries"]]
    rows, notes, n_searched = F.search_rows(records, k, W, step, lambda r, f, j: counts[at[(r, f, j)]], len(paths), errors, fraction, with_counts=True)
    rows = [(n, paths[u]) + tuple(str(x) for x in rest) for n, u, *rest in rows]
    assert n_searched == sum(1 for t in thr if t > 0)
    _expected_cache[key] = (rows, notes, n_searched)
    return _expected_cache[key]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("alphabet", list(ALPHABETS))
def test_cli_search_frame_window(oracle, setups, tmp_path, alphabet, layout):
    setup = setups[alphabet]
    k, path = setup["k"], setup["indexes"][layout]
    want, (no_kmer, unsearched), n_searched = _expected(oracle, setup, layout, S, errors=EDITS)
    assert no_kmer == ["tiny"] and unsearched == []
    # non-vacuity, on the expected side: both segments of every contig are found where they were planted ...
    for name, s, plants in setup["queries"]:
        for b, f, rs, re in plants or []:
            nb, ne = F.residues_on_record(len(s), f, rs + S - 1, re - S + 1)
            rows = [(int(r[3]), int(r[4])) for r in want if r[0] == name and r[1] == setup["files"][b] and r[2] == T.FRAMES[f]]
            assert any(x <= nb and y >= ne for x, y in rows), (alphabet, layout, name, T.FRAMES[f], (nb, ne), rows)
    for n in ("exact", "tail", "short"):
        assert any(r[0] == n for r in want), n
    # ... and plain --translate finds nothing at all for at least half of them
    rc, pso, pse = _run("search", "--translate", "-e", str(EDITS), path, setup["qfile"])
    assert rc == 0, pse
    plain = {line.split("\t")[0] for line in pso.splitlines()}
    contigs = [n for n, _, p in setup["queries"] if p]
    assert sum(1 for n in contigs if n not in plain) * 2 >= len(contigs), (alphabet, layout, sorted(plain))
    flags = ["search", "--translate", "--frame-window", str(W), "--frame-step", str(S), "-e", str(EDITS)]
    rc, so, se = _run(*flags, "--counts", "-v", path, setup["qfile"])
    assert rc == 0, se
    assert "[tetrex search] tiny: no frame" in se and "Search time:" in se and "no window with a threshold" not in se
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
    rc, so2, se = _run(*flags, "-o", str(dest), path, setup["qfile"])
    assert rc == 0 and so2 == "", se
    assert [tuple(line.split("\t")) for line in dest.read_text().splitlines()] == [r[:5] for r in want], (alphabet, layout)
    # sub-ranges of 7 windows (runs are merged across them), and of one window with units of 3: the same bytes
    rc, so3, se = _run(*flags, "--counts", path, setup["qfile"], env={"TETREX_SEARCH_BATCH_WINDOWS": "7", "TETREX_TRACE": "1"})
    assert rc == 0 and so3 == so, se
    assert se.count("frame window batch:") > 10
    rc, so4, se = _run(*flags, "--counts", path, setup["qfile"], env={"TETREX_SEARCH_BATCH_WINDOWS": "1", "TXQ_COUNT_WINDOWS_UNIT": "3"})
    assert rc == 0 and so4 == so, se


@pytest.mark.parametrize("alphabet", list(ALPHABETS))
def test_cli_threshold_default_step_and_unsearched_record(oracle, setups, alphabet):
    setup = setups[alphabet]
    k, path = setup["k"], setup["indexes"]["flat"]
    want, _, _ = _expected(oracle, setup, "flat", W // 2, fraction=0.7)  # (the default step: W / 2)
    rc, so, se = _run("search", "--translate", "--frame-window", str(W), "--threshold", "0.7", path, setup["qfile"])
    assert rc == 0, se
    assert [tuple(line.split("\t")) for line in so.splitlines()] == [r[:5] for r in want]
    assert want
    # -e so large that every window of the short record has threshold 0 while stop-free full windows keep one: one note, no row
    E = math.ceil((W - 7 - k + 1) / k)
    assert W - k + 1 > k * E >= W - 7 - k + 1
    want, (no_kmer, unsearched), _ = _expected(oracle, setup, "flat", S, errors=E)
    assert "short" in unsearched and "tiny" in no_kmer
    rc, so, se = _run("search", "--translate", "--frame-window", str(W), "--frame-step", str(S), "-e", str(E), "--counts", path, setup["qfile"])
    assert rc == 0, se
    assert [tuple(line.split("\t")) for line in so.splitlines()] == want
    assert se.count("short: no window with a threshold above 0") == 1 and not any(r[0] == "short" for r in want)
    for n, _, _ in setup["queries"]:
        assert (("[tetrex search] %s: no window with a threshold above 0" % n) in se) == (n in unsearched), n
        assert (("[tetrex search] %s: no frame" % n) in se) == (n in no_kmer), n


def test_cli_refusals_that_need_the_index(setups, tmp_path):
    setup = setups["peptide"]
    path, k = setup["indexes"]["flat"], setup["k"]
    dest = tmp_path / "out.tsv"
    rc, so, se = _run("search", "--translate", "--frame-window", str(k - 1), "-e", "0", "-o", str(dest), path, setup["qfile"])
    assert rc != 0 and se.startswith("[Search Parser Error] --frame-window must be") and "k = %d" % k in se and so == "" and not dest.exists()
    # W - k + 1 <= k E: every window would have threshold 0; the smallest workable W is k E + k
    rc, so, se = _run("search", "--translate", "--frame-window", "17", "-e", "2", "-o", str(dest), path, setup["qfile"])
    assert rc != 0 and se.startswith("[Search Parser Error] ") and "smallest workable --frame-window is 18" in se and so == "" and not dest.exists()
    rc, so, se = _run("search", "--translate", "--frame-window", "18", "-e", "2", "-o", str(dest), path, setup["qfile"])
    assert rc == 0 and dest.exists(), se
    # a nucleotide index is refused, as --translate refuses it
    d = setup["dir"]
    rng = np.random.default_rng(1)
    files = []
    for b in range(2):
        p = d / ("nt%d.fa" % b)
        p.write_text(">n%d\n%s\n" % (b, _nt(rng, 400)))
        files.append(str(p))
    rc, so, se = _run("index", "-n", "-k", "16", "-i", str(d / "nt"), *files)
    assert rc == 0, se
    dest2 = tmp_path / "out2.tsv"
    rc, so, se = _run("search", "--translate", "--frame-window", "40", "-e", "2", "-o", str(dest2), str(d / "nt.ibf"), setup["qfile"])
    assert rc != 0 and "--translate needs a peptide index" in se and so == "" and not dest2.exists()
    # without the new flags nothing changes: plain --translate of the contigs still runs
    rc, so, se = _run("search", "--translate", "-e", "2", path, setup["qfile"])
    assert rc == 0, se
