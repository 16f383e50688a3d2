"""`tetrex search --translate --frame-window W [--frame-step S] -e E --verify-frame-windows` on indexes that
`tetrex index` builds from generated FASTA, against the Python restatement tests/verify_frame_windows_ref.py: the frames and
windows of tests/frame_window_ref.py, the distances of tests/edit_ref.py (a stop matches nothing) and the run merge.  The
queries are nucleotide chimeras — random flank, a back-translated stretch of one bin with 0..E residue edits, flank, the
reverse complement of such a stretch of another bin, flank, a stretch of a third bin in which one codon is a stop and at most
E - 1 further residues are edited (it must still be covered: the guarantee §18 does not give), flank, and a decoy: a stretch of
a fourth bin with blocks of E + 2 adjacent substitutions so close that every window in it holds one, which the k-mer filter
lets through and verification must reject — and a few records whose frames have at most W residues."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import frame_window_ref as F
import translate_ref as T
import verify_frame_windows_ref as R
from helpers import oracle_ibf_from_words
from search_ref import TreeRef, flat_search, csr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TETREX = os.path.join(ROOT, "bin", "tetrex")
AMINO = "ACDEFGHIKLMNPQRSTVWY"
ALPHABETS = {"peptide": (6, [], 0), "murphy": (5, ["-r", "murphy"], 1)}  # name: (k, index flags, reduction)
LAYOUTS = {"flat": ["-i"], "default": [], "sized": ["--layout", "sized"]}
W, S, EDITS, BINS, CHIMERAS, SHORT = 40, 10, 2, 24, 5, 4
SEEDS = {"peptide": 501, "murphy": 502}  # (settled on the CPU: generate() with the restatement alone meets check_case())
CODONS_OF = {}
for _codon, _aa in T.CODON.items():
    CODONS_OF.setdefault(_aa, []).append(_codon)


def _run(*args, env=None):
    r = subprocess.run([TETREX, *args], capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    return r.returncode, r.stdout, r.stderr


def _nt(rng, n):
    return "".join(rng.choice(list("ACGT"), size=n))


def _back(pep, rng):
    return "".join(CODONS_OF[a][int(rng.integers(0, len(CODONS_OF[a])))] for a in pep)


def _edit(seq, e, rng):
    """e residue-level substitutions or indels (never a stop)"""
    s = list(seq)
    for _ in range(e):
        kind, at = int(rng.integers(0, 3)), int(rng.integers(1, len(s) - 1))
        if kind == 0:
            s[at] = AMINO[(AMINO.index(s[at]) + 1 + int(rng.integers(0, len(AMINO) - 1))) % len(AMINO)] if s[at] in AMINO else "A"
        elif kind == 1:
            s.insert(at, AMINO[int(rng.integers(0, len(AMINO)))])
        else:
            del s[at]
    return "".join(s)


def _substituted(rng, s):
    return "".join(AMINO[(AMINO.index(c) + 1 + int(rng.integers(0, len(AMINO) - 1))) % len(AMINO)] for c in s)


def generate(name):
    """the bins (two records each; bin 5's second one is long), the chimeric queries with where their stretches lie, the short
    queries, and the restatement's distances of every searched window of every query to every bin"""
    k = ALPHABETS[name][0]
    rng = np.random.default_rng(SEEDS[name])
    seqs = []
    for b in range(BINS):
        lens = [int(rng.integers(2 * W + 20, 2 * W + 200)) for _ in range(2)]
        if b == 5:
            lens[1] = 2200
        seqs.append(["".join(rng.choice(list(AMINO), size=n)) for n in lens])

    def cut(b, n):
        rec = seqs[b][int(rng.integers(0, 2))]
        at = int(rng.integers(0, len(rec) - n + 1))
        return rec[at:at + n]
    queries, planted, decoys = [], [], []  # planted / decoys: (query, bin, begin, end, with a stop) of a stretch, 0-based half-open nucleotides
    for q in range(CHIMERAS):
        a, b, c, d = (int(x) for x in rng.choice(BINS, size=4, replace=False))
        parts, at = [], 0

        def add(s, into=None, bin_=None, stop=False):
            nonlocal at
            parts.append(s)
            if into is not None:
                into.append((q, bin_, at, at + len(s), stop))
            at += len(s)
        stretch = lambda u: _edit(cut(u, W + S + 1 + int(rng.integers(0, 2 * S + 1))), int(rng.integers(0, EDITS + 1)), rng)
        add(_nt(rng, int(rng.integers(0, 3 * S))))
        add(_back(stretch(a), rng), planted, a)
        add(_nt(rng, 3 * (W // 2) + int(rng.integers(0, 3 * S))))
        add(T.reverse_complement(_back(stretch(b), rng)), planted, b)
        add(_nt(rng, 3 * (W // 2) + int(rng.integers(0, 3 * S))))
        # a stretch of bin c with one codon a stop, W / 4 residues from either end at least, and at most E - 1 further edits
        pep = _edit(cut(c, W + S + 1 + int(rng.integers(0, 2 * S + 1))), int(rng.integers(0, EDITS)), rng)
        stop_at = int(rng.integers(W // 4, len(pep) - W // 4))
        nt = _back(pep, rng)
        add(nt[:3 * stop_at] + ["TAA", "TAG", "TGA"][q % 3] + nt[3 * stop_at + 3:], planted, c, True)
        add(_nt(rng, 3 * (W // 2) + int(rng.integers(0, 3 * S))))
        # the decoy: W + 2 S residues of bin d, a block of E + 2 substitutions every W - S - (E + 2) residues from S / 2 on: every
        # window of W residues that lies in it holds a whole block, and so does every window that leaves it by up to E residues
        pep, block = cut(d, W + 2 * S), EDITS + 2
        for o in range(S // 2, len(pep) - block, W - S - block):
            pep = pep[:o] + _substituted(rng, pep[o:o + block]) + pep[o + block:]
        add(_back(pep, rng), decoys, d)
        add(_nt(rng, int(rng.integers(0, 3 * S))))
        s = "".join(parts)
        if q % 3 == 0:
            s = s.lower()
        if q % 3 == 1:
            s = s.replace("T", "U")
        queries.append(("chimera%d_b%d_b%d_b%d_d%d" % (q, a, b, c, d), s))
    short = []  # records whose frames have at most W residues: one window a frame, the whole frame
    for q in range(SHORT):
        b = int(rng.integers(0, BINS))
        n = W if q == 0 else int(rng.integers(W // 2 + k, W + 1))
        pep = _edit(cut(b, n), int(rng.integers(0, EDITS + 1)), rng)[:W]
        nt = _back(pep, rng)
        if q == 1:  # a stop in it: one edit is spent
            nt = _back(cut(b, n), rng)
            nt = nt[:3 * (n // 2)] + "TGA" + nt[3 * (n // 2) + 3:]
        if q == SHORT - 1:  # E + 2 substitutions: out of reach
            pep = cut(b, n)
            nt = _back(pep[:n // 2] + _substituted(rng, pep[n // 2:n // 2 + EDITS + 2]) + pep[n // 2 + EDITS + 2:], rng)
        short.append(("short%d_b%d" % (q, b), (nt if q % 2 else T.reverse_complement(nt)) + "AC"[:q % 3]))
    bins = [[("b%d_%d" % (b, i), r) for i, r in enumerate(recs)] for b, recs in enumerate(seqs)]
    distances, n_searched = R.window_distances(queries + short, k, W, S, EDITS, bins)
    return dict(name=name, seqs=seqs, bins=bins, queries=queries, short=short, planted=planted, decoys=decoys, distances=distances, n_searched=n_searched, k=k)


def exact_hits(case):
    """(query, frame, window, bin) with at least t of the window's stop-free k-mers, as plain letters, in the bin: a lower bound
    of the filter's hits whatever reduction, layout or Bloom filter the index uses"""
    k = case["k"]
    kmers = [set(r[i:i + k] for r in recs for i in range(len(r) - k + 1)) for recs in case["seqs"]]
    hits = set()
    for q, (_, s) in enumerate(case["queries"]):
        for f in range(6):
            residues = T.translate_frame(s, f)
            for j, (a, n) in enumerate(F.windows_of(len(residues), k, W, S)):
                mine = [residues[i:i + k] for i in range(a, a + n - k + 1) if "*" not in residues[i:i + k]]
                t = R.stop_threshold(len(mine), residues[a:a + n].count("*"), k, EDITS)
                for u in range(BINS):
                    if t != R.NOT_SEARCHED and sum(x in kmers[u] for x in mine) >= t:
                        hits.add((q, f, j, u))
    return hits


def check_case(case, rows, bin_name):
    """the conditions that keep the tests from passing on nothing, on any list of rows (the restatement's or the command's):
    every planted stretch — the one with a stop included — is covered by a row of its bin sharing at least W residues (3 W
    nucleotides) with it, and no row of a decoy's bin overlaps the decoy"""
    for q, b, begin, end, stop in case["planted"]:
        name = case["queries"][q][0]
        assert any(r[0] == name and r[1] == bin_name(b) and min(int(r[4]), end) - max(int(r[3]) - 1, begin) >= 3 * W for r in rows), (case["name"], q, b, stop)
    for q, b, begin, end, _ in case["decoys"]:
        name = case["queries"][q][0]
        assert not any(r[0] == name and r[1] == bin_name(b) and int(r[3]) - 1 < end and int(r[4]) > begin for r in rows), (case["name"], q, b)


def expected_rows(case, files, records=None, distances=None, w=W, s=S, **kw):
    want, n_confirmed = R.rows_of(records or case["queries"] + case["short"], case["k"], w, s, BINS, case["distances"] if distances is None else distances, **kw)
    return [(r[0], files[r[1]]) + tuple(str(x) for x in r[2:]) for r in want], n_confirmed


@pytest.fixture(scope="module")
def setups(tmp_path_factory):
    root = tmp_path_factory.mktemp("verify_frame_windows_cli")
    out = {}
    for name, (k, flags, red) in ALPHABETS.items():
        case = generate(name)
        d = root / name
        d.mkdir()
        files = []
        for b, recs in enumerate(case["bins"]):
            text = "".join(">%s description\n%s\n" % (n, r) for n, r in recs)
            p = d / ("bin%02d.fa" % b + (".gz" if b % 3 == 0 else ""))
            if b % 3 == 0:
                with gzip.open(p, "wt") as f:
                    f.write(text)
            else:
                p.write_text(text)
            files.append(os.path.abspath(str(p)))
        qf = d / "queries.fa"
        qf.write_text("".join(">%s some comment\n%s\n" % (n, s) for n, s in case["queries"] + case["short"]))
        indexes = {}
        for lay, lflags in LAYOUTS.items():
            rc, so, se = _run("index", "-k", str(k), *flags, *lflags, str(d / lay), *files)
            assert rc == 0 and os.path.exists(d / (lay + ".ibf")), se
            indexes[lay] = str(d / (lay + ".ibf"))
        want, n_confirmed = expected_rows(case, files)
        # the restatement alone meets the conditions, the stretches with a stop are there, and the filter must let through at
        # least 5 windows of the chimeras that verification rejects
        check_case(case, want, lambda b: files[b])
        assert sum(1 for p in case["planted"] if p[4]) == CHIMERAS
        assert len(exact_hits(case) - set(case["distances"])) >= 5, name
        out[name] = dict(case=case, files=files, qfile=str(qf), indexes=indexes, want=want, n_confirmed=n_confirmed, k=k, red=red, dir=d,
                         flags=("--translate", "--frame-window", str(W), "--frame-step", str(S), "-e", str(EDITS)))
    return out


def _rows(stdout):
    return [tuple(line.split("\t")) for line in stdout.splitlines()]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("alphabet", list(ALPHABETS))
def test_rows_match_the_reference(setups, alphabet, layout):
    s = setups[alphabet]
    rc, so, se = _run("search", *s["flags"], "--verify-frame-windows", "-v", s["indexes"][layout], s["qfile"], env={"TETREX_TRACE": "1"})
    assert rc == 0, se
    got = _rows(so)
    assert got == s["want"], (alphabet, layout, [x for x in got if x not in s["want"]][:3], [x for x in s["want"] if x not in got][:3])
    m = re.search(r"Verified: (\d+) of (\d+) candidate windows", se)
    assert m and int(m.group(1)) == s["n_confirmed"], se
    assert int(m.group(2)) - int(m.group(1)) >= 5, "the filter passes what verification rejects"
    w = re.search(r"Windows: (\d+) searched, (\d+) hit, (\d+) rows", se)
    assert w and int(w.group(1)) == s["case"]["n_searched"] and int(w.group(3)) == len(got), se
    routes = re.search(r"verify routes: device (\d+), device-long (\d+), host (\d+), windows (\d+)", se)
    assert routes and [int(x) for x in routes.groups()] == [0, 0, 0, int(m.group(2))], se
    check_case(s["case"], got, lambda b: s["files"][b])
    assert {r[2][0] for r in got} == {"+", "-"}


def _restatement(oracle, path):
    """search(values, offsets, thresholds) -> (hits, counts) of the index file"""
    from tetrex_amd import host
    ix = host.IndexFile.load(path)
    d = ix.describe()
    if d["is_hibf"]:
        descs = []
        for i, f in enumerate(d["ibfs"]):
            nxt, tbu = ix.maps(i)
            descs.append(dict(bins=f["bins"], bin_size=f["bin_size"], hash_funs=f["hash_funs"], words=ix.words(i), next_ibf_id=nxt, tb_to_user=tbu))
        return TreeRef(oracle, d["bins"], descs).search
    f = d["ibfs"][0]
    ox = oracle_ibf_from_words(oracle, f["bins"], f["bin_size"], f["hash_funs"], ix.words(0))
    return lambda v, o, t: flat_search(ox, f["bins"], v, o, t)


@pytest.mark.parametrize("alphabet", list(ALPHABETS))
def test_counts_column_against_the_oracle(oracle, setups, alphabet):
    """with --counts the rows are those of the candidates the index really gives — the oracle restatement of the index file
    counts every searched window's values — confirmed by the restatement's distances: exact equality, count/w included"""
    s = setups[alphabet]
    k, red, case = s["k"], s["red"], s["case"]
    search = _restatement(oracle, s["indexes"]["default"])
    records = case["queries"] + case["short"]
    owner, qs, thr = [], [], []
    for r, (_, seq) in enumerate(records):
        for f in range(6):
            values, residues = T.frame_values(seq, f, k, red), T.translate_frame(seq, f)
            for j, ((a, n), (b, w)) in enumerate(zip(F.windows_of(len(residues), k, W, S), F.window_ranges(seq, f, k, W, S))):
                t = R.stop_threshold(w, residues[a:a + n].count("*"), k, EDITS)
                if t != R.NOT_SEARCHED:
                    owner.append((r, f, j))
                    qs.append(values[b:b + w])
                    thr.append(t)
    assert len(owner) == case["n_searched"]
    v, off = csr(qs)
    _, counts = search(v, off, np.array(thr, dtype=np.uint32))
    hit_counts = {(r, f, j, u): int(counts[i, u]) for i, (r, f, j) in enumerate(owner) for u in range(BINS) if counts[i, u] >= thr[i]}
    assert set(case["distances"]) <= set(hit_counts), "the filter dropped a window within E edits"
    want, n_confirmed = expected_rows(case, s["files"], hit_counts=hit_counts, with_counts=True)
    assert [r[:5] + r[6:] for r in want] == s["want"] and n_confirmed == s["n_confirmed"]
    rc, so, se = _run("search", *s["flags"], "--verify-frame-windows", "--counts", "-v", s["indexes"]["default"], s["qfile"])
    assert rc == 0, se
    assert _rows(so) == want
    m = re.search(r"Verified: (\d+) of (\d+) candidate windows", se)
    assert m and int(m.group(2)) == len(hit_counts), se


@pytest.mark.parametrize("alphabet", list(ALPHABETS))
def test_routes_thresholds_and_batches_give_the_same_output(setups, alphabet):
    s = setups[alphabet]
    args = ("search", *s["flags"], "--verify-frame-windows", "--counts", "-v", s["indexes"]["flat"], s["qfile"])
    rc, base, se = _run(*args)
    assert rc == 0 and base, se
    candidates = int(re.search(r"of (\d+) candidate windows", se).group(1))
    rc, so, se = _run(*args, env={"TETREX_VERIFY_FRAME_WINDOWS": "written", "TETREX_TRACE": "1"})
    assert rc == 0 and so == base, se
    assert re.search(r"verify routes: device [1-9]\d*, device-long 0, host 0, windows 0", se), se
    # §18's threshold: windows with more than E stops are searched too, more candidates, the same rows
    rc, so, se = _run(*args, env={"TETREX_FRAME_WINDOW_THRESHOLD": "plain"})
    assert rc == 0 and so == base, se
    plain = re.search(r"Windows: (\d+) searched", se), re.search(r"of (\d+) candidate windows", se)
    assert int(plain[0].group(1)) > s["case"]["n_searched"] and int(plain[1].group(1)) >= candidates, se
    rc, so, se = _run(*args, env={"TETREX_SEARCH_BATCH_WINDOWS": "7"})
    assert rc == 0 and so == base, se
    rc, so, se = _run(*args, env={"TXQ_EDIT_WINDOWS_BUNDLE": "4"})
    assert rc == 0 and so == base, se


def test_the_variable_is_inert_without_the_flag(setups):
    s = setups["peptide"]
    args = ("search", *s["flags"], "--counts", s["indexes"]["default"], s["qfile"])
    rc, base, se = _run(*args)
    assert rc == 0 and base, se
    rc, so, se2 = _run(*args, env={"TETREX_FRAME_WINDOW_THRESHOLD": "plain", "TETREX_VERIFY_FRAME_WINDOWS": "written"})
    assert rc == 0 and so == base and se2 == se
    assert all(len(r) == 6 for r in _rows(base))


def test_a_window_above_512_residues_is_written_out(setups):
    """W = 520: every window takes --verify's long-pattern route through the host-translated frames, with the restatement's rows"""
    s = setups["peptide"]
    case = s["case"]
    rng = np.random.default_rng(5)
    src = case["seqs"][5][1]
    body = _edit(src[300:1100], 2, rng)
    records = [("long_b5", _nt(rng, 250) + _back(body, rng)), ("long_rc_b5", T.reverse_complement(_back(body[:600], rng)) + "G")]
    qf = os.path.join(os.path.dirname(s["qfile"]), "long.fa")
    with open(qf, "w") as f:
        f.write("".join(">%s\n%s\n" % r for r in records))
    w, step = 520, 100
    distances, n_searched = R.window_distances(records, case["k"], w, step, EDITS, case["bins"])
    want, n_confirmed = expected_rows(case, s["files"], records=records, distances=distances, w=w, s=step)
    assert n_confirmed >= 3 and {r[2][0] for r in want} == {"+", "-"}
    rc, so, se = _run("search", "--translate", "--frame-window", str(w), "--frame-step", str(step), "-e", str(EDITS), "--verify-frame-windows", "-v",
                      s["indexes"]["default"], qf, env={"TETREX_TRACE": "1"})
    assert rc == 0, se
    assert _rows(so) == want
    m = re.search(r"Windows: (\d+) searched", se)
    assert m and int(m.group(1)) == n_searched, se
    routes = re.search(r"verify routes: device (\d+), device-long (\d+), host (\d+), windows (\d+)", se)
    assert routes and int(routes.group(2)) >= n_confirmed and int(routes.group(4)) == 0 and int(routes.group(1)) == 0, se


def test_a_nucleotide_index_is_refused(setups, tmp_path):
    s = setups["peptide"]
    rng = np.random.default_rng(1)
    files = []
    for b in range(2):
        p = tmp_path / ("nt%d.fa" % b)
        p.write_text(">n%d\n%s\n" % (b, _nt(rng, 400)))
        files.append(str(p))
    rc, so, se = _run("index", "-n", "-k", "16", "-i", str(tmp_path / "nt"), *files)
    assert rc == 0, se
    dest = tmp_path / "out.tsv"
    rc, so, se = _run("search", *s["flags"], "--verify-frame-windows", "-o", str(dest), str(tmp_path / "nt.ibf"), s["qfile"])
    assert rc != 0 and "--translate needs a peptide index" in se and so == "" and not dest.exists()
