"""`tetrex search --window W [--step S] -e E --verify-windows` on indexes that `tetrex index` builds from generated
FASTA, against the Python restatement tests/verify_windows_ref.py: the window layout of tests/search_window_ref.py, the
distances of tests/edit_ref.py and the run merge.  The queries are chimeric records — a stretch of one bin with 0..E edits,
random letters, a stretch of another bin (on DNA reverse-complemented for half of them), random letters, and a decoy: a
stretch of a third bin with blocks of E + 2 adjacent substitutions so close that every window in it holds one, which the
k-mer filter lets through and verification must reject."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import edit_cases
import edit_ref as E
import verify_windows_ref as R
from search_window_ref import windows_of, threshold_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TETREX = os.path.join(ROOT, "bin", "tetrex")
AMINO = "ACDEFGHIKLMNPQRSTVWY"
ALPHABETS = {  # name: (residues, k, index flags, dna, W, S)
    "peptide": (AMINO, 6, [], False, 60, 15),
    "murphy": (AMINO, 5, ["-r", "murphy"], False, 60, 15),
    "dna": ("ACGT", 16, ["-n"], True, 150, 50),
}
LAYOUTS = {"flat": ["-i"], "default": [], "sized": ["--layout", "sized"]}
EDITS, BINS, CHIMERAS, SHORT = 2, 24, 6, 5
SEEDS = {"peptide": 407, "murphy": 406, "dna": 403}  # (settled on the CPU: generate() with the reference alone meets check_case())


def _run(*args, env=None):
    r = subprocess.run([TETREX, *args], capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    return r.returncode, r.stdout, r.stderr


def _substituted(rng, res, s):
    return "".join(res[(res.index(c) + 1 + int(rng.integers(0, len(res) - 1))) % len(res)] for c in s)


def generate(name):
    """the bins (two records each; bin 5's second one is long), the chimeric queries with where their stretches lie, the short
    queries, and the reference distances of every searched window of every query to every bin"""
    res, k, _, dna, W, S = ALPHABETS[name]
    rng = np.random.default_rng(SEEDS[name])
    seqs = []
    for b in range(BINS):
        lens = [int(rng.integers(150, 400)) * (3 if dna else 1) for _ in range(2)]
        if b == 5:
            lens[1] = 2200
        seqs.append(["".join(rng.choice(list(res), size=n)) for n in lens])
    rand = lambda n: "".join(rng.choice(list(res), size=n))
    cut = lambda b, n: (lambda rec: (lambda at: rec[at:at + n])(int(rng.integers(0, len(rec) - n))))(seqs[b][int(rng.integers(0, 2))])
    edited = lambda s, e: edit_cases.edited(rng, res, np.frombuffer(s.encode(), dtype=np.uint8), e).tobytes().decode().upper()
    queries, planted, decoys = [], [], []  # planted / decoys: (query, bin, begin, end) of a stretch, 0-based half-open
    for q in range(CHIMERAS):
        a, b, d = (int(x) for x in rng.choice(BINS, size=3, replace=False))
        parts, at = [], 0

        def add(s, into=None, bin_=None):
            nonlocal at
            parts.append(s)
            if into is not None:
                into.append((q, bin_, at, at + len(s)))
            at += len(s)
        add(rand(int(rng.integers(0, S))))
        add(edited(cut(a, W + S + 1 + int(rng.integers(0, 2 * S))), int(rng.integers(0, EDITS + 1))), planted, a)
        add(rand(W // 2 + int(rng.integers(0, S))))
        s = edited(cut(b, W + S + 1 + int(rng.integers(0, 2 * S))), int(rng.integers(0, EDITS + 1)))
        add(R.revcomp(s) if dna and q % 2 else s, planted, b)
        add(rand(W // 2 + int(rng.integers(0, S))))
        # the decoy: W + 2 S letters of bin d, a block of E + 2 substitutions every W - S - (E + 2) letters from S / 2 on:
        # every window of W letters that lies in it holds a whole block, and so does every window that leaves it by up to E letters
        s, block = cut(d, W + 2 * S), EDITS + 2
        for o in range(S // 2, len(s) - block, W - S - block):
            s = s[:o] + _substituted(rng, res, s[o:o + block]) + s[o + block:]
        add(s, decoys, d)
        add(rand(int(rng.integers(0, S))))
        s = "".join(parts)
        if dna and q % 3 == 0:
            s = s.lower()
        if dna and q % 3 == 1:
            s = s.replace("T", "U")
        queries.append(("chimera%d_b%d_b%d_d%d" % (q, a, b, d), s))
    short = []  # records of at most W letters: one window each, the whole record
    for q in range(SHORT):
        b = int(rng.integers(0, BINS))
        n = W if q == 0 else int(rng.integers(W // 2 + k, W + 1))
        s = cut(b, n)
        s = edited(s, int(rng.integers(0, EDITS + 1)))[:W] if q < SHORT - 1 else s[:n // 2] + _substituted(rng, res, s[n // 2:n // 2 + EDITS + 2]) + s[n // 2 + EDITS + 2:]
        short.append(("short%d_b%d" % (q, b), R.revcomp(s) if dna and q % 2 else s))
    codes = E.letter_codes("ACGT", {"U": 3}) if dna else E.letter_codes("ABCDEFGHIJKLMNOPQRSTUVWXYZ")
    bins = [[("b%d_%d" % (b, i), r) for i, r in enumerate(recs)] for b, recs in enumerate(seqs)]
    distances, n_searched = R.window_distances(queries + short, k, W, S, EDITS, bins, codes, dna)
    return dict(name=name, seqs=seqs, bins=bins, codes=codes, queries=queries, short=short, planted=planted, decoys=decoys, distances=distances,
                n_searched=n_searched, dna=dna, k=k, W=W, S=S)


def exact_hits(case):
    """(query, window, bin) with at least t of the window's k-mers, as plain letters on the given strand, in the bin: a lower
    bound of the filter's hits whatever reduction, canonical form or Bloom filter the index uses"""
    k, W, S = case["k"], case["W"], case["S"]
    kmers = [set(r[i:i + k] for r in recs for i in range(len(r) - k + 1)) for recs in case["seqs"]]
    hits = set()
    for q, (_, s) in enumerate(case["queries"]):
        s = s.upper().replace("U", "T")
        for j, (b, n) in enumerate(windows_of(len(s), k, W, S)):
            t = threshold_of(n - k + 1, k, EDITS)
            for u in range(BINS):
                if t and sum(s[i:i + k] in kmers[u] for i in range(b, b + n - k + 1)) >= t:
                    hits.add((q, j, u))
    return hits


def covered(rows, name, bin_path, begin, end, W):
    """does a row of (name, bin) share at least W letters with the 0-based stretch [begin, end)?"""
    return any(r[0] == name and r[1] == bin_path and min(int(r[3]), end) - max(int(r[2]) - 1, begin) >= W for r in rows)


def check_case(case, rows, bin_name):
    """the conditions that keep the tests from passing on nothing, on any list of rows (the reference's or the command's)"""
    W = case["W"]
    for q, b, begin, end in case["planted"]:
        assert end - begin >= W + case["S"] - 1 and covered(rows, case["queries"][q][0], bin_name(b), begin, end, W), (case["name"], q, b)
    for q, b, begin, end in case["decoys"]:
        assert not any(r[0] == case["queries"][q][0] and r[1] == bin_name(b) and int(r[2]) - 1 < end and int(r[3]) > begin for r in rows), (case["name"], q, b)


@pytest.fixture(scope="module")
def setups(tmp_path_factory):
    root = tmp_path_factory.mktemp("verify_windows_cli")
    out = {}
    for name, (res, k, flags, dna, W, S) in ALPHABETS.items():
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
        qf, sf = d / "queries.fa", d / "short.fa"
        qf.write_text("".join(">%s some comment\n%s\n" % (n, s) for n, s in case["queries"] + case["short"]))
        sf.write_text("".join(">%s some comment\n%s\n" % (n, s) for n, s in case["short"]))
        indexes = {}
        for lay, lflags in LAYOUTS.items():
            rc, so, se = _run("index", "-k", str(k), *flags, *lflags, str(d / lay), *files)
            assert rc == 0 and os.path.exists(d / (lay + ".ibf")), se
            indexes[lay] = str(d / (lay + ".ibf"))
        want, n_confirmed = R.rows_of(case["queries"] + case["short"], k, W, S, BINS, case["distances"])
        want = [(r[0], files[r[1]]) + tuple(str(x) for x in r[2:]) for r in want]
        # the reference alone meets the conditions, and the filter must let through at least 5 windows that it rejects
        check_case(case, want, lambda b: files[b])
        n_chimera = sum(1 for (r, j, u) in case["distances"] if r < CHIMERAS)
        assert len(exact_hits(case) - {key for key in case["distances"]}) >= 5 and n_chimera >= 2 * CHIMERAS, name
        out[name] = dict(case=case, files=files, qfile=str(qf), sfile=str(sf), indexes=indexes, want=want, n_confirmed=n_confirmed,
                         flags=("--window", str(W), "--step", str(S), "-e", str(EDITS)))
    return out


def _rows(stdout):
    return [tuple(line.split("\t")) for line in stdout.splitlines()]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("alphabet", list(ALPHABETS))
def test_rows_match_the_reference(setups, alphabet, layout):
    s = setups[alphabet]
    rc, so, se = _run("search", *s["flags"], "--verify-windows", "-v", s["indexes"][layout], s["qfile"], env={"TETREX_TRACE": "1"})
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
    if s["case"]["dna"]:
        assert {r[-1] for r in got} == {"+", "-"}


@pytest.mark.parametrize("alphabet", list(ALPHABETS))
def test_counts_column(setups, alphabet):
    s = setups[alphabet]
    k = s["case"]["k"]
    rc, so, se = _run("search", *s["flags"], "--verify-windows", "--counts", s["indexes"]["default"], s["qfile"])
    assert rc == 0, se
    got = _rows(so)
    assert [r[:4] + r[5:] for r in got] == s["want"]
    for r in got:
        count, w = (int(x) for x in r[4].split("/"))
        assert threshold_of(w, k, EDITS) <= count <= w and w <= s["case"]["W"] - k + 1, r


@pytest.mark.parametrize("alphabet", list(ALPHABETS))
def test_routes_and_batches_give_the_same_output(setups, alphabet):
    s = setups[alphabet]
    args = ("search", *s["flags"], "--verify-windows", "--counts", s["indexes"]["flat"], s["qfile"])
    rc, base, se = _run(*args)
    assert rc == 0 and base, se
    rc, so, se = _run(*args, env={"TETREX_VERIFY_WINDOWS": "written", "TETREX_TRACE": "1"})
    assert rc == 0 and so == base, se
    assert re.search(r"verify routes: device [1-9]\d*, device-long 0, host 0, windows 0", se), se
    rc, so, se = _run(*args, env={"TETREX_SEARCH_BATCH_WINDOWS": "7", "TXQ_EDIT_WINDOWS_BUNDLE": "2"})
    assert rc == 0 and so == base, se


@pytest.mark.parametrize("alphabet", list(ALPHABETS))
def test_short_records_are_what_verify_gives(setups, alphabet):
    """a record of at most W letters is one window, the whole record: its rows are those of -e E --verify with 1 and L inserted"""
    s = setups[alphabet]
    rc, so, se = _run("search", "-e", str(EDITS), "--verify", s["indexes"]["default"], s["sfile"])
    assert rc == 0, se
    length = dict((n, len(letters)) for n, letters in s["case"]["short"])
    want = [r[:2] + ("1", str(length[r[0]])) + r[2:] for r in _rows(so)]
    rc, so, se = _run("search", *s["flags"], "--verify-windows", s["indexes"]["default"], s["sfile"])
    assert rc == 0, se
    assert _rows(so) == want and len(want) >= SHORT - 1
    assert want == [r for r in s["want"] if r[0] in length]


def test_a_window_above_512_letters_is_written_out(setups):
    """W = 600 on the nucleotide index: every window takes --verify's long-pattern route, with the same rows as the reference"""
    s = setups["dna"]
    case = s["case"]
    rng = np.random.default_rng(5)
    src = case["seqs"][5][1]
    body = edit_cases.edited(rng, "ACGT", np.frombuffer(src[300:1700].encode(), dtype=np.uint8), 3).tobytes().decode().upper()
    records = [("long_b5", "".join(rng.choice(list("ACGT"), size=250)) + body), ("long_rc_b5", R.revcomp(body[:900]))]
    qf = os.path.join(os.path.dirname(s["qfile"]), "long.fa")
    with open(qf, "w") as f:
        f.write("".join(">%s\n%s\n" % r for r in records))
    W, S = 600, 200
    distances, _ = R.window_distances(records, case["k"], W, S, EDITS, case["bins"], case["codes"], True)
    want, n_confirmed = R.rows_of(records, case["k"], W, S, BINS, distances)
    want = [(r[0], s["files"][r[1]]) + tuple(str(x) for x in r[2:]) for r in want]
    assert n_confirmed >= 3 and {r[-1] for r in want} == {"+", "-"}
    rc, so, se = _run("search", "--window", str(W), "--step", str(S), "-e", str(EDITS), "--verify-windows", "-v", s["indexes"]["default"], qf, env={"TETREX_TRACE": "1"})
    assert rc == 0, se
    assert _rows(so) == want
    routes = re.search(r"verify routes: device (\d+), device-long (\d+), host (\d+), windows (\d+)", se)
    assert routes and int(routes.group(2)) >= n_confirmed and int(routes.group(4)) == 0 and int(routes.group(1)) == 0, se
