"""`tetrex search --verify --align` and `--translate --verify-frames --align` on tiny libraries that `tetrex index`
builds from generated FASTA: five bins of two records of tens to a few hundred letters, one bin with a record of 4600; queries
of 60 letters, one of 700 (the long-pattern kernel) and one of 4200 (the host route), cut from the bins and given up to three
edits.  Every row's start and cigar are checked against the full matrix of tests/edit_align_ref.py on the letters the row
names; the rows with TETREX_VERIFY_ALIGN=host are the same bytes; without --align the rows are the prefix of the rows with it."""
import os
import re
import subprocess

import numpy as np
import pytest

import edit_align_ref as A
import edit_cases
import edit_ref as E
import translate_ref as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TETREX = os.path.join(ROOT, "bin", "tetrex")
AMINO = "ACDEFGHIKLMNPQRSTVWY"
LIBRARIES = {"peptide": (AMINO, 6, [], False), "dna": ("ACGT", 16, ["-n"], True)}  # name: (letters, k, index flags, dna)
CODES = {"peptide": E.letter_codes("ABCDEFGHIJKLMNOPQRSTUVWXYZ"), "dna": E.letter_codes("ACGT", {"U": 3})}
EDITS, BINS = 3, 5
CODONS_OF = {}
for _codon, _aa in T.CODON.items():
    CODONS_OF.setdefault(_aa, []).append(_codon)


def _run(*args, env=None):
    r = subprocess.run([TETREX, *args], capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    return r.returncode, r.stdout, r.stderr


def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _library(root, name, letters, k, flags, seed):
    """bins, their index, and `pieces(n, e)`: a cut of n letters from a bin with e edits"""
    rng = np.random.default_rng(seed)
    seqs = [["".join(rng.choice(list(letters), size=int(n))) for n in rng.integers(40, 300, size=2)] for _ in range(BINS)]
    seqs[2][1] = "".join(rng.choice(list(letters), size=4600))
    d = root / name
    d.mkdir()
    files = []
    for b, recs in enumerate(seqs):
        p = d / ("bin%02d.fa" % b)
        p.write_text("".join(">b%d_%d description\n%s\n" % (b, i, r) for i, r in enumerate(recs)))
        files.append(os.path.abspath(str(p)))
    rc, so, se = _run("index", "-k", str(k), *flags, "-i", str(d / "flat"), *files)
    assert rc == 0 and os.path.exists(d / "flat.ibf"), se

    def piece(n, e):
        b = 2 if n > 250 else int(rng.integers(0, BINS))
        rec = 1 if n > 250 else int(np.argmax([len(r) for r in seqs[b]]))
        n = min(n, len(seqs[b][rec]))
        at = int(rng.integers(0, len(seqs[b][rec]) - n + 1))
        cut = np.frombuffer(seqs[b][rec][at:at + n].encode(), dtype=np.uint8)
        return edit_cases.edited(rng, letters, cut, e).tobytes().decode().upper()

    records = {"b%d_%d" % (b, i): r for b, recs in enumerate(seqs) for i, r in enumerate(recs)}
    return dict(index=str(d / "flat.ibf"), files=files, records=records, piece=piece, rng=rng, dir=d)


@pytest.fixture(scope="module")
def libraries(tmp_path_factory):
    root = tmp_path_factory.mktemp("search_align_cli")
    out = {}
    for name, (letters, k, flags, dna) in LIBRARIES.items():
        lib = _library(root, name, letters, k, flags, seed=400 + len(name))
        queries = {}
        for i, (n, e) in enumerate([(60, 0), (60, 1), (60, 2), (60, 3), (60, 3), (48, 1), (700, 3), (4200, 1)]):
            s = lib["piece"](n, e)
            queries["q%d_%d" % (n, i)] = _revcomp(s) if dna and i % 2 else s
        qf = lib["dir"] / "queries.fa"
        qf.write_text("".join(">%s some comment\n%s\n" % (n, s) for n, s in queries.items()))
        out[name] = dict(lib, queries=queries, qfile=str(qf), dna=dna)
    # nucleotide reads for --translate on the peptide library: the coding strand of a cut, every other one reverse-complemented
    lib = out["peptide"]
    rng, reads = lib["rng"], {}
    for i, (n, e) in enumerate([(50, 0), (50, 1), (50, 3), (50, 2), (700, 2)]):
        nt = "ACGT"[i % 4] * (i % 3) + "".join(CODONS_OF[a][int(rng.integers(0, len(CODONS_OF[a])))] for a in lib["piece"](n, e))
        reads["r%d_%d" % (n, i)] = _revcomp(nt) if i % 2 else nt
    rf = lib["dir"] / "reads.fa"
    rf.write_text("".join(">%s\n%s\n" % (n, s) for n, s in reads.items()))
    out["translated"] = dict(lib, queries=reads, qfile=str(rf), dna=False)
    return out


def _check_rows(stdout, letters_of, records, codes, columns, at):
    """every row (distance, target, end in columns at .. at + 2, start and cigar last): distance, start and cigar against the
    yardstick on the letters the row names; returns the rows and the operations seen"""
    rows = [line.split("\t") for line in stdout.splitlines()]
    ops = set()
    for row in rows:
        assert len(row) == columns, row
        distance, target, end = int(row[at]), row[at + 1], int(row[at + 2])
        d, j, start, runs = A.align(letters_of(row), records[target], codes, j=end)
        assert (d, start + 1, A.cigar(runs)) == (distance, int(row[-2]), row[-1]), (row, d, start, A.cigar(runs))
        A.check_identities(len(letters_of(row)), d, j, start, runs)
        ops.update(c for c, _ in runs)
    return rows, ops


def _align_routes(stderr):
    m = re.search(r"align routes: device (\d+), host (\d+)", stderr)
    assert m, stderr
    return int(m.group(1)), int(m.group(2))


@pytest.mark.parametrize("library", list(LIBRARIES))
def test_cli_verify_align(libraries, library):
    lib = libraries[library]
    dna = lib["dna"]
    args = ("search", "-e", str(EDITS), "--verify", lib["index"], lib["qfile"])
    rc, plain, se = _run(*args)
    assert rc == 0 and "align routes" not in se, se
    rc, so, se = _run(*args, "--align", env={"TETREX_TRACE": "1"})
    assert rc == 0, se

    def letters_of(row):
        s = lib["queries"][row[0]]
        return _revcomp(s) if dna and row[5] == "-" else s

    rows, ops = _check_rows(so, letters_of, lib["records"], CODES[library], 8 if dna else 7, 2)
    # every query is confirmed in the bin it was cut from; the query of 4200 letters is aligned on the host, the others on the device
    assert {r[0] for r in rows} == set(lib["queries"]) and ops >= set("=X") and ops & set("ID")
    assert _align_routes(se) == (len(rows) - 1, 1)
    if dna:
        assert {r[5] for r in rows} == {"+", "-"}
    # without --align: the same rows, less the two columns
    assert plain.splitlines() == ["\t".join(r[:-2]) for r in rows]
    # the host twin for every pair: the same bytes
    rc, so_host, se = _run(*args, "--align", env={"TETREX_TRACE": "1", "TETREX_VERIFY_ALIGN": "host"})
    assert rc == 0 and so_host == so, se
    assert _align_routes(se) == (0, len(rows))
    # the long-pattern kernel off: the query of 700 letters is searched on the host and aligned there too
    rc, so_short, se = _run(*args, "--align", env={"TETREX_TRACE": "1", "TETREX_VERIFY_LONG": "0"})
    assert rc == 0 and so_short == so, se
    assert _align_routes(se) == (len(rows) - 2, 2)


def test_cli_verify_frames_align(libraries):
    lib = libraries["translated"]
    args = ("search", "--translate", "-e", str(EDITS), "--verify-frames", lib["index"], lib["qfile"])
    rc, plain, se = _run(*args)
    assert rc == 0, se
    rc, so, se = _run(*args, "--align", env={"TETREX_TRACE": "1"})
    assert rc == 0, se
    rows, ops = _check_rows(so, lambda row: T.translate_frame(lib["queries"][row[0]], T.FRAMES.index(row[2])), lib["records"], CODES["peptide"], 8, 3)
    assert {r[0] for r in rows} == set(lib["queries"]) and {r[2][0] for r in rows} == {"+", "-"}
    assert _align_routes(se) == (len(rows), 0)
    assert plain.splitlines() == ["\t".join(r[:-2]) for r in rows]
    rc, so_host, se = _run(*args, "--align", env={"TETREX_TRACE": "1", "TETREX_VERIFY_ALIGN": "host"})
    assert rc == 0 and so_host == so and _align_routes(se) == (0, len(rows)), se


def test_align_alone_is_refused(libraries):
    lib = libraries["peptide"]
    for args in (("search", "-e", "1", "--align"), ("search", "--translate", "-e", "1", "--align"), ("search", "--threshold", "0.5", "--align")):
        rc, so, se = _run(*args, lib["index"], lib["qfile"])
        assert rc == 1 and so == "" and "[Search Parser Error] --align" in se and "--verify" in se, (args, se)
