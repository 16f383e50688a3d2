"""`tetrex search ... --verify-windows --align-windows` and `... --verify-frame-windows --align-windows` on small
libraries of 24 bins that `tetrex index` builds from generated FASTA: a peptide library under a flat index and under the default
HIBF, a nucleotide library with hits on both strands, and nucleotide contigs on the peptide library.  Every row is checked
against the Python restatements — the window layouts of tests/search_window_ref.py and tests/frame_window_ref.py, the distances
of tests/verify_windows_ref.py and tests/verify_frame_windows_ref.py, the full alignment matrix of tests/edit_align_ref.py:
  (a) without its last four columns it is, byte for byte, the row of the same command without the flag;
  (b) [wbegin, wend] is a searched window inside [begin, end] whose distance is the row's and the least of the run, the earliest
      on a tie;
  (c) that window, cut, reverse-complemented or translated as documented, aligns to the named target at j = target_end with the
      row's start and cigar;
and the routes — the device call, the host twin, the written-out windows, several rounds of resident bins, small device
batches, a window above 512 letters, a window 32 edits away — give the same bytes."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import edit_align_ref as A
import edit_cases
import edit_ref as E
import frame_window_ref as F
import translate_ref as T
import verify_frame_windows_ref as RF
import verify_windows_ref as R
from search_window_ref import windows_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TETREX = os.path.join(ROOT, "bin", "tetrex")
AMINO = "ACDEFGHIKLMNPQRSTVWY"
BINS, CHIMERAS, EDITS = 24, 4, 2
PEPTIDE_CODES, DNA_CODES = RF.PEPTIDE_CODES, E.letter_codes("ACGT", {"U": 3})
CODONS_OF = {}
for _codon, _aa in T.CODON.items():
    CODONS_OF.setdefault(_aa, []).append(_codon)
# name: (library, index flags, mode, k, W, S)
SCENARIOS = {
    "peptide_flat": ("peptide", ["-i"], "windows", 6, 60, 15),
    "peptide_hibf": ("peptide", [], "windows", 6, 60, 15),
    "dna_hibf": ("dna", ["-n"], "windows", 16, 150, 50),
    "contigs_hibf": ("peptide", [], "frames", 6, 40, 10),
}
ROUTES = {  # environment of a run that must write the bytes of the default run
    "host": {"TETREX_VERIFY_ALIGN": "host"},
    "written": {"TETREX_VERIFY_WINDOWS": "written", "TETREX_VERIFY_FRAME_WINDOWS": "written"},
    "rounds": {"TETREX_VERIFY_TEXT_MB": "0.004"},  # about 4 KiB of resident text: a few bins a round, the long bin alone
    "batches": {"TETREX_SEARCH_BATCH_WINDOWS": "7"},
}


def _run(*args, env=None):
    r = subprocess.run([TETREX, *args], capture_output=True, text=True, timeout=600, env=dict(os.environ, TETREX_TRACE="1", **(env or {})))
    return r.returncode, r.stdout, r.stderr


def _library(kind, rng):
    """24 bins of two records; bin 5's second one is long"""
    res = "ACGT" if kind == "dna" else AMINO
    seqs = []
    for b in range(BINS):
        lens = [int(rng.integers(150, 400)) * (3 if kind == "dna" else 1) for _ in range(2)]
        if b == 5:
            lens[1] = 2200
        seqs.append(["".join(rng.choice(list(res), size=n)) for n in lens])
    return seqs


def _chimeras(kind, mode, seqs, W, S, rng):
    """records with stretches of two or three bins, 0 .. E edits each, between random letters: as letters of the library, on a
    nucleotide library every other second stretch reverse-complemented, or back-translated (the second stretch on the reverse
    strand) for the translated search"""
    res = "ACGT" if kind == "dna" else AMINO
    rand = lambda n: "".join(rng.choice(list(res if mode == "windows" else "ACGT"), size=n))
    back = lambda pep: "".join(CODONS_OF[a][int(rng.integers(0, len(CODONS_OF[a])))] for a in pep)
    unit = 3 if mode == "frames" else 1

    def stretch(b):
        rec = seqs[b][int(rng.integers(0, 2))]
        n = W + 2 * S + 1 + int(rng.integers(0, 2 * S))
        at = int(rng.integers(0, len(rec) - n))
        s = edit_cases.edited(rng, res, np.frombuffer(rec[at:at + n].encode(), dtype=np.uint8), int(rng.integers(0, EDITS + 1))).tobytes().decode().upper()
        return back(s) if mode == "frames" else s
    queries = []
    for q in range(CHIMERAS):
        a, b, c = (int(x) for x in rng.choice(BINS, size=3, replace=False))
        second = stretch(b)
        if mode == "frames":
            second = T.reverse_complement(second)
        elif kind == "dna" and q % 2:
            second = R.revcomp(second)
        s = rand(int(rng.integers(0, unit * S))) + stretch(a) + rand(unit * (W // 2) + int(rng.integers(0, unit * S))) + second + \
            rand(unit * (W // 2) + int(rng.integers(0, 3))) + stretch(c) + rand(int(rng.integers(0, unit * S)))
        queries.append(("chimera%d_b%d_b%d_b%d" % (q, a, b, c), s))
    return queries


def _write_bins(d, seqs):
    files, bins = [], [[("b%d_%d" % (b, i), r) for i, r in enumerate(recs)] for b, recs in enumerate(seqs)]
    for b, recs in enumerate(bins):
        text = "".join(">%s description\n%s\n" % (n, r) for n, r in recs)
        p = d / ("bin%02d.fa" % b + (".gz" if b % 3 == 0 else ""))
        if b % 3 == 0:
            with gzip.open(p, "wt") as f:
                f.write(text)
        else:
            p.write_text(text)
        files.append(os.path.abspath(str(p)))
    return files, bins


@pytest.fixture(scope="module")
def libraries(tmp_path_factory):
    """the two libraries on disk, and an index per distinct set of index flags"""
    root = tmp_path_factory.mktemp("align_windows_cli")
    out = {}
    for kind, seed in (("peptide", 811), ("dna", 812)):
        d = root / kind
        d.mkdir()
        seqs = _library(kind, np.random.default_rng(seed))
        files, bins = _write_bins(d, seqs)
        out[kind] = dict(dir=d, seqs=seqs, files=files, bins=bins, targets={n: r for recs in bins for n, r in recs}, indexes={})
    for name, (kind, flags, _, k, _, _) in SCENARIOS.items():
        lib = out[kind]
        key = " ".join(flags)
        if key not in lib["indexes"]:
            dest = lib["dir"] / ("index%d" % len(lib["indexes"]))
            rc, so, se = _run("index", "-k", str(k), *flags, str(dest), *lib["files"])
            assert rc == 0 and os.path.exists(str(dest) + ".ibf"), se
            lib["indexes"][key] = str(dest) + ".ibf"
    return out


class Case:
    """one command on one query file: its flags, the restatement's distances, and the runs of the command remembered by
    environment, so that the default run is made once"""

    def __init__(self, lib, index, mode, k, W, S, edits, queries, qfile):
        self.lib, self.index, self.mode, self.k, self.W, self.S, self.edits, self.queries = lib, index, mode, k, W, S, edits, queries
        self.dna = mode == "windows" and lib["bins"][0][0][1].strip("ACGT") == ""
        with open(qfile, "w") as f:
            f.write("".join(">%s some comment\n%s\n" % q for q in queries))
        if mode == "windows":
            self.flags = ("--window", str(W), "--step", str(S), "-e", str(edits), "--verify-windows")
            self.distances, _ = R.window_distances(queries, k, W, S, edits, lib["bins"], DNA_CODES if self.dna else PEPTIDE_CODES, self.dna)
        else:
            self.flags = ("--translate", "--frame-window", str(W), "--frame-step", str(S), "-e", str(edits), "--verify-frame-windows")
            self.distances, _ = RF.window_distances(queries, k, W, S, edits, lib["bins"])
        self.qfile, self.runs = qfile, {}

    def run(self, align=True, counts=False, **env):
        key = (align, counts, tuple(sorted(env.items())))
        if key not in self.runs:
            rc, so, se = _run("search", *self.flags, *(["--align-windows"] if align else []), *(["--counts"] if counts else []), self.index, self.qfile, env=env)
            assert rc == 0, se
            self.runs[key] = (so, se)
        return self.runs[key]


@pytest.fixture(scope="module")
def cases(libraries):
    out = {}
    for name, (kind, flags, mode, k, W, S) in SCENARIOS.items():
        lib = libraries[kind]
        queries = _chimeras(kind, mode, lib["seqs"], W, S, np.random.default_rng(900 + len(name)))
        out[name] = Case(lib, lib["indexes"][" ".join(flags)], mode, k, W, S, EDITS, queries, str(lib["dir"] / (name + ".fa")))
    return out


def _trace(se):
    m = re.search(r"align windows: device (\d+), host (\d+), calls (\d+)", se)
    assert m and len(re.findall(r"align windows:", se)) == 1, se
    return tuple(int(x) for x in m.groups())


def check_rows(case, so, counts=False):
    """(b) and (c) for every row of an --align-windows output; returns the rows"""
    rows = [line.split("\t") for line in so.splitlines()]
    assert rows
    names = [n for n, _ in case.queries]
    path_bin = {p: u for u, p in enumerate(case.lib["files"])}
    frames, strands, ops = set(), set(), set()
    for row in rows:
        r, u = names.index(row[0]), path_bin[row[1]]
        seq = case.queries[r][1]
        at = 2
        f = None
        if case.mode == "frames":
            f = T.FRAMES.index(row[at])
            frames.add(row[at])
            at += 1
        begin, end = int(row[at]), int(row[at + 1])
        at += 2 + (1 if counts else 0)
        distance, target, target_end = int(row[at]), row[at + 1], int(row[at + 2])
        at += 3
        strand = ""
        if case.dna:
            strand = row[at]
            strands.add(strand)
            at += 1
        assert len(row) == at + 4, row
        wbegin, wend, start, cigar = int(row[at]), int(row[at + 1]), int(row[at + 2]), row[at + 3]
        assert begin <= wbegin <= wend <= end, row
        # (b) the window, the run it belongs to, and the distances of the run's windows
        if case.mode == "windows":
            wins = [(b + 1, b + n) for b, n in windows_of(len(seq), case.k, case.W, case.S)]
            key = lambda j: (r, j, u)
        else:
            wins = [F.residues_on_record(len(seq), f, a, a + n) for a, n in F.frame_windows(len(seq), f, case.k, case.W, case.S)]
            key = lambda j: (r, f, j, u)
        assert (wbegin, wend) in wins, row
        j = wins.index((wbegin, wend))
        run = [x for x, (wb, we) in enumerate(wins) if begin <= wb and we <= end]
        assert all(key(x) in case.distances and (not case.dna or case.distances[key(x)][3] == strand) for x in run), (row, run)
        least = min(run, key=lambda x: (case.distances[key(x)][0], x))
        assert j == least and case.distances[key(j)][:3] == (distance, target, target_end), (row, j, least, case.distances[key(j)])
        # (c) cut, reverse-complement or translate; the full matrix against the target, walked back from (m, target_end)
        if case.mode == "windows":
            piece = seq[wbegin - 1:wend]
            pattern = R.revcomp(piece) if strand == "-" else piece
        else:
            pattern = F.cut_and_translate(seq, f, wbegin, wend)
        d, _, want_start, runs = A.align(pattern, case.lib["targets"][target][:target_end], DNA_CODES if case.dna else PEPTIDE_CODES, target_end)
        assert (d, want_start + 1, A.cigar(runs)) == (distance, start, cigar), (row, d, want_start + 1, A.cigar(runs))
        A.check_identities(len(pattern), d, target_end, want_start, runs)
        ops.update(c for c, _ in runs)
    return rows, frames, strands, ops


@pytest.mark.parametrize("scenario", list(SCENARIOS))
def test_rows(cases, scenario):
    """(a), (b), (c), and the trace line of the default route: pairs on the device, and fewer calls than bins with a row — one
    call aligns the rows of all bins of a batch"""
    case = cases[scenario]
    plain, _ = case.run(align=False)
    so, se = case.run()
    assert ["\t".join(line.split("\t")[:-4]) for line in so.splitlines()] == plain.splitlines() and so.endswith("\n")
    rows, frames, strands, ops = check_rows(case, so)
    device, host, calls = _trace(se)
    n_bins = len({row[1] for row in rows})
    assert n_bins >= 2 * CHIMERAS and device + host == len(rows) and device > 0 and host == 0 and 1 <= calls < n_bins, (se, n_bins)
    assert "=" in ops and ops & set("XID"), ops
    if case.dna:
        assert strands == {"+", "-"}
    if case.mode == "frames":
        assert {x[0] for x in frames} == {"+", "-"}
    assert "align windows" not in case.run(align=False)[1]


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("scenario", list(SCENARIOS))
def test_routes_give_the_same_bytes(cases, scenario, route):
    case = cases[scenario]
    base, _ = case.run()
    so, se = case.run(**ROUTES[route])
    assert so == base, (scenario, route)
    device, host, calls = _trace(se)
    n_rows = len(base.splitlines())
    if route in ("host", "written"):  # every pair on the host: no window took the window kernel, or the variable says so
        assert (device, host, calls) == (0, n_rows, 0), se
    elif route == "rounds":
        assert device == n_rows and host == 0 and calls >= 2, se
    else:
        assert device == n_rows and host == 0, se


@pytest.mark.parametrize("scenario", ["peptide_hibf", "contigs_hibf"])
def test_counts_column(cases, scenario):
    case = cases[scenario]
    plain, _ = case.run(align=False, counts=True)
    so, _ = case.run(counts=True)
    assert ["\t".join(line.split("\t")[:-4]) for line in so.splitlines()] == plain.splitlines()
    check_rows(case, so, counts=True)
    at = 5 if case.mode == "frames" else 4
    assert ["\t".join(x for i, x in enumerate(line.split("\t")) if i != at) for line in so.splitlines()] == case.run()[0].splitlines()


def test_a_window_above_512_letters_goes_to_the_host(libraries):
    """W = 600 on the nucleotide library: every window is written out and verified as a record, and its alignment is the host
    twin's"""
    lib = libraries["dna"]
    rng = np.random.default_rng(5)
    body = edit_cases.edited(rng, "ACGT", np.frombuffer(lib["seqs"][5][1][300:1700].encode(), dtype=np.uint8), 3).tobytes().decode().upper()
    queries = [("long_b5", "".join(rng.choice(list("ACGT"), size=250)) + body), ("long_rc_b5", R.revcomp(body[:900]))]
    case = Case(lib, lib["indexes"]["-n"], "windows", 16, 600, 200, EDITS, queries, str(lib["dir"] / "long.fa"))
    plain, _ = case.run(align=False)
    so, se = case.run()
    assert ["\t".join(line.split("\t")[:-4]) for line in so.splitlines()] == plain.splitlines()
    rows, _, strands, _ = check_rows(case, so)
    assert strands == {"+", "-"} and _trace(se) == (0, len(rows), 0)
    assert case.run(TETREX_VERIFY_ALIGN="host")[0] == so


def test_a_window_32_edits_away_goes_to_the_host_next_to_device_ones(libraries):
    """-e 32, W = 260 on the peptide library: one record's windows are 32 substitutions from bin 5 — in blocks, so that the
    filter still passes them —, which the device declines and the host twin aligns, the other record's are 3 edits from it"""
    lib = libraries["peptide"]
    rng = np.random.default_rng(32)
    src = lib["seqs"][5][1]
    far = list(src[400:660])
    for block in range(4):  # 4 blocks of 8 adjacent substitutions
        for at in range(30 + 60 * block, 38 + 60 * block):
            far[at] = AMINO[(AMINO.index(far[at]) + 1 + int(rng.integers(0, 19))) % 20]
    near = edit_cases.edited(rng, AMINO, np.frombuffer(src[1200:1600].encode(), dtype=np.uint8), 3).tobytes().decode().upper()
    queries = [("far_b5", "".join(far)), ("near_b5", near)]
    case = Case(lib, lib["indexes"][""], "windows", 6, 260, 70, 32, queries, str(lib["dir"] / "e32.fa"))
    assert case.distances[(0, 0, 5)][0] == 32 and all(d[0] <= 31 for key, d in case.distances.items() if key[0] == 1)
    plain, _ = case.run(align=False)
    so, se = case.run()
    assert ["\t".join(line.split("\t")[:-4]) for line in so.splitlines()] == plain.splitlines()
    rows, _, _, _ = check_rows(case, so)
    assert [row[0] for row in rows] == ["far_b5", "near_b5"] and rows[0][4] == "32"
    assert _trace(se) == (1, 1, 1)
    so_host, se_host = case.run(TETREX_VERIFY_ALIGN="host")
    assert so_host == so and _trace(se_host) == (0, 2, 0)
