"""`tetrex search --verify --all-targets` on two small libraries, peptide and nucleotide, that `tetrex index`
builds from generated FASTA: 5 bins of 3 to 4 records.  Queries of about 300, 600 and 1500 letters and one of 4200 (the host
route) are cut with 0 to 3 edits from letters that lie in two records of one bin and in one record of another; every other
nucleotide query is reverse-complemented; a decoy per length has five adjacent substitutions.  The reference is
tetrex_amd.host.edit_search (code that was there before the flag) with every record a group of its own."""
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
LIBRARIES = {"peptide": (AMINO, 6, [], False), "dna": ("ACGT", 16, ["-n"], True)}  # name: (residues, k, index flags, dna)
CODES = {"peptide": E.letter_codes("ABCDEFGHIJKLMNOPQRSTUVWXYZ"), "dna": E.letter_codes("ACGT", {"U": 3})}
EDITS, BINS = 3, 5
QUERY_LENGTHS = [300, 600, 1500]
CODONS_OF = {}
for _codon, _aa in T.CODON.items():
    CODONS_OF.setdefault(_aa, []).append(_codon)


def _run(*args, env=None):
    r = subprocess.run([TETREX, *args], capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    return r.returncode, r.stdout, r.stderr


def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _letters(rng, res, n):
    return "".join(rng.choice(list(res), size=int(n)))


def _generate(name):
    """the library's records, its queries (name, letters, edits applied or None for a decoy) and a 60-residue piece that lies
    in two proteins of one bin (for --translate)"""
    res, _, _, dna = LIBRARIES[name]
    rng = np.random.default_rng(300 + len(name))
    n_records = [3, 4, 3, 4, 3]
    seqs = [[_letters(rng, res, rng.integers(100, 300)) for _ in range(n)] for n in n_records]
    queries = []

    def plant(source, twice_only=False):
        b = int(rng.integers(0, BINS))
        i1, i2 = (int(x) for x in rng.choice(n_records[b], size=2, replace=False))
        places = [(b, i1), (b, i2)]
        if not twice_only:
            b2 = (b + 1 + int(rng.integers(0, BINS - 1))) % BINS
            places.append((b2, int(rng.integers(0, n_records[b2]))))
        for bb, ii in places:
            seqs[bb][ii] += source + _letters(rng, res, rng.integers(100, 300))
        return b

    for qlen in QUERY_LENGTHS + [4200]:
        for q in range(1 if qlen == 4200 else 4):
            source = _letters(rng, res, qlen)
            b = plant(source, twice_only=qlen == 4200)
            if q < 3:
                e = 1 if qlen == 4200 else q if q < 2 else EDITS
                s = edit_cases.edited(rng, res, np.frombuffer(source.encode(), dtype=np.uint8), e).tobytes().decode().upper()
            else:
                e, mid = None, qlen // 2
                s = source[:mid] + "".join(res[(res.index(c) + 1) % len(res)] for c in source[mid:mid + 5]) + source[mid + 5:]
            if dna and q % 2:
                s = _revcomp(s)
            queries.append(("q%d_%d_b%d" % (qlen, q, b), s, e))
    piece = _letters(rng, res, 60)
    plant(piece, twice_only=True)
    return seqs, queries, piece


@pytest.fixture(scope="module")
def cli_setup(tmp_path_factory):
    from tetrex_amd import host
    root = tmp_path_factory.mktemp("search_targets_cli")
    out = {}
    for name, (res, k, flags, dna) in LIBRARIES.items():
        seqs, queries, piece = _generate(name)
        d = root / name
        d.mkdir()
        files = []
        for b, recs in enumerate(seqs):
            p = d / ("bin%02d.fa" % b)
            p.write_text("".join(">b%d_%d description\n%s\n" % (b, i, r) for i, r in enumerate(recs)))
            files.append(os.path.abspath(str(p)))
        qf = d / "queries.fa"
        qf.write_text("".join(">%s some comment\n%s\n" % (n, s) for n, s, _ in queries))
        rc, so, se = _run("index", "-k", str(k), *flags, "-i", str(d / "flat"), *files)
        assert rc == 0 and os.path.exists(d / "flat.ibf"), se
        # the reference: every query (on DNA both strands) against every record as a group of its own
        records = [r for recs in seqs for r in recs]
        names = ["b%d_%d" % (b, i) for b, recs in enumerate(seqs) for i in range(len(recs))]
        first = np.cumsum([0] + [len(recs) for recs in seqs])
        patterns = [s for _, s, _ in queries] + ([_revcomp(s) for _, s, _ in queries] if dna else [])
        pairs = [(p, r, EDITS) for p in range(len(patterns)) for r in range(len(records))]
        ref = host.edit_search(patterns, records, list(range(len(records) + 1)), pairs, CODES[name], threads=8).reshape(len(patterns), len(records), 3)
        out[name] = dict(files=files, queries=queries, qfile=str(qf), index=str(d / "flat.ibf"), dna=dna, ref=ref, names=names, first=first,
                         records=dict(zip(names, records)), piece=piece, dir=d, rng=np.random.default_rng(9))
    return out


def _reference_rows(setup, q, b):
    """the columns the reference gives for query q in bin b: one tuple per target within EDITS, in the order of the bin's file"""
    n, rows = len(setup["queries"]), []
    for r in range(setup["first"][b], setup["first"][b + 1]):
        best = None
        for strand in ((0, 1) if setup["dna"] else (0,)):
            d, _, j = (int(x) for x in setup["ref"][q + strand * n, r])
            if d != E.NONE and (best is None or d < best[0]):
                best = (d, setup["names"][r], j, "+-"[strand])
        if best is not None:
            rows.append((str(best[0]), best[1], str(best[2])) + ((best[3],) if setup["dna"] else ()))
    return rows


def _routes(stderr):
    m = re.search(r"verify routes: device (\d+), device-long (\d+), host (\d+)", stderr)
    assert m, stderr
    return tuple(int(x) for x in m.groups())


@pytest.fixture(scope="module")
def runs(cli_setup):
    """per library: the plain search, --verify, and --verify --all-targets -v with its trace, run once"""
    out = {}
    for library, setup in cli_setup.items():
        args = ("search", "-e", str(EDITS), "--counts")
        rc, plain, se = _run(*args, setup["index"], setup["qfile"])
        assert rc == 0, se
        rc, best, se = _run(*args, "--verify", setup["index"], setup["qfile"])
        assert rc == 0, se
        rc, every, se = _run(*args, "--verify", "--all-targets", "-v", setup["index"], setup["qfile"], env={"TETREX_TRACE": "1"})
        assert rc == 0, se
        out[library] = dict(plain=plain, best=best, every=every, stderr=se, args=args)
    return out


@pytest.mark.parametrize("library", list(LIBRARIES))
def test_rows_equal_the_per_record_reference(cli_setup, runs, library):
    setup, run = cli_setup[library], runs[library]
    index_of = {n: i for i, (n, _, _) in enumerate(setup["queries"])}
    length_of = {n: len(s) for n, s, _ in setup["queries"]}
    bin_of = {p: b for b, p in enumerate(setup["files"])}
    plain = [tuple(line.split("\t")) for line in run["plain"].splitlines()]
    want, per_pair = [], []
    for row in plain:
        cols = _reference_rows(setup, index_of[row[0]], bin_of[row[1]])
        want += [row + c for c in cols]
        per_pair.append(len(cols))
    got = [tuple(line.split("\t")) for line in run["every"].splitlines()]
    assert got == want, (library, [x for x in got if x not in want][:3], [x for x in want if x not in got][:3])
    # -v and the trace: pairs, rows, and the routes counting pairs as without the flag
    n_4200 = sum(1 for r in plain if length_of[r[0]] > 4096)
    n_short = sum(1 for r in plain if length_of[r[0]] <= 512)
    confirmed = sum(1 for n in per_pair if n)
    assert "Verified: %d of %d candidate pairs" % (confirmed, len(plain)) in run["stderr"] and "Targets: %d\n" % len(want) in run["stderr"], run["stderr"]
    assert _routes(run["stderr"]) == (n_short, len(plain) - n_short - n_4200, n_4200) and n_short >= 6 and n_4200 >= 1
    # the conditions that keep this test from passing on nothing
    assert sum(1 for n in per_pair if n >= 2) >= 4 and sum(1 for n in per_pair if n == 0) >= 3, per_pair
    if setup["dna"]:
        assert {r[6] for r in got} == {"+", "-"}
    for n, _, e in setup["queries"]:  # a query lies in two records of one bin and one of another; a decoy in none
        mine = [r for r in got if r[0] == n]
        if e is None:
            assert not mine and sum(1 for r in plain if r[0] == n) >= 2, n
        else:
            assert len(mine) >= (2 if length_of[n] > 4096 else 3) and all(int(r[3]) <= e for r in mine), (n, mine)


@pytest.mark.parametrize("library", list(LIBRARIES))
def test_best_row_of_each_pair_is_the_row_without_the_flag(runs, library):
    """the lowest-distance, first-target row of each (record, bin) is the row of --verify, byte for byte"""
    run = runs[library]
    best = {}
    for line in run["every"].splitlines():
        cols = line.split("\t")
        key = (cols[0], cols[1])
        if key not in best or int(cols[3]) < int(best[key].split("\t")[3]):
            best[key] = line
    assert list(best.values()) == run["best"].splitlines() and len(best) >= 10


@pytest.mark.parametrize("library", list(LIBRARIES))
def test_routes_and_cuts_give_the_same_rows(cli_setup, runs, library):
    setup, run = cli_setup[library], runs[library]
    n_pairs = len(run["plain"].splitlines())
    for env in ({"TETREX_VERIFY_TARGETS": "host"}, {"TXQ_EDIT_CHUNK": "64", "TXQ_EDIT_LONG_SPAN": "64"}, {"TETREX_VERIFY_TARGET_SLOTS": "5"},
                {"TETREX_VERIFY_TARGET_SLOTS": "2"}, {"TETREX_VERIFY_LONG": "0"}):
        rc, so, se = _run(*run["args"], "--verify", "--all-targets", setup["index"], setup["qfile"], env=dict(env, TETREX_TRACE="1"))
        assert rc == 0 and so == run["every"], (env, se)
        device, device_long, on_host = _routes(se)
        assert device + device_long + on_host == n_pairs
        if "TETREX_VERIFY_TARGETS" in env:
            assert on_host == n_pairs
        if env.get("TETREX_VERIFY_TARGET_SLOTS") == "5":  # (a bin of 3 or 4 records: one pair a call, two where the bin has 3 and one strand)
            assert (device, device_long, on_host) == _routes(run["stderr"])
        if env.get("TETREX_VERIFY_TARGET_SLOTS") == "2":  # (every bin has more records than a call may have slots)
            assert on_host == n_pairs
        if "TETREX_VERIFY_LONG" in env:
            assert device_long == 0 and device == _routes(run["stderr"])[0]
    # --counts repeats the pair's count on each of its rows; without it the rows lose that column
    rc, so, se = _run("search", "-e", str(EDITS), "--verify", "--all-targets", setup["index"], setup["qfile"])
    assert rc == 0, se
    assert so.splitlines() == ["\t".join(c for i, c in enumerate(line.split("\t")) if i != 2) for line in run["every"].splitlines()]


@pytest.mark.parametrize("library", list(LIBRARIES))
def test_every_row_gets_its_own_alignment(cli_setup, runs, library):
    setup, run = cli_setup[library], runs[library]
    dna = setup["dna"]
    letters = {n: s for n, s, _ in setup["queries"]}
    rc, so, se = _run(*run["args"], "--verify", "--all-targets", "--align", setup["index"], setup["qfile"], env={"TETREX_TRACE": "1"})
    assert rc == 0, se
    rows = [line.split("\t") for line in so.splitlines()]
    assert ["\t".join(r[:-2]) for r in rows] == run["every"].splitlines()
    starts = set()
    for row in rows:
        s = letters[row[0]]
        if dna and row[6] == "-":
            s = _revcomp(s)
        distance, target, end = int(row[3]), row[4], int(row[5])
        # An alignment of at most EDITS edits that ends at `end` begins no earlier than end - m - EDITS, and so does every path
        # the walk's rules compare it with: the letters in front of that change nothing, the yardstick need not fill them in
        lo = max(0, end - len(s) - EDITS - 5)
        d, j, start, ops = A.align(s, setup["records"][target][lo:end], CODES[library], j=end - lo)
        assert (d, lo + start + 1, A.cigar(ops)) == (distance, int(row[-2]), row[-1]), (row[:6], d, lo + start, A.cigar(ops)[:80])
        starts.add((row[0], row[1], int(row[-2])))
    m = re.search(r"align routes: device (\d+), host (\d+)", se)
    n_host_rows = sum(1 for r in rows if len(letters[r[0]]) > 4096)
    assert m and (int(m.group(1)), int(m.group(2))) == (len(rows) - n_host_rows, n_host_rows) and n_host_rows >= 2, se
    rc, so_host, se = _run(*run["args"], "--verify", "--all-targets", "--align", setup["index"], setup["qfile"], env={"TETREX_VERIFY_ALIGN": "host"})
    assert rc == 0 and so_host == so, se


def test_translated_frames_get_a_row_per_protein(cli_setup):
    """--translate --verify-frames --all-targets on the peptide library: a read whose frame lies in two proteins of one bin gets
    two rows there, equal to the reference's per-record answers"""
    from tetrex_amd import host
    setup = cli_setup["peptide"]
    rng = setup["rng"]
    piece = edit_cases.edited(rng, AMINO, np.frombuffer(setup["piece"].encode(), dtype=np.uint8), 1).tobytes().decode().upper()
    reads = {}
    for i, aa in enumerate((piece, setup["piece"][5:55])):
        nt = "ACGT"[i] * i + "".join(CODONS_OF[a][int(rng.integers(0, len(CODONS_OF[a])))] for a in aa)
        reads["r%d" % i] = _revcomp(nt) if i % 2 else nt
    rf = setup["dir"] / "reads.fa"
    rf.write_text("".join(">%s\n%s\n" % (n, s) for n, s in reads.items()))
    args = ("search", "--translate", "-e", str(EDITS), "--verify-frames")
    rc, best, se = _run(*args, setup["index"], str(rf))
    assert rc == 0, se
    rc, every, se = _run(*args, "--all-targets", "-v", setup["index"], str(rf))
    assert rc == 0, se
    rows = [line.split("\t") for line in every.splitlines()]
    names = list(setup["records"])
    records = list(setup["records"].values())
    bin_of = {p: b for b, p in enumerate(setup["files"])}
    want = []
    for name, path, frame in sorted({(r[0], r[1], r[2]) for r in rows}, key=lambda x: (x[0], T.FRAMES.index(x[2]), x[1])):
        b = bin_of[path]
        span = range(setup["first"][b], setup["first"][b + 1])
        res = host.edit_search([T.translate_frame(reads[name], T.FRAMES.index(frame))], records, list(range(len(records) + 1)),
                               [(0, r, EDITS) for r in span], CODES["peptide"])
        want += [[name, path, frame, str(d), names[r], str(j)] for d, r, j in res.tolist() if d != E.NONE]
    assert rows == want
    for name in reads:  # two proteins of one bin, the rows next to each other
        mine = [r for r in rows if r[0] == name]
        assert len(mine) == 2 and mine[0][1] == mine[1][1] and mine[0][4] != mine[1][4] and mine[0][2] == mine[1][2], mine
    assert {r[2][0] for r in rows} == {"+", "-"}
    assert "Targets: %d\n" % len(rows) in se and "Verified: 2 of " in se, se
    # without the flag: the better row of each pair
    assert best.splitlines() == ["\t".join(min((r for r in rows if r[0] == name), key=lambda r: int(r[3]))) for name in reads]


def test_all_targets_is_refused_without_verification(cli_setup):
    setup = cli_setup["peptide"]
    for args in (("search", "--all-targets"), ("search", "--threshold", "0.5", "--all-targets"), ("search", "-e", "1", "--all-targets"),
                 ("search", "--translate", "-e", "1", "--all-targets")):
        rc, so, se = _run(*args, str(setup["dir"] / "missing.ibf"), setup["qfile"])
        assert rc == 1 and so == "" and "[Search Parser Error] --all-targets" in se and "--verify" in se and "Index not valid" not in se, (args, se)


@pytest.mark.parametrize("library", list(LIBRARIES))
def test_small_text_cache_gives_the_same_rows(cli_setup, runs, library):
    """TETREX_VERIFY_TEXT_MB is a bound, not a result: with room for one bin at a time (a fraction of a MiB: every bin pushes
    the one before it out, and the align stage brings each back once more) the rows, their target names included, are the same"""
    setup, run = cli_setup[library], runs[library]
    args = (*run["args"], "--verify", "--all-targets", "--align", setup["index"], setup["qfile"])
    rc, so, se = _run(*args)
    assert rc == 0 and so, se
    assert ["\t".join(line.split("\t")[:-2]) for line in so.splitlines()] == run["every"].splitlines()
    for env in ({"TETREX_VERIFY_TEXT_MB": "0.001"}, {"TETREX_VERIFY_TEXT_MB": "0.001", "TETREX_VERIFY_TARGET_SLOTS": "5", "TXQ_EDIT_CHUNK": "64"}):
        rc, small, se = _run(*args, env=env)
        assert rc == 0 and small == so, (env, se)
    rc, small, se = _run(*run["args"], "--verify", "--all-targets", setup["index"], setup["qfile"], env={"TETREX_VERIFY_TEXT_MB": "0.001"})
    assert rc == 0 and small == run["every"], se
