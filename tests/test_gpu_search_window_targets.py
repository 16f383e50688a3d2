"""`tetrex search ... --verify-windows --window-targets` and `... --verify-frame-windows --window-targets` on indexes
that `tetrex index` builds from generated FASTA, against the Python restatement tests/window_targets_ref.py: the window layout of
tests/search_window_ref.py, the distances of tests/edit_ref.py on one-record groups, and the merge of target hits into rows.
The bins are FAMILIES: a first member, a second one that is a copy with 0 .. E + 1 edits and one block of E + 2 substitutions
(a stretch over the block matches the first member and not the second), and a third that is a shifted part of it with one edit
and, in every fourth bin, a tail of its own (a stretch of the tail matches the later record and not the first).  The queries are
chimeric records as in tests/test_gpu_search_verify_windows.py: stretches of two bins with 0 .. E edits between random letters,
and a decoy that the k-mer filter lets through and verification must reject for every member."""
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
import window_targets_ref as WT
from search_window_ref import windows_of

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
EDITS, BINS, CHIMERAS = 2, 24, 5
SEEDS = {"peptide": 511, "murphy": 512, "dna": 523, "contigs": 514}  # (settled on the CPU: the reference alone meets check_reference())
FW, FS = 40, 10  # the frame windows of the translated search, in residues
PEPTIDE_CODES, DNA_CODES = RF.PEPTIDE_CODES, E.letter_codes("ACGT", {"U": 3})
CODONS_OF = {}
for _codon, _aa in T.CODON.items():
    CODONS_OF.setdefault(_aa, []).append(_codon)


def _run(*args, env=None):
    r = subprocess.run([TETREX, *args], capture_output=True, text=True, timeout=600, env=dict(os.environ, TETREX_TRACE="1", **(env or {})))
    return r.returncode, r.stdout, r.stderr


def _substituted(rng, res, s):
    return "".join(res[(res.index(c) + 1 + int(rng.integers(0, len(res) - 1))) % len(res)] for c in s)


def _families(res, W, S, rng):
    """24 bins of three records: see the module's docstring"""
    rand = lambda n: "".join(rng.choice(list(res), size=n))
    edited = lambda s, e: edit_cases.edited(rng, res, np.frombuffer(s.encode(), dtype=np.uint8), e).tobytes().decode().upper()
    seqs, tails = [], {}
    for b in range(BINS):
        first = rand(int(rng.integers(5 * W, 6 * W)))
        at = int(rng.integers(len(first) // 2, len(first) - W))
        second = edited(first[:at] + _substituted(rng, res, first[at:at + EDITS + 2]) + first[at + EDITS + 2:], int(rng.integers(0, EDITS + 2)))
        third = edited(first[len(first) // 3:], 1)
        if b % 4 == 1:
            tails[b] = rand(W + 3 * S)
            third += tails[b]
        seqs.append([first, second, third])
    return seqs, tails


def generate(name):
    """bins, chimeric queries with where their stretches lie, and the restatement's target distances"""
    frames = name == "contigs"
    res, k, _, dna, W, S = ALPHABETS["peptide" if frames else name]
    if frames:
        W, S = FW, FS
    rng = np.random.default_rng(SEEDS[name])
    seqs, tails = _families(res, W, S, rng)
    rand = lambda n: "".join(rng.choice(list("ACGT" if frames else res), size=n))
    back = lambda pep: "".join(CODONS_OF[a][int(rng.integers(0, len(CODONS_OF[a])))] for a in pep)
    edited = lambda s, e: edit_cases.edited(rng, res, np.frombuffer(s.encode(), dtype=np.uint8), e).tobytes().decode().upper()
    unit = 3 if frames else 1

    def cut(rec, n):
        at = int(rng.integers(0, len(rec) - n + 1))
        return rec[at:at + n]
    queries, planted, decoys = [], [], []  # planted / decoys: (query, bin, begin, end) of a stretch on the record, 0-based half-open
    for q in range(CHIMERAS):
        a, d = (int(x) for x in rng.choice([b for b in range(BINS) if b % 4 != 1], size=2, replace=False))
        b = 4 * int(rng.integers(0, BINS // 4)) + 1
        parts, at = [], 0

        def add(s, into=None, bin_=None):
            nonlocal at
            s = back(s) if frames and into is not None else s
            parts.append(s)
            if into is not None:
                into.append((q, bin_, at, at + len(s)))
            at += len(s)
        add(rand(int(rng.integers(0, unit * S))))
        # a long stretch of the first member, over the place where the second has its block: the members' intervals differ
        s = edited(cut(seqs[a][0][len(seqs[a][0]) // 3:], 2 * W + 2 * S + int(rng.integers(0, S))), int(rng.integers(0, EDITS + 1)) if q else 0)
        if frames and q == 0:  # a stop in the middle of the first stretch: an edit of its own for every window that holds it (§20)
            s = back(s)
            parts.append(s[:3 * (len(s) // 6)] + "TAA" + s[3 * (len(s) // 6) + 3:])
            planted.append((q, a, at, at + len(s)))
            at += len(s)
        else:
            add(s, planted, a)
        add(rand(unit * (W // 2) + int(rng.integers(0, unit * S))))
        s = edited(cut(tails[b], W + S + 1 + int(rng.integers(0, S))), int(rng.integers(0, EDITS + 1)))  # only the third member has it
        if frames:
            parts.append(T.reverse_complement(back(s)))
            planted.append((q, b, at, at + 3 * len(s)))
            at += 3 * len(s)
        else:
            add(R.revcomp(s) if dna and q % 2 else s, planted, b)
        add(rand(unit * (W // 2) + int(rng.integers(0, unit * S))))
        s, block = cut(seqs[d][0], W + 2 * S), EDITS + 2
        for o in range(S // 2, len(s) - block, W - S - block):
            s = s[:o] + _substituted(rng, res, s[o:o + block]) + s[o + block:]
        add(s, decoys, d)
        add(rand(int(rng.integers(0, unit * S))))
        s = "".join(parts)
        if dna and q % 3 == 0:
            s = s.lower()
        queries.append(("chimera%d_b%d_b%d_d%d" % (q, a, b, d), s))
    bins = [[("b%d_%d" % (b, i), r) for i, r in enumerate(recs)] for b, recs in enumerate(seqs)]
    if frames:
        distances, n_searched = WT.frame_target_distances(queries, k, W, S, EDITS, bins)
    else:
        distances, n_searched = WT.target_distances(queries, k, W, S, EDITS, bins, DNA_CODES if dna else PEPTIDE_CODES, dna)
    return dict(name=name, frames=frames, seqs=seqs, bins=bins, queries=queries, planted=planted, decoys=decoys, distances=distances, n_searched=n_searched,
                dna=dna, k=k, W=W, S=S, targets={n: r for recs in bins for n, r in recs})


def _spans(case, r):
    """(begin, end) of a row, 1-based inclusive on the record"""
    at = 3 if case["frames"] else 2
    return int(r[at]), int(r[at + 1])


def check_reference(case, rows, plain, bin_name):
    """the conditions that keep the tests from passing on nothing, on the reference's rows with the flag and without it"""
    name = case["name"]
    at = 5 if case["frames"] else 4  # the column of the distance; the target follows
    by_pair = {}
    for r in rows:
        by_pair.setdefault((r[0], r[1]), {}).setdefault(r[at + 1], set()).add(_spans(case, r))
    assert any(len(t) >= 2 and len({frozenset(s) for s in t.values()}) >= 2 for t in by_pair.values()), (name, "two targets of a pair with other intervals")
    named = {(r[0], r[1], r[at + 1]) for r in plain}
    assert any((r[0], r[1], r[at + 1]) not in named for r in rows), (name, "a target --verify-windows does not name")
    first_missing = [key for key in case["distances"] if key[-1] > 0 and key[:-1] + (0,) not in case["distances"]]
    assert first_missing, (name, "a window that hits a later record and not the first")
    unit = 3 if case["frames"] else 1
    for q, b, begin, end in case["planted"]:
        assert any(r[0] == case["queries"][q][0] and r[1] == bin_name(b) and min(_spans(case, r)[1], end) - max(_spans(case, r)[0] - 1, begin) >= unit * case["W"]
                   for r in rows), (name, "planted", q, b)
    for q, b, begin, end in case["decoys"]:
        assert not any(r[0] == case["queries"][q][0] and r[1] == bin_name(b) and _spans(case, r)[0] - 1 < end and _spans(case, r)[1] > begin for r in rows), (name, "decoy", q, b)


def reference(case, files):
    """(rows with the flag, rows without it, confirmed candidates, target hits) of the restatement, bins as file paths"""
    k, W, S, queries = case["k"], case["W"], case["S"], case["queries"]
    if case["frames"]:
        rows, n_confirmed, n_targets = WT.frame_rows_of(queries, k, W, S, BINS, case["distances"])
        plain, n_plain = RF.rows_of(queries, k, W, S, BINS, WT.frame_nearest_of(case["distances"]))
    else:
        rows, n_confirmed, n_targets = WT.rows_of(queries, k, W, S, BINS, case["distances"])
        plain, n_plain = R.rows_of(queries, k, W, S, BINS, WT.nearest_of(case["distances"]))
    assert n_plain == n_confirmed
    text = lambda rs: [(r[0], files[r[1]]) + tuple(str(x) for x in r[2:]) for r in rs]
    return text(rows), text(plain), n_confirmed, n_targets


@pytest.fixture(scope="module")
def setups(tmp_path_factory):
    root = tmp_path_factory.mktemp("window_targets_cli")
    out = {}
    for name in list(ALPHABETS) + ["contigs"]:
        case = generate(name)
        res, k, flags, dna, _, _ = ALPHABETS["peptide" if name == "contigs" else name]
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
        qf.write_text("".join(">%s some comment\n%s\n" % (n, s) for n, s in case["queries"]))
        indexes = {}
        for lay, lflags in LAYOUTS.items():
            if name == "contigs" and lay != "default":
                continue
            rc, so, se = _run("index", "-k", str(k), *flags, *lflags, str(d / lay), *files)
            assert rc == 0 and os.path.exists(d / (lay + ".ibf")), se
            indexes[lay] = str(d / (lay + ".ibf"))
        want, plain, n_confirmed, n_targets = reference(case, files)
        check_reference(case, want, plain, lambda b: files[b])
        if name == "contigs":
            flags = ("--translate", "--frame-window", str(FW), "--frame-step", str(FS), "-e", str(EDITS), "--verify-frame-windows")
        else:
            flags = ("--window", str(case["W"]), "--step", str(case["S"]), "-e", str(EDITS), "--verify-windows")
        out[name] = dict(case=case, files=files, qfile=str(qf), indexes=indexes, want=want, plain=plain, n_confirmed=n_confirmed, n_targets=n_targets, flags=flags)
    return out


def _rows(stdout):
    return [tuple(line.split("\t")) for line in stdout.splitlines()]


def _trace(se):
    m = re.search(r"window targets: device (\d+), host (\d+), calls (\d+)", se)
    assert m and len(re.findall(r"window targets:", se)) == 1, se
    return tuple(int(x) for x in m.groups())


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("alphabet", list(ALPHABETS))
def test_rows_match_the_reference(setups, alphabet, layout):
    s = setups[alphabet]
    rc, so, se = _run("search", *s["flags"], "--window-targets", "-v", s["indexes"][layout], s["qfile"])
    assert rc == 0, se
    got = _rows(so)
    assert got == s["want"], (alphabet, layout, [x for x in got if x not in s["want"]][:3], [x for x in s["want"] if x not in got][:3])
    # the output without the flag: --verify-windows' own, which is what the least target hit of every window gives (invariant (b))
    rc, plain_so, plain_se = _run("search", *s["flags"], "-v", s["indexes"][layout], s["qfile"])
    assert rc == 0 and _rows(plain_so) == s["plain"], plain_se
    assert "Targets:" not in plain_se and "window targets:" not in plain_se
    # invariant (a): the same letters of every (record, bin) are covered
    assert WT.union_of(got) == WT.union_of(_rows(plain_so))
    m, p = (re.search(r"Verified: (\d+) of (\d+) candidate windows", x) for x in (se, plain_se))
    assert m and p and m.groups() == p.groups() and int(m.group(1)) == s["n_confirmed"], (se, plain_se)
    t = re.search(r"Targets: (\d+)", se)
    assert t and int(t.group(1)) == s["n_targets"] > s["n_confirmed"], se
    w = re.search(r"Windows: (\d+) searched, (\d+) hit, (\d+) rows", se)
    assert w and int(w.group(1)) == s["case"]["n_searched"] and int(w.group(3)) == len(got), se
    # ONE call per round over all bins: fewer calls than bins with a row, every candidate on the device
    device, host, calls = _trace(se)
    assert device == int(m.group(2)) and host == 0 and 1 <= calls < len({r[1] for r in got}), se
    if s["case"]["dna"]:
        assert {r[-1] for r in got} == {"+", "-"}


ROUTES = {  # environment of a run that must write the bytes of the default run, and what its trace line must say
    "host": ({"TETREX_VERIFY_TARGETS": "host"}, lambda device, host, calls, n: device == 0 and calls == 0 and host == n),
    "written": ({"TETREX_VERIFY_WINDOWS": "written", "TETREX_VERIFY_FRAME_WINDOWS": "written"}, lambda device, host, calls, n: device == 0 and calls == 0 and host == n),
    "rounds": ({"TETREX_VERIFY_TEXT_MB": "0.004"}, lambda device, host, calls, n: device + host == n and calls > 1),  # about 4 KiB of resident text: a few bins a round
    "bin above the slots": ({"TETREX_VERIFY_TARGET_SLOTS": "2"}, lambda device, host, calls, n: device == 0 and calls == 0 and host == n),  # every bin has 3 records
    "several calls": ({"TETREX_VERIFY_TARGET_SLOTS": "5"}, lambda device, host, calls, n: device == n and host == 0 and calls > 1),  # 40 slots a round
    "batches": ({"TETREX_SEARCH_BATCH_WINDOWS": "7"}, lambda device, host, calls, n: device == n and host == 0),
}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("alphabet", list(ALPHABETS) + ["contigs"])
def test_routes_give_the_same_bytes(setups, alphabet, route):
    s = setups[alphabet]
    args = ("search", *s["flags"], "--window-targets", "--counts", "-v", s["indexes"]["default"], s["qfile"])
    if "base" not in s:
        rc, so, se = _run(*args)
        assert rc == 0 and so, se
        s["base"] = (so, int(re.search(r"Verified: \d+ of (\d+) candidate windows", se).group(1)))
    env, expect = ROUTES[route]
    rc, so, se = _run(*args, env=env)
    assert rc == 0 and so == s["base"][0], se
    assert expect(*_trace(se), s["base"][1]), (route, se)


def test_frame_windows(setups):
    """the translated search on contigs: rows, the output without the flag, invariants, the lines of -v"""
    s = setups["contigs"]
    rc, so, se = _run("search", *s["flags"], "--window-targets", "-v", s["indexes"]["default"], s["qfile"])
    assert rc == 0, se
    got = _rows(so)
    assert got == s["want"], ([x for x in got if x not in s["want"]][:3], [x for x in s["want"] if x not in got][:3])
    rc, plain_so, plain_se = _run("search", *s["flags"], "-v", s["indexes"]["default"], s["qfile"])
    assert rc == 0 and _rows(plain_so) == s["plain"], plain_se
    key = lambda rows: WT.union_of([(r[0], r[1] + r[2]) + r[3:] for r in rows])  # per (record, frame, bin)
    assert key(got) == key(_rows(plain_so))
    m, p = (re.search(r"Verified: (\d+) of (\d+) candidate windows", x) for x in (se, plain_se))
    assert m and p and m.groups() == p.groups() and int(m.group(1)) == s["n_confirmed"], (se, plain_se)
    t = re.search(r"Targets: (\d+)", se)
    assert t and int(t.group(1)) == s["n_targets"] > s["n_confirmed"], se
    device, host, calls = _trace(se)
    assert device == int(m.group(2)) and host == 0 and 1 <= calls < len({r[1] for r in got}), se
    assert {r[2][0] for r in got} == {"+", "-"}  # (frames of both strands)
    # a stretch with a stop in a window: §20's rule decides what is searched, with the flag as without it
    w, pw = (re.search(r"Windows: (\d+) searched, (\d+) hit", x) for x in (se, plain_se))
    assert w and pw and w.groups() == pw.groups() and int(w.group(1)) == s["case"]["n_searched"]


@pytest.mark.parametrize("alphabet", list(ALPHABETS) + ["contigs"])
def test_align_windows(setups, alphabet):
    """with --align-windows: four columns more on the same rows, and every row's start and cigar re-derived by the full matrix of
    its window against ITS target"""
    s = setups[alphabet]
    case = s["case"]
    rc, so, se = _run("search", *s["flags"], "--window-targets", "--align-windows", s["indexes"]["default"], s["qfile"])
    assert rc == 0, se
    got = _rows(so)
    assert [r[:-4] for r in got] == s["want"]
    names = [n for n, _ in case["queries"]]
    ops = set()
    for row in got:
        seq = case["queries"][names.index(row[0])][1]
        at = 3 if case["frames"] else 2
        begin, end, distance, target, target_end = int(row[at]), int(row[at + 1]), int(row[at + 2]), row[at + 3], int(row[at + 4])
        strand = row[at + 5] if case["dna"] else ""
        wbegin, wend, start, cigar = int(row[-4]), int(row[-3]), int(row[-2]), row[-1]
        assert begin <= wbegin <= wend <= end, row
        if case["frames"]:
            f = T.FRAMES.index(row[2])
            assert (wbegin, wend) in [F.residues_on_record(len(seq), f, a, a + n) for a, n in F.frame_windows(len(seq), f, case["k"], case["W"], case["S"])], row
            pattern = F.cut_and_translate(seq, f, wbegin, wend)
        else:
            assert (wbegin, wend) in [(b + 1, b + n) for b, n in windows_of(len(seq), case["k"], case["W"], case["S"])], row
            pattern = R.revcomp(seq[wbegin - 1:wend]) if strand == "-" else seq[wbegin - 1:wend]
        d, _, want_start, runs = A.align(pattern, case["targets"][target][:target_end], DNA_CODES if case["dna"] else PEPTIDE_CODES, target_end)
        assert (d, want_start + 1, A.cigar(runs)) == (distance, start, cigar), (row, d, want_start + 1, A.cigar(runs))
        ops.update(c for c, _ in runs)
    assert "=" in ops and len(ops) >= 2, ops
    m = re.search(r"align windows: device (\d+), host (\d+), calls (\d+)", se)
    assert m and int(m.group(1)) == len(got) and int(m.group(2)) == 0, se


def test_a_window_above_512_letters_is_written_out(setups):
    """W = 600 on the nucleotide index: every window takes verify()'s long-pattern route with rows, and gives the reference's rows"""
    s = setups["dna"]
    case = s["case"]
    rng = np.random.default_rng(5)
    src = case["seqs"][5][0]
    body = edit_cases.edited(rng, "ACGT", np.frombuffer(src[20:].encode(), dtype=np.uint8), 2).tobytes().decode().upper()
    records = [("long_b5", "".join(rng.choice(list("ACGT"), size=250)) + body), ("long_rc_b5", R.revcomp(body[:650]))]
    qf = os.path.join(os.path.dirname(s["qfile"]), "long.fa")
    with open(qf, "w") as f:
        f.write("".join(">%s\n%s\n" % r for r in records))
    W, S = 600, 100
    distances, _ = WT.target_distances(records, case["k"], W, S, EDITS, case["bins"], DNA_CODES, True)
    want, n_confirmed, n_targets = WT.rows_of(records, case["k"], W, S, BINS, distances)
    want = [(r[0], s["files"][r[1]]) + tuple(str(x) for x in r[2:]) for r in want]
    assert n_confirmed >= 2 and {r[-1] for r in want} == {"+", "-"}
    rc, so, se = _run("search", "--window", str(W), "--step", str(S), "-e", str(EDITS), "--verify-windows", "--window-targets", "-v", s["indexes"]["default"], qf)
    assert rc == 0, se
    assert _rows(so) == want
    device, host, calls = _trace(se)
    assert device == 0 and calls == 0 and host >= n_confirmed, se
