"""The record filter of `tetrex query --gpu-verify` on the CPU: the exported automaton (include/txq_regex.h,
txh_regex_automaton) and its inline interpreter (txh_regex_filter) against the verification matcher itself — an automaton
accepts a record exactly when txh_regex_find_all reports a match in it.  No GPU."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from family_fasta import family_library
from motifs import DNA_QUERIES, PEPTIDE_QUERIES
from tetrex_amd import host

EXTRA = ["^M.K", "GT$", "^MAEG$", "(A|)", "A.{12}C"]
PEPTIDE = PEPTIDE_QUERIES + EXTRA
DNA = DNA_QUERIES + EXTRA
AA = "ACDEFGHIKLMNPQRSTVWY"
COMPLEMENT = np.arange(256, dtype=np.uint8)  # comp_tab of verification (host/verify.cpp), IUPAC letters
for a, b in ("AT", "CG", "GC", "TA", "UA", "at", "cg", "gc", "ta", "ua", "MK", "KM", "RY", "YR", "VB", "BV", "HD", "DH"):
    COMPLEMENT[ord(a)] = ord(b)


def sample(rx, rng, alphabet):
    """a string the pattern matches: a random walk over the grammar the motifs use (literals . [] [^] () | ? * + {m} {m,n};
    ^ and $ give nothing)"""
    pos = 0

    def alt():
        nonlocal pos
        branches = [cat()]
        while pos < len(rx) and rx[pos] == "|":
            pos += 1
            branches.append(cat())
        return branches[int(rng.integers(len(branches)))]

    def cat():
        nonlocal pos
        parts = []
        while pos < len(rx) and rx[pos] not in "|)":
            parts.append(repeat())
        return lambda: "".join(p() for p in parts)

    def repeat():
        nonlocal pos
        a = atom()
        while pos < len(rx) and rx[pos] in "*+?{":
            c = rx[pos]
            if c == "{":
                end = rx.index("}", pos)
                lo, _, hi = rx[pos + 1:end].partition(",")
                lo = int(lo)
                hi = lo if not _ else (lo + 2 if hi == "" else int(hi))
                pos = end + 1
            else:
                lo, hi = {"*": (0, 2), "+": (1, 3), "?": (0, 1)}[c]
                pos += 1
            a = (lambda a, lo, hi: lambda: "".join(a() for _ in range(int(rng.integers(lo, hi + 1)))))(a, lo, hi)
        return a

    def atom():
        nonlocal pos
        c = rx[pos]
        pos += 1
        if c == "(":
            inner = alt()
            pos += 1  # )
            return inner
        if c in "^$":
            return lambda: ""
        if c == ".":
            return lambda: alphabet[int(rng.integers(len(alphabet)))]
        if c == "[":
            end = rx.index("]", pos + 1)
            body = rx[pos:end]
            pos = end + 1
            letters = [x for x in alphabet if x not in body[1:]] if body[0] == "^" else list(body)
            return lambda: letters[int(rng.integers(len(letters)))]
        return lambda: c

    return alt()()


def records_for(rx, alphabet, seed):
    """random records, some with a planted match: in the middle, at the first byte, at the last byte, the match alone; records
    of no bytes, lower case, bytes outside the alphabet"""
    rng = np.random.default_rng(seed)
    rnd = lambda n: "".join(rng.choice(list(alphabet), size=n)) if n else ""
    recs = [b"", rnd(1).encode(), rnd(40).encode(), rnd(120).encode()]
    for _ in range(3):
        hit = sample(rx, rng, alphabet)
        recs += [(rnd(17) + hit + rnd(23)).encode(), (hit + rnd(30)).encode(), (rnd(30) + hit).encode(), hit.encode(),
                 (rnd(9) + hit.lower() + rnd(9)).encode(), (rnd(5) + hit[:len(hit) // 2] + "\n" + hit[len(hit) // 2:] + rnd(5)).encode(),
                 rnd(8).encode() + b"\x00\xff*-" + hit.encode() + b"\x80"]
    recs.append(b"")
    return recs


def filtered(blob, recs, **kw):
    return host.regex_filter([blob], recs, [0, len(recs)], [(0, 0)], **kw)[0].tolist()


@pytest.mark.parametrize("posix", [True, False])
@pytest.mark.parametrize("family", ["peptide", "dna"])
def test_automaton_accepts_exactly_the_records_find_all_matches_in(family, posix):
    motifs, alphabet = (PEPTIDE, AA) if family == "peptide" else (DNA, "ACGT")
    planted = 0
    for i, rx in enumerate(motifs):
        pattern = "(" + rx + ")"  # as verification hands it to the matcher
        blob = host.regex_automaton(pattern, posix)
        assert blob is not None and len(blob) % 16 == 0, rx
        recs = records_for(rx, alphabet, 100 + i)
        want = [len(host.regex_find_all(pattern, r, posix)) > 0 for r in recs]
        assert filtered(blob, recs) == want, rx
        planted += sum(want)
    assert planted > 4 * len(motifs)  # the planted matches are matches


def test_reverse_strand_automaton_is_the_matcher_on_the_reverse_complement():
    for i, rx in enumerate(DNA):
        pattern = "(" + rx + ")"
        blob = host.regex_automaton(pattern, False, strand=1, byte_map=COMPLEMENT)
        recs = records_for(rx, "ACGT", 300 + i)
        recs += [bytes(COMPLEMENT[np.frombuffer(r, dtype=np.uint8)])[::-1] for r in recs[4:12]] + [b"ACGTNRYKMacgtn", b"TGTAATC"]
        want = [len(host.regex_find_all(pattern, bytes(COMPLEMENT[np.frombuffer(r, dtype=np.uint8)])[::-1], False)) > 0 for r in recs]
        assert filtered(blob, recs) == want, rx
        assert any(want), rx


def test_murphy_byte_map_is_matching_on_the_reduced_text():
    table = host.reduce_table(1)
    assert bytes(table[[ord("L"), ord("V"), ord("I"), ord("M")]]) == b"IIII"
    reduced = lambda s: "".join(chr(table[ord(c)]) if c.isalpha() else c for c in s)
    for i, rx in enumerate(PEPTIDE):
        pattern = "(" + reduced(rx) + ")"  # (what reduce_query_alphabet makes of these motifs: letter by letter)
        blob = host.regex_automaton(pattern, True, byte_map=table)
        recs = records_for(rx, AA, 500 + i)
        want = [len(host.regex_find_all(pattern, bytes(table[np.frombuffer(r, dtype=np.uint8)]), True)) > 0 for r in recs]
        assert filtered(blob, recs) == want, rx
        assert any(want), rx


def test_size_limits():
    assert host.regex_automaton("(A.{15}C)", True) is None  # 2^16 states and two: too large
    big = host.regex_automaton("(A.{12}C)", True)
    assert big is not None and len(big) > 65536
    h = host.regex_automaton_header(big)
    assert h["n_states"] <= 65535 and h["total_bytes"] == len(big) == 288 + h["n_states"] * (2 * h["n_classes"] + 1) + (-(288 + h["n_states"] * (2 * h["n_classes"] + 1)) % 16)
    with pytest.raises(host.HostError):
        host.regex_automaton("(AC", True)
    for rx in PEPTIDE_QUERIES:
        assert len(host.regex_automaton("(" + rx + ")", True)) <= 1062 + 288 + 16, rx


def test_lmax_is_finite_exactly_without_star_plus_and_open_ranges():
    for rx in PEPTIDE + DNA + ["A{2,}C", "A{2,5}C", "(AB){3}", "A?B"]:
        unbounded = any(op in rx for op in ("*", "+", ",}"))
        lmax = host.regex_automaton_header(host.regex_automaton("(" + rx + ")", True))["lmax"]
        assert (lmax == host.REGEX_UNBOUNDED) == unbounded, rx
    header = lambda rx: host.regex_automaton_header(host.regex_automaton(rx, True))
    assert header("(LMA(E|Q)GLYN)")["lmax"] == 8 and header("(C.{2,4}C.{3}[LIVMFYWC])")["lmax"] == 10 and header("(^MAEG$)")["lmax"] == 4
    assert header("(A|)")["start_begin"] == 1  # the empty match: accepted before the first byte


def test_pairs_groups_and_refusals():
    """several groups and pairs, bitmaps of more than one word, a serial cap, and pairs that cannot be answered"""
    a = host.regex_automaton("(A(C+|G+)T)", False)
    b = host.regex_automaton("(GATTACA)", False)
    rng = np.random.default_rng(9)
    recs = [bytes(rng.choice(list(b"ACGT"), size=int(n))) for n in rng.integers(0, 60, size=75)]
    recs[70] = b"TTGATTACATT"
    groups = [0, 70, 70, 75]
    pairs = [(0, 0), (1, 0), (0, 1), (1, 2), (2, 0), (0, 3), (0, 2)]
    got, status = host.regex_filter([a, b], recs, groups, pairs, return_status=True)
    assert status.tolist() == [0, 0, 0, 0, host.REGEX_REFUSED, host.REGEX_REFUSED, 0]
    for (p, g), res in zip(pairs, got):
        if p < 2 and g < 3:
            rx = ["(A(C+|G+)T)", "(GATTACA)"][p]
            assert res.tolist() == [len(host.regex_find_all(rx, r, False)) > 0 for r in recs[groups[g]:groups[g + 1]]]
        else:
            assert res.size == 0
    assert got[3].tolist() == [True, False, False, False, False]
    # an unbounded automaton and a serial cap: the longer record is flagged unseen; a bounded one ignores the cap
    long = [b"T" * 300, b"T" * 256, b"T" * 250 + b"ACCT"]
    assert host.regex_filter([a, b], long, [0, 3], [(0, 0), (1, 0)], max_serial=256)[0].tolist() == [True, False, True]
    assert host.regex_filter([a, b], long, [0, 3], [(0, 0), (1, 0)], max_serial=256)[1].tolist() == [False, False, False]
    # a blob cut short or with a broken header is refused, not read
    broken = bytearray(a)
    broken[4] = 0xFF
    got, status = host.regex_filter([a[:-16], bytes(broken), a], [b"ACT"], [0, 1], [(0, 0), (1, 0), (2, 0)], return_status=True)
    assert status.tolist() == [host.REGEX_REFUSED, host.REGEX_REFUSED, 0] and got[2].tolist() == [True]


def test_native_fuzz_under_sanitizers(tmp_path):
    """tests/native/regex_filter_fuzz.cpp: random patterns x random texts, the blob's interpreter against Matcher::contains and
    find_all, both strands, built with AddressSanitizer and UBSan"""
    exe = str(tmp_path / "regex_filter_fuzz")
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "regex_filter_fuzz.cpp"), os.path.join(ROOT, "tetrex_amd", "csrc", "host", "matcher.cpp")],
                   check=True, timeout=600)
    r = subprocess.run([exe, "1", "600"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "regex_filter_fuzz ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.fixture(scope="module")
def verify_selection(tmp_path_factory):
    """tests/native/verify_selection.cpp under AddressSanitizer and UBSan"""
    exe = str(tmp_path_factory.mktemp("verify_selection") / "verify_selection")
    src = os.path.join(ROOT, "tetrex_amd", "csrc", "host")
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fopenmp", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "verify_selection.cpp")] +
                   [os.path.join(src, f + ".cpp") for f in ("verify", "fasta", "matcher", "encoder", "regex_front")] + ["-lz"], check=True, timeout=900)
    return exe


@pytest.mark.parametrize("library,reduction,threads", [("peptide", 0, 1), ("peptide", 1, 3), ("dna", 0, 2)])
def test_verification_with_records_to_look_at_writes_the_same_rows(verify_selection, tmp_path, library, reduction, threads):
    """verify_batch and verify_bins with a RecordSelection made by the automata (every motif on every bin, some pairs and one
    motif left without a list, as refused pairs and too-large automata are) against the same calls without one"""
    if library == "dna":
        files = sorted(glob.glob(os.path.join(GOLDEN, "dna_example_split", "*.fa")))
        motifs = DNA_QUERIES + ["^ACG", "T$", "ACGT"]
    else:
        names, _, _ = family_library(str(tmp_path), families=3, members=3, seed=5, core=(300, 600), own=(100, 300), empty=(4,))
        files = [str(tmp_path / n) for n in names]
        motifs = PEPTIDE_QUERIES + ["^M.K", "[KR]$", "A.{15}C"]
    (tmp_path / "motifs.txt").write_text("".join(m + "\n" for m in motifs))
    r = subprocess.run([verify_selection, "1" if library == "dna" else "0", str(reduction), str(threads), str(tmp_path / "motifs.txt"), *files],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("verify_selection ok: "), r.stdout[-2000:] + r.stderr[-2000:]
    rows, listed, records = [int(x) for x in re.findall(r"\d+", r.stdout)]
    assert rows > 20 and 0 < listed < records
