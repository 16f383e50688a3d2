"""GPU parity of approximate matching for patterns of up to 4096 bytes (include/txq.h txq_edit_search_long, DESIGN.md §12 "Long
patterns"): every (distance, record, end) against tetrex_amd.host.edit_search (txh_edit_search), which tests/test_edit_cpu.py and
tests/native/edit_fuzz.cpp hold to the O(mn) table; then `tetrex search --verify` with queries of 600 .. 4200 letters on indexes
that `tetrex index` builds from generated FASTA, against the plain search filtered by that reference."""
import os
import re
import subprocess

import numpy as np
import pytest

import edit_cases
import edit_ref as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TETREX = os.path.join(ROOT, "bin", "tetrex")
# the smallest shapes at which a group size (1024 | 1025, 2048 | 2049), a word count or the score bit changes
LENGTHS = [1, 64, 65, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4032, 4033, 4095, 4096]
REFUSED = [0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFE]


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def host():
    from tetrex_amd import host as h
    return h


def _raw(case):
    patterns, records, groups, pairs, codes = case
    return [p.tobytes() for p in patterns], [r.tobytes() for r in records], groups, pairs, codes


@pytest.fixture(scope="module")
def parity_cases(host):
    """inputs and reference results of the parity test, computed once per alphabet"""
    out = {}
    for alphabet in edit_cases.ALPHABETS:
        case = _raw(edit_cases.build(LENGTHS, alphabet, seed=31 + len(alphabet), long_bytes=3000))
        out[alphabet] = (case, host.edit_search(*case, threads=8))
    return out


def _differing(got, want, pairs):
    bad = np.flatnonzero((got != want).any(axis=1))
    return [(tuple(pairs[i]), got[i].tolist(), want[i].tolist()) for i in bad[:6]], bad.size


@pytest.mark.parametrize("span", [None, "64", "16"])
@pytest.mark.parametrize("alphabet", list(edit_cases.ALPHABETS))
def test_parity_with_host(capi, parity_cases, monkeypatch, alphabet, span):
    """m on either side of every group size and word count, records of 0, 1, m - 1, m and some thousand bytes, caps 0 .. m + 5,
    four groups per pattern and a group of no records; with the default span and with spans shorter than every lead-in"""
    if span:
        monkeypatch.setenv("TXQ_EDIT_LONG_SPAN", span)
    (patterns, records, groups, pairs, codes), want = parity_cases[alphabet]
    got = capi.edit_search_long(patterns, records, groups, pairs, codes)
    assert _differing(got, want, pairs) == ([], 0)
    assert (want[:, 0] != E.NONE).sum() > len(pairs) // 3 and (want[:, 0] == E.NONE).sum() > len(pairs) // 10


@pytest.mark.parametrize("alphabet", list(edit_cases.ALPHABETS))
def test_cross_check_with_the_short_kernel(capi, alphabet):
    """the lengths both kernels take: the same answers from either"""
    case = _raw(edit_cases.build([m for m in LENGTHS if m <= capi.EDIT_MAX_PATTERN], alphabet, seed=5, long_bytes=3000))
    short, long_ = capi.edit_search(*case), capi.edit_search_long(*case)
    assert _differing(long_, short, case[3]) == ([], 0)
    assert (short[:, 0] != E.NONE).sum() > len(case[3]) // 3


@pytest.mark.parametrize("span", ["1024", None])
def test_span_boundaries(capi, host, monkeypatch, span):
    """one record of 60 000 letters; cuts of 700 and of 3000 letters with 0..3 substitutions inside, which end on, one before
    and one behind multiples of 4096 (of either span, then)"""
    if span:
        monkeypatch.setenv("TXQ_EDIT_LONG_SPAN", span)
    rng = np.random.default_rng(41)
    codes = E.letter_codes("ACGT")
    text = edit_cases.random_text(rng, "ACGT", 60_000, junk=0)
    swap = bytes.maketrans(b"ACGTacgt", b"CATGcatg")
    patterns, ends = [], []
    for m in (700, 3000):
        for k in (1, 5, 9, 14):
            for delta in (-1, 0, 1):
                end = 4096 * k + delta
                cut = bytearray(text[end - m:end].tobytes())
                for at in rng.integers(10, m - 10, size=int(rng.integers(0, 4))):
                    cut[at:at + 1] = bytes(cut[at:at + 1]).translate(swap)
                patterns.append(bytes(cut))
                ends.append(end)
    pairs = [(i, 0, 3) for i in range(len(patterns))]
    want = host.edit_search(patterns, [text.tobytes()], [0, 1], pairs, codes)
    assert want[:, 2].tolist() == ends and set(want[:, 0].tolist()) == {0, 1, 2, 3}
    got = capi.edit_search_long(patterns, [text.tobytes()], [0, 1], pairs, codes)
    assert _differing(got, want, pairs) == ([], 0)


@pytest.mark.parametrize("m", [600, 2100])
def test_no_match_across_records(capi, host, monkeypatch, m):
    rng = np.random.default_rng(43 + m)
    codes = E.letter_codes("ACGT")
    p = edit_cases.random_text(rng, "ACGT", m, junk=0).tobytes().upper()
    h = m // 2
    records = [b"", b"GGGGGGGG" + p[:h], p[h:] + b"GGGG", b"", b"####", b""]
    groups = [0, 3, 3, 6, 6]  # (group 1 and group 3 have no records)
    pairs = [(0, 0, m), (0, 0, h // 2), (0, 1, 5000), (0, 2, m), (0, 2, m - 1), (0, 3, 0), (0, 0, h), (0, 0, m + 4)]
    want = host.edit_search([p], records, groups, pairs, codes)
    # the halves of p at the end of one record and the start of the next: about m / 2 edits in either, never 0
    assert h * 3 // 4 < want[0, 0] <= h and want[0, 1] == 1 and want[1].tolist() == [E.NONE] * 3 and want[2].tolist() == [E.NONE] * 3
    # nothing matches in records 3 .. 5: distance m, first reached by the empty match in the empty record in front
    assert want[3].tolist() == [m, 3, 0] and want[4].tolist() == [E.NONE] * 3
    for span in (None, "16"):
        if span:
            monkeypatch.setenv("TXQ_EDIT_LONG_SPAN", span)
        got = capi.edit_search_long([p], records, groups, pairs, codes)
        assert _differing(got, want, pairs) == ([], 0), span


@pytest.mark.parametrize("m", [600, 2100])
def test_empty_records_between_records(capi, host, monkeypatch, m):
    """[A, "", B] and [A, "", "", B]: the reset that leaves A travels over the empty records into B, and the record index and
    the end position that the scoring lane reports count them; with the default span and with spans of 16 bytes"""
    rng = np.random.default_rng(47 + m)
    codes = E.letter_codes("ACGT")
    p = edit_cases.random_text(rng, "ACGT", m, junk=0).tobytes().upper()
    mid = m // 2
    one_edit = p[:mid] + p[mid:mid + 1].translate(bytes.maketrans(b"ACGT", b"CATG")) + p[mid + 1:]
    records = [b"GG" + one_edit + b"GG", b"", b"TTT" + p + b"TT",                   # group 0: the exact copy behind one empty record
               b"GG" + p + b"G", b"", b"", b"C" + p + b"CC",                        # group 1: exact in the first and in the last
               b"G" * (m + 5), b"", b"", b"G" + p[:m - 4],                          # group 2: the best hit behind two empty records
               b"", b"", p, b"", b"", b"", one_edit + p, b""]                       # group 3: empties in front, between and behind
    groups = [0, 3, 7, 11, 19]
    pairs = [(0, g, e) for g in range(4) for e in (0, 1, 3, 4, m)]
    want = host.edit_search([p], records, groups, pairs, codes)
    by = {(g, e): want[i].tolist() for i, (_, g, e) in enumerate(pairs)}
    assert by[0, 0] == [0, 2, 3 + m] and by[0, 1] == [0, 2, 3 + m]           # B, although A is within the cap
    assert by[1, 0] == [0, 3, 2 + m]                                          # the tie: the lower record
    assert by[2, 3] == [E.NONE] * 3 and by[2, 4] == [4, 10, m - 3]            # p[:m - 4] in B: 4 letters missing
    assert by[3, 0] == [0, 13, m] and by[3, m] == [0, 13, m]
    for span in (None, "16"):
        if span:
            monkeypatch.setenv("TXQ_EDIT_LONG_SPAN", span)
        got = capi.edit_search_long([p], records, groups, pairs, codes)
        assert _differing(got, want, pairs) == ([], 0), span


def _device_call(capi, t, shapes, out, work, stream):
    po, pat, ro, txt, go, pr = shapes
    capi.check(capi.lib().txq_edit_search_long_device(t[0].data_ptr(), t[1].data_ptr(), po.size - 1, pat.size, t[2].data_ptr(), t[3].data_ptr(),
                                                       ro.size - 1, txt.size, t[4].data_ptr(), go.size - 1, t[5].data_ptr(), pr.shape[0],
                                                       t[6].data_ptr(), out.data_ptr(), work.data_ptr(), stream))


def test_device_entry_point_on_a_stream(capi, host):
    """txq_edit_search_long_device on torch's buffers and a stream of torch's making; nothing is waited for inside the call"""
    import torch
    case = _raw(edit_cases.build([5, 300, 700, 1100, 2100], "peptide", seed=3, long_bytes=900))
    want = host.edit_search(*case, threads=8)
    pat, po, txt, ro, go, pr, cd = capi.edit_arrays(*case)
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).to(dev) for x in (pat, po, txt, ro, go, pr, cd)]
    out = torch.zeros(pr.shape[0] * 12, dtype=torch.uint8, device=dev)
    work = torch.empty(capi.edit_long_workspace(pr.shape[0]) // 8, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        _device_call(capi, t, (po, pat, ro, txt, go, pr), out, work, stream.cuda_stream)
    stream.synchronize()
    got = out.cpu().numpy().view(np.uint32).reshape(-1, 3)
    assert _differing(got, want, case[3]) == ([], 0)


def test_text_that_is_not_16_byte_aligned(capi, host, monkeypatch):
    """txq_edit_search_long_device on a text that begins 1, 7 and 15 bytes behind a 16-byte boundary: records of 700, 0 and 1500
    bytes, patterns of 70 and 1100 bytes (groups of 16 and of 32 lanes), spans of 16 bytes.  The 16-byte blocks at either end of
    the text are assembled from byte loads; the bytes around the text are letters, so a block that took them in would change
    the answer."""
    import torch
    monkeypatch.setenv("TXQ_EDIT_LONG_SPAN", "16")
    rng = np.random.default_rng(17)
    codes = E.letter_codes("ACGT")
    text = edit_cases.random_text(rng, "ACGT", 2200, junk=0)
    records = [text[:700].tobytes(), b"", text[700:].tobytes()]
    swap = bytes.maketrans(b"ACGTacgt", b"CATGcatg")
    cut70, cut1100 = text[0:70].tobytes(), text[1100:2200].tobytes()  # the text's first bytes; its last ones
    patterns = [cut70[:3] + cut70[3:4].translate(swap) + cut70[4:],
                cut1100[:9] + cut1100[9:10].translate(swap) + cut1100[10:640] + cut1100[640:641].translate(swap) + cut1100[641:]]
    groups, pairs = [0, 3], [(0, 0, 2), (1, 0, 2)]
    want = host.edit_search(patterns, records, groups, pairs, codes)
    assert want.tolist() == [[1, 0, 70], [2, 2, 1500]]
    pat, po, txt, ro, go, pr, cd = capi.edit_arrays(patterns, records, groups, pairs, codes)
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).to(dev) for x in (pat, po, txt, ro, go, pr, cd)]
    work = torch.empty(capi.edit_long_workspace(pr.shape[0]) // 8, dtype=torch.int64, device=dev)
    results = {}
    for at in (0, 1, 7, 15):
        around = torch.full((at + txt.size + 33,), ord("A"), dtype=torch.uint8, device=dev)
        shifted = around[at:at + txt.size]
        shifted.copy_(t[2])
        assert shifted.data_ptr() % 16 == at
        out = torch.zeros(pr.shape[0] * 12, dtype=torch.uint8, device=dev)
        _device_call(capi, [t[0], t[1], shifted] + t[3:], (po, pat, ro, txt, go, pr), out, work, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        results[at] = out.cpu().numpy().view(np.uint32).reshape(-1, 3)
    for at in (1, 7, 15):
        assert results[at].tolist() == results[0].tolist(), at
    assert _differing(results[0], want, pairs) == ([], 0)


def test_refusals_leave_the_library_usable(capi, host):
    codes = E.letter_codes("ACGT")
    records, groups = ["ACGTACGT", "TTTT"], [0, 1, 2]
    ok = (["ACGT", "A" * 4096], [(0, 0, 1), (1, 1, 5000)])
    want_ok = host.edit_search(ok[0], records, groups, ok[1], codes).tolist()
    assert want_ok == [[0, 0, 4], [4096, 1, 0]]
    for patterns, pairs in ((["ACGT", ""], [(0, 0, 1), (1, 0, 1)]),          # m = 0
                            (["ACGT", "A" * 4097], [(1, 0, 1)]),            # m = 4097
                            (["ACGT"], [(0, 0, 1), (1, 0, 1)]),             # a pattern out of range
                            (["ACGT"], [(0, 2, 1)]),                        # a group out of range
                            (["ACGT"], [(0xFFFFFFFF, 0xFFFFFFFF, 1)])):
        with pytest.raises(capi.TxqError) as e:
            capi.edit_search_long(patterns, records, groups, pairs, codes)
        assert e.value.code == -1
        got = capi.edit_search_long(ok[0], records, groups, ok[1], codes)
        assert got.tolist() == want_ok, (patterns, pairs)
    # the device entry point cannot read its buffers before it launches: the kernels refuse such a pair, and only it
    patterns, pairs = ["ACGT", "A" * 4097, "", "T" * 600], [(0, 0, 1), (1, 0, 5000), (2, 0, 5), (7, 0, 1), (0, 9, 1), (0, 1, 4), (3, 1, 600)]
    pat, po, txt, ro, go, pr, cd = capi.edit_arrays(patterns, records, groups, pairs, codes)
    bufs = [capi.DeviceBuffer.from_numpy(x) for x in (pat, po, txt, ro, go, pr, cd)]
    out = capi.DeviceBuffer(len(pairs) * 12)
    work = capi.DeviceBuffer(capi.edit_long_workspace(len(pairs)))
    bufs.append(work)
    try:
        assert capi.lib().txq_edit_search_long_device(bufs[0].ptr, bufs[1].ptr, 4, pat.size, bufs[2].ptr, bufs[3].ptr, 2, txt.size, bufs[4].ptr, 2,
                                                      bufs[5].ptr, len(pairs), bufs[6].ptr, out.ptr, None, None) == -1  # no workspace
        capi.check(capi.lib().txq_edit_search_long_device(bufs[0].ptr, bufs[1].ptr, 4, pat.size, bufs[2].ptr, bufs[3].ptr, 2, txt.size, bufs[4].ptr, 2,
                                                           bufs[5].ptr, len(pairs), bufs[6].ptr, out.ptr, work.ptr, None))
        capi.synchronize()
        got = out.to_numpy(np.uint32, (len(pairs), 3))
    finally:
        for b in bufs + [out]:
            b.free()
    valid = host.edit_search(["ACGT", "T" * 600], records, groups, [(0, 0, 1), (0, 1, 4), (1, 1, 600)], codes).tolist()
    assert valid == [[0, 0, 4], [3, 1, 1], [596, 1, 4]]
    assert got.tolist() == [valid[0], REFUSED, REFUSED, REFUSED, REFUSED, valid[1], valid[2]]
    got = capi.edit_search_long(ok[0], records, groups, ok[1], codes)
    assert got.tolist() == want_ok


# ---- the command line ---------------------------------------------------------------------------------------------------

AMINO = "ACDEFGHIKLMNPQRSTVWY"
LIBRARIES = {"peptide": (AMINO, 6, [], False), "dna": ("ACGT", 16, ["-n"], True)}  # name: (residues, k, index flags, dna)
EDITS, BINS = 3, 5
QUERY_LENGTHS = [600, 1500, 4000]


def _run(*args, env=None):
    r = subprocess.run([TETREX, *args], capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    return r.returncode, r.stdout, r.stderr


def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _generate(name):
    """the library's records and its queries (name, source bin, letters, edits applied or None for a decoy), and the reference:
    every query (on DNA both strands) against every bin, cap EDITS"""
    from tetrex_amd import host
    res, _, _, dna = LIBRARIES[name]
    rng = np.random.default_rng(200 + len(name))
    seqs = [["".join(rng.choice(list(res), size=n)) for n in (5000, int(rng.integers(150, 400)))] for _ in range(BINS)]
    queries = []
    for qlen in QUERY_LENGTHS + [4200]:
        for q in range(1 if qlen == 4200 else 4):
            b = int(rng.integers(0, BINS))
            at = int(rng.integers(0, 5000 - qlen))
            cut = seqs[b][0][at:at + qlen]
            if q < 3:
                e = 1 if qlen == 4200 else q if q < 2 else EDITS
                s = edit_cases.edited(rng, res, np.frombuffer(cut.encode(), dtype=np.uint8), e).tobytes().decode().upper()
            else:
                e, mid = None, qlen // 2
                s = cut[:mid] + "".join(res[(res.index(c) + 1) % len(res)] for c in cut[mid:mid + 5]) + cut[mid + 5:]
            if dna and q % 2:
                s = _revcomp(s)
            queries.append(("q%d_%d_b%d" % (qlen, q, b), b, s, e))
    codes = E.letter_codes("ACGT", {"U": 3}) if dna else E.letter_codes("ABCDEFGHIJKLMNOPQRSTUVWXYZ")
    patterns = [s for _, _, s, _ in queries] + ([_revcomp(s) for _, _, s, _ in queries] if dna else [])
    records = [r for recs in seqs for r in recs]
    pairs = [(p, b, EDITS) for p in range(len(patterns)) for b in range(BINS)]
    ref = host.edit_search(patterns, records, list(range(0, 2 * BINS + 1, 2)), pairs, codes, threads=8).reshape(len(patterns), BINS, 3)
    return seqs, queries, ref


@pytest.fixture(scope="module")
def cli_setup(tmp_path_factory):
    """For each library: 5 bins of two records (5000 letters and a few hundred), a flat index, and the queries: for each of
    600, 1500 and 4000 letters three cut from the bins with 0, 1 and 3 edits (on DNA every other one reverse-complemented) and one
    decoy cut the same way and given five adjacent substitutions; and one of 4200 letters with one edit (answered on the host)."""
    root = tmp_path_factory.mktemp("verify_long_cli")
    out = {}
    for name, (res, k, flags, dna) in LIBRARIES.items():
        seqs, queries, ref = _generate(name)
        d = root / name
        d.mkdir()
        files = []
        for b, recs in enumerate(seqs):
            p = d / ("bin%02d.fa" % b)
            p.write_text("".join(">b%d_%d description\n%s\n" % (b, i, r) for i, r in enumerate(recs)))
            files.append(os.path.abspath(str(p)))
        qf = d / "queries.fa"
        qf.write_text("".join(">%s some comment\n%s\n" % (n, s) for n, _, s, _ in queries))
        rc, so, se = _run("index", "-k", str(k), *flags, "-i", str(d / "flat"), *files)
        assert rc == 0 and os.path.exists(d / "flat.ibf"), se
        out[name] = dict(files=files, queries=queries, qfile=str(qf), index=str(d / "flat.ibf"), dna=dna, ref=ref,
                         names=[["b%d_%d" % (b, i) for i in range(2)] for b in range(BINS)])
    return out


def _reference_columns(setup, q, b):
    """the columns the reference gives for query q in bin b, or None where it is not within EDITS"""
    n = len(setup["queries"])
    best = None
    for strand in ((0, 1) if setup["dna"] else (0,)):
        d, r, j = (int(x) for x in setup["ref"][q + strand * n, b])
        if d != E.NONE and (best is None or d < best[0]):
            best = (d, setup["names"][b][r - 2 * b], j, "+-"[strand])
    if best is None:
        return None
    cols = (str(best[0]), best[1], str(best[2]))
    return cols + (best[3],) if setup["dna"] else cols


def _routes(stderr):
    m = re.search(r"verify routes: device (\d+), device-long (\d+), host (\d+)", stderr)
    assert m, stderr
    return tuple(int(x) for x in m.groups())


@pytest.mark.parametrize("library", list(LIBRARIES))
def test_cli_search_verify_long_queries(cli_setup, library):
    setup = cli_setup[library]
    index_of = {n: i for i, (n, _, _, _) in enumerate(setup["queries"])}
    length_of = {n: len(s) for n, _, s, _ in setup["queries"]}
    bin_of = {p: b for b, p in enumerate(setup["files"])}
    args = ("search", "-e", str(EDITS), "--counts")
    rc, so, se = _run(*args, setup["index"], setup["qfile"])
    assert rc == 0, se
    plain = [tuple(line.split("\t")) for line in so.splitlines()]
    want = []
    for row in plain:
        cols = _reference_columns(setup, index_of[row[0]], bin_of[row[1]])
        if cols is not None:
            want.append(row + cols)
    n_4200 = sum(1 for r in plain if length_of[r[0]] > 4096)  # (the query of 4200 letters, give or take its edit)
    n_long = len(plain) - n_4200
    assert all(512 < n <= 4096 for n in length_of.values() if n < 4190)
    assert n_4200 >= 1 and n_long >= 12
    outputs = {}
    for label, env in (("default", {}), ("host", {"TETREX_VERIFY_LONG": "0"}), ("span64", {"TXQ_EDIT_LONG_SPAN": "64"})):
        rc, so, se = _run(*args, "--verify", "-v", setup["index"], setup["qfile"], env=dict(env, TETREX_TRACE="1"))
        assert rc == 0, se
        outputs[label] = so
        assert "Verified: %d of %d candidate pairs" % (len(want), len(plain)) in se, label
        assert _routes(se) == ((0, 0, len(plain)) if label == "host" else (0, n_long, n_4200)), label
    assert outputs["host"] == outputs["default"] and outputs["span64"] == outputs["default"]
    got = [tuple(line.split("\t")) for line in outputs["default"].splitlines()]
    assert got == want, (library, [x for x in got if x not in want][:3], [x for x in want if x not in got][:3])
    # the conditions that keep this test from passing on nothing
    confirmed = {(r[0], r[1]): int(r[3]) for r in got}
    assert len(plain) - len(got) >= 3 and len(got) >= 10, (library, len(plain), len(got))
    for n, b, _, e in setup["queries"]:
        if e is not None:  # the guarantee of -e survives: confirmed in its source bin, no further away than it was edited
            assert confirmed.get((n, setup["files"][b]), 99) <= e, (library, n)
        else:
            assert (n, setup["files"][b]) not in confirmed and any(r[0] == n and r[1] == setup["files"][b] for r in plain), (library, n)
    if setup["dna"]:
        assert {r[6] for r in got} == {"+", "-"}
