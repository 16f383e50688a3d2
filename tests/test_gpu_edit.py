"""GPU parity of approximate matching by edit distance (include/txq.h txq_edit_search): every (distance,
record, end) against the dynamic program restated in tests/edit_ref.py; then `tetrex search --verify` on indexes that
`tetrex index` builds from generated FASTA, against the plain search filtered by that reference."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import edit_cases
import edit_ref as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TETREX = os.path.join(ROOT, "bin", "tetrex")
LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512]


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def parity_cases():
    """inputs and reference results of the parity test, computed once per alphabet"""
    out = {}
    for alphabet in edit_cases.ALPHABETS:
        case = edit_cases.build(LENGTHS, alphabet, seed=7 + len(alphabet), long_bytes=4000)
        out[alphabet] = (case, E.search(*case))
    return out


def _differing(got, want, pairs):
    bad = np.flatnonzero((got != want).any(axis=1))
    return [(tuple(pairs[i]), got[i].tolist(), want[i].tolist()) for i in bad[:6]], bad.size


@pytest.mark.parametrize("chunk", [None, "64", "16"])
@pytest.mark.parametrize("alphabet", list(edit_cases.ALPHABETS))
def test_parity_with_reference(capi, parity_cases, monkeypatch, alphabet, chunk):
    """m on either side of every word count, records of 0, 1, m - 1, m and some thousand bytes, caps 0 .. m + 5, three groups
    per pattern and a group of no records; with the default chunk and with chunks shorter than the patterns"""
    if chunk:
        monkeypatch.setenv("TXQ_EDIT_CHUNK", chunk)
    (patterns, records, groups, pairs, codes), want = parity_cases[alphabet]
    got = capi.edit_search([p.tobytes() for p in patterns], [r.tobytes() for r in records], groups, pairs, codes)
    assert _differing(got, want, pairs) == ([], 0)
    assert (want[:, 0] != E.NONE).sum() > len(pairs) // 3 and (want[:, 0] == E.NONE).sum() > len(pairs) // 10


def _edited_cuts(rng, text, starts, m, letters):
    return [edit_cases.edited(rng, letters, text[s:s + m], int(rng.integers(0, 4))) for s in starts]


def test_chunk_boundaries_small_chunks(capi, monkeypatch):
    """TXQ_EDIT_CHUNK=64: an 8192-byte record is 128 lane chunks in two units; 4096 patterns of (about) 32 bytes cut at every
    start 0 .. 4095 with 0..3 edits, cap 3: matches end on, just before and just behind every chunk boundary there"""
    monkeypatch.setenv("TXQ_EDIT_CHUNK", "64")
    rng = np.random.default_rng(11)
    codes = E.letter_codes("ACGT")
    text = edit_cases.random_text(rng, "ACGT", 8192, junk=0)
    patterns = _edited_cuts(rng, text, range(4096), 32, "ACGT")
    pairs = [(i, 0, 3) for i in range(4096)]
    want = E.search(patterns, [text], [0, 1], pairs, codes)
    got = capi.edit_search([p.tobytes() for p in patterns], [text.tobytes()], [0, 1], pairs, codes)
    assert _differing(got, want, pairs) == ([], 0)
    assert (want[:, 0] != E.NONE).all() and len(set(want[:, 0].tolist())) == 4


def test_chunk_boundaries_default_chunk(capi):
    """the default chunk: one record of 300 000 bytes (several units of 64 chunks), 64 patterns from all over it"""
    rng = np.random.default_rng(12)
    codes = E.letter_codes("ACGT")
    text = edit_cases.random_text(rng, "ACGT", 300_000, junk=0)
    starts = [int(s) for s in rng.integers(0, 300_000 - 40, size=60)] + [0, 511, 512, 300_000 - 32]
    patterns = _edited_cuts(rng, text, starts, 32, "ACGT")
    pairs = [(i, 0, 3) for i in range(64)]
    want = E.search(patterns, [text], [0, 1], pairs, codes)
    got = capi.edit_search([p.tobytes() for p in patterns], [text.tobytes()], [0, 1], pairs, codes)
    assert _differing(got, want, pairs) == ([], 0)
    assert (want[:, 0] != E.NONE).sum() >= 60


def test_no_match_across_records(capi, monkeypatch):
    codes = E.letter_codes("ACGT")
    p = "ACGTTGCAAGGCTTAC"
    records = ["", "GGGGGGGG" + p[:8], p[8:] + "GGGG", "", "####", ""]
    groups = [0, 3, 3, 6, 6]  # (group 1 and group 3 have no records)
    pairs = [(0, 0, 16), (0, 0, 7), (0, 1, 100), (0, 2, 16), (0, 2, 15), (0, 3, 0), (0, 0, 8), (0, 0, 20)]
    want = E.search([p], records, groups, pairs, codes)
    # the halves of p at the end of one record and the start of the next: 8 edits in either, the lower record wins
    assert want[0].tolist() == [8, 1, 16] and want[1].tolist() == [E.NONE] * 3 and want[2].tolist() == [E.NONE] * 3
    # nothing matches in records 3 .. 5: distance m, first reached by the empty match in the empty record in front
    assert want[3].tolist() == [16, 3, 0] and want[4].tolist() == [E.NONE] * 3
    for chunk in (None, "16"):
        if chunk:
            monkeypatch.setenv("TXQ_EDIT_CHUNK", chunk)
        got = capi.edit_search([p], records, groups, pairs, codes)
        assert _differing(got, want, pairs) == ([], 0)
        assert got[0, 0] != 0


def test_empty_records_between_records(capi, monkeypatch):
    """[A, "", B] and [A, "", "", B]: a lane that leaves A steps over the empty records into B, and the record index and the
    end position it reports count them.  The best hit in B; a tie of A and B (A wins); with the default chunk, where one
    lane walks the whole group, and with chunks of 16 bytes, where a chunk begins in every part of every record"""
    codes = E.letter_codes("ACGT")
    p = "ACGTTGCAAGGCTTAC"
    one_edit = p[:7] + "T" + p[8:]
    records = ["GG" + one_edit + "GG", "", "TTT" + p + "TT",          # group 0: the exact copy behind one empty record
               "GG" + p + "G", "", "", "C" + p + "CC",                # group 1: exact in the first and in the last
               "GGGGGGGGGGGGGGGGGGGGG", "", "", "G" + p[:12],         # group 2: the best hit behind two empty records
               "", "", p, "", "", "", one_edit + p, ""]               # group 3: empties in front, between and behind
    groups = [0, 3, 7, 11, 19]
    pairs = [(0, g, e) for g in range(4) for e in (0, 1, 3, 4, 16)]
    want = E.search([p], records, groups, pairs, codes)
    by = {(g, e): want[i].tolist() for i, (_, g, e) in enumerate(pairs)}
    assert by[0, 0] == [0, 2, 19] and by[0, 1] == [0, 2, 19]           # B, although A is within the cap
    assert by[1, 0] == [0, 3, 18]                                       # the tie: the lower record
    assert by[2, 3] == [E.NONE] * 3 and by[2, 4] == [4, 10, 13]         # p[:12] in B: 4 letters missing
    assert by[3, 0] == [0, 13, 16] and by[3, 16] == [0, 13, 16]
    for chunk in (None, "16"):
        if chunk:
            monkeypatch.setenv("TXQ_EDIT_CHUNK", chunk)
        got = capi.edit_search([p], records, groups, pairs, codes)
        assert _differing(got, want, pairs) == ([], 0), chunk


def test_device_entry_point_on_a_stream(capi):
    """txq_edit_search_device on torch's buffers and a stream of torch's making; nothing is waited for inside the call"""
    import torch
    rng = np.random.default_rng(13)
    codes = E.letter_codes(edit_cases.ALPHABETS["peptide"])
    patterns, records, groups, pairs, _ = edit_cases.build([5, 70, 200, 300], "peptide", seed=3, long_bytes=900)
    want = E.search(patterns, records, groups, pairs, codes)
    pat, po, txt, ro, go, pr, cd = capi.edit_arrays([p.tobytes() for p in patterns], [r.tobytes() for r in records], groups, pairs, codes)
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).to(dev) for x in (pat, po, txt, ro, go, pr, cd)]
    out = torch.zeros(pr.shape[0] * 12, dtype=torch.uint8, device=dev)
    work = torch.empty(capi.edit_workspace_bytes(pr.shape[0]) // 8, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        capi.check(capi.lib().txq_edit_search_device(t[0].data_ptr(), t[1].data_ptr(), po.size - 1, pat.size, t[2].data_ptr(), t[3].data_ptr(),
                                                      ro.size - 1, txt.size, t[4].data_ptr(), go.size - 1, t[5].data_ptr(), pr.shape[0],
                                                      t[6].data_ptr(), out.data_ptr(), work.data_ptr(), stream.cuda_stream))
    stream.synchronize()
    got = out.cpu().numpy().view(np.uint32).reshape(-1, 3)
    assert _differing(got, want, pairs) == ([], 0)
    del rng


def test_text_that_is_not_16_byte_aligned(capi, monkeypatch):
    """txq_edit_search_device on a text that begins 1, 7 and 15 bytes behind a 16-byte boundary: records of 40, 0 and 150 bytes,
    patterns of 8 and 70 bytes (one and two words), chunks of 16 bytes.  The 16-byte blocks at either end of the text are
    assembled from byte loads; the bytes around the text are letters, so a block that took them in would change the answer."""
    import torch
    from tetrex_amd import host
    monkeypatch.setenv("TXQ_EDIT_CHUNK", "16")
    rng = np.random.default_rng(17)
    codes = E.letter_codes("ACGT")
    text = edit_cases.random_text(rng, "ACGT", 190, junk=0)
    records = [text[:40].tobytes(), b"", text[40:].tobytes()]
    swap = bytes.maketrans(b"ACGTacgt", b"CATGcatg")
    cut8, cut70 = text[20:28].tobytes(), text[100:170].tobytes()  # from the first record and from the last, one and two substitutions
    patterns = [cut8[:3] + cut8[3:4].translate(swap) + cut8[4:], cut70[:9] + cut70[9:10].translate(swap) + cut70[10:40] + cut70[40:41].translate(swap) + cut70[41:]]
    groups, pairs = [0, 3], [(0, 0, 2), (1, 0, 2)]
    want = E.search(patterns, records, groups, pairs, codes)
    assert want.tolist() == [[1, 0, 28], [2, 2, 130]]
    pat, po, txt, ro, go, pr, cd = capi.edit_arrays(patterns, records, groups, pairs, codes)
    assert np.array_equal(host.edit_search((pat, po), (txt, ro), go, pr, cd), want)
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).to(dev) for x in (pat, po, txt, ro, go, pr, cd)]
    work = torch.empty(capi.edit_workspace_bytes(pr.shape[0]) // 8, dtype=torch.int64, device=dev)
    results = {}
    for at in (0, 1, 7, 15):
        around = torch.full((at + txt.size + 33,), ord("A"), dtype=torch.uint8, device=dev)
        shifted = around[at:at + txt.size]
        shifted.copy_(t[2])
        assert shifted.data_ptr() % 16 == at
        out = torch.zeros(pr.shape[0] * 12, dtype=torch.uint8, device=dev)
        capi.check(capi.lib().txq_edit_search_device(t[0].data_ptr(), t[1].data_ptr(), po.size - 1, pat.size, shifted.data_ptr(), t[3].data_ptr(),
                                                      ro.size - 1, txt.size, t[4].data_ptr(), go.size - 1, t[5].data_ptr(), pr.shape[0],
                                                      t[6].data_ptr(), out.data_ptr(), work.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize(dev)
        results[at] = out.cpu().numpy().view(np.uint32).reshape(-1, 3)
    for at in (1, 7, 15):
        assert results[at].tolist() == results[0].tolist(), at
    assert _differing(results[0], want, pairs) == ([], 0)


def test_refusals_leave_the_library_usable(capi):
    codes = E.letter_codes("ACGT")
    records, groups = ["ACGTACGT", "TTTT"], [0, 1, 2]
    ok = (["ACGT", "A" * 512], [(0, 0, 1), (1, 1, 600)])
    want_ok = E.search(ok[0], records, groups, ok[1], codes).tolist()
    for patterns, pairs in ((["ACGT", ""], [(0, 0, 1), (1, 0, 1)]),          # m = 0
                            (["ACGT", "A" * 513], [(1, 0, 1)]),             # m = 513
                            (["ACGT"], [(0, 0, 1), (1, 0, 1)]),             # a pattern out of range
                            (["ACGT"], [(0, 2, 1)]),                        # a group out of range
                            (["ACGT"], [(0xFFFFFFFF, 0xFFFFFFFF, 1)])):
        with pytest.raises(capi.TxqError) as e:
            capi.edit_search(patterns, records, groups, pairs, codes)
        assert e.value.code == -1
        got = capi.edit_search(ok[0], records, groups, ok[1], codes)
        assert got.tolist() == want_ok, (patterns, pairs)
    # the device entry point cannot read its buffers before it launches: the kernels refuse such a pair, and only it
    patterns, pairs = ["ACGT", "A" * 513, ""], [(0, 0, 1), (1, 0, 600), (2, 0, 5), (7, 0, 1), (0, 9, 1), (0, 1, 4)]
    pat, po, txt, ro, go, pr, cd = capi.edit_arrays(patterns, records, groups, pairs, codes)
    bufs = [capi.DeviceBuffer.from_numpy(x if x.size else np.zeros(1, x.dtype)) for x in (pat, po, txt, ro, go, pr, cd)]
    out = capi.DeviceBuffer(len(pairs) * 12)
    work = capi.DeviceBuffer(capi.edit_workspace_bytes(len(pairs)))
    bufs.append(work)
    try:
        assert capi.lib().txq_edit_search_device(bufs[0].ptr, bufs[1].ptr, 3, pat.size, bufs[2].ptr, bufs[3].ptr, 2, txt.size, bufs[4].ptr, 2,
                                                 bufs[5].ptr, len(pairs), bufs[6].ptr, out.ptr, None, None) == -1  # no workspace
        capi.check(capi.lib().txq_edit_search_device(bufs[0].ptr, bufs[1].ptr, 3, pat.size, bufs[2].ptr, bufs[3].ptr, 2, txt.size, bufs[4].ptr, 2,
                                                      bufs[5].ptr, len(pairs), bufs[6].ptr, out.ptr, work.ptr, None))
        capi.synchronize()
        got = out.to_numpy(np.uint32, (len(pairs), 3))
    finally:
        for b in bufs + [out]:
            b.free()
    refused = [0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFE]
    valid = E.search(["ACGT"], records, groups, [pairs[0], pairs[5]], codes).tolist()
    assert valid == [[0, 0, 4], [3, 1, 1]]
    assert got.tolist() == [valid[0], refused, refused, refused, refused, valid[1]]


# ---- the command line ---------------------------------------------------------------------------------------------------

AMINO = "ACDEFGHIKLMNPQRSTVWY"
ALPHABETS = {  # name: (residues, k, index flags, dna, query length)
    "peptide": (AMINO, 6, [], False, 60),
    "murphy": (AMINO, 5, ["-r", "murphy"], False, 60),
    "dna": ("ACGT", 16, ["-n"], True, 150),
}
LAYOUTS = {"flat": ["-i"], "default": [], "sized": ["--layout", "sized"]}
EDITS, BINS = 2, 24


def _run(*args):
    r = subprocess.run([TETREX, *args], capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTUacgtu", "TGCAAtgcaa"))


@pytest.fixture(scope="module")
def cli_setup(tmp_path_factory):
    """For each alphabet: 24 bins of two records (every third file gzip), its three indexes, and the queries: 30 cut from
    the bins with 0..2 edits (on DNA every other one reverse-complemented, some in lower case or with U for T), 6 decoys
    cut the same way and given four adjacent substitutions, and one of 600 letters with one edit (answered on the host)."""
    root = tmp_path_factory.mktemp("verify_cli")
    out = {}
    for name, (res, k, flags, dna, qlen) in ALPHABETS.items():
        rng = np.random.default_rng(100 + len(name))
        d = root / name
        d.mkdir()
        files, seqs = [], []
        for b in range(BINS):
            lens = [int(rng.integers(150, 400)) * (3 if dna else 1) for _ in range(2)]
            if b == 5:
                lens[1] = 2000
            recs = ["".join(rng.choice(list(res), size=n)) for n in lens]
            seqs.append(recs)
            text = "".join(">b%d_%d description\n%s\n" % (b, i, r) for i, r in enumerate(recs))
            p = d / ("bin%02d.fa" % b + (".gz" if b % 3 == 0 else ""))
            if b % 3 == 0:
                with gzip.open(p, "wt") as f:
                    f.write(text)
            else:
                p.write_text(text)
            files.append(os.path.abspath(str(p)))
        queries = []  # (name, source bin, letters, edits applied or None for a decoy)
        for q in range(36):
            b = int(rng.integers(0, BINS))
            rec = seqs[b][int(rng.integers(0, 2))]
            at = int(rng.integers(0, len(rec) - qlen))
            cut = rec[at:at + qlen]
            if q < 30:
                e = int(rng.integers(0, EDITS + 1))
                s = edit_cases.edited(rng, res, np.frombuffer(cut.encode(), dtype=np.uint8), e).tobytes().decode().upper()
            else:
                e, mid = None, qlen // 2
                s = cut[:mid] + "".join(res[(res.index(c) + 1 + int(rng.integers(0, len(res) - 1))) % len(res)] for c in cut[mid:mid + 4]) + cut[mid + 4:]
            if dna and q % 2:
                s = _revcomp(s)
            if dna and q % 5 == 0:
                s = s.lower()
            if dna and q % 7 == 0:
                s = s.replace("T", "U").replace("t", "u")
            queries.append(("q%d_b%d" % (q, b), b, s, e))
        cut = seqs[5][1][700:1300]
        queries.append(("long_b5", 5, cut[:300] + cut[301:], 1))
        qf = d / "queries.fa"
        qf.write_text("".join(">%s some comment\n%s\n" % (n, s) for n, _, s, _ in queries))
        indexes = {}
        for lay, lflags in LAYOUTS.items():
            rc, so, se = _run("index", "-k", str(k), *flags, *lflags, str(d / lay), *files)
            assert rc == 0 and os.path.exists(d / (lay + ".ibf")), se
            indexes[lay] = str(d / (lay + ".ibf"))
        # the reference, once: every query (on DNA both strands) against every bin, cap EDITS
        codes = E.letter_codes("ACGT", {"U": 3}) if dna else E.letter_codes("ABCDEFGHIJKLMNOPQRSTUVWXYZ")
        patterns = [s for _, _, s, _ in queries] + ([_revcomp(s) for _, _, s, _ in queries] if dna else [])
        records = [r for recs in seqs for r in recs]
        pairs = [(p, b, EDITS) for p in range(len(patterns)) for b in range(BINS)]
        ref = E.search(patterns, records, list(range(0, 2 * BINS + 1, 2)), pairs, codes).reshape(len(patterns), BINS, 3)
        # decoys are at distance 3 or more from every bin (their least distance without the cap)
        decoys = [x for _, _, s, e in queries if e is None for x in ([s, _revcomp(s)] if dna else [s])]
        far = E.search(decoys, records, list(range(0, 2 * BINS + 1, 2)), [(p, b, 10 ** 6) for p in range(len(decoys)) for b in range(BINS)], codes)
        assert len(decoys) == (12 if dna else 6) and far[:, 0].min() >= 3
        out[name] = dict(files=files, queries=queries, qfile=str(qf), indexes=indexes, dna=dna, ref=ref,
                         names=[["b%d_%d" % (b, i) for i in range(2)] for b in range(BINS)])
    return out


def _reference_columns(setup, q, b):
    """the four columns the reference gives for query q in bin b, or None where it is not within EDITS"""
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


@pytest.mark.parametrize("alphabet", list(ALPHABETS))
def test_cli_search_verify(cli_setup, tmp_path, alphabet):
    setup = cli_setup[alphabet]
    index_of = {n: i for i, (n, _, _, _) in enumerate(setup["queries"])}
    bin_of = {p: b for b, p in enumerate(setup["files"])}
    for layout, path in setup["indexes"].items():
        rc, so, se = _run("search", "-e", str(EDITS), "--counts", path, setup["qfile"])
        assert rc == 0, se
        plain = [tuple(line.split("\t")) for line in so.splitlines()]
        rc, so, se = _run("search", "-e", str(EDITS), "--counts", "--verify", "-v", path, setup["qfile"])
        assert rc == 0, se
        got = [tuple(line.split("\t")) for line in so.splitlines()]
        want = []
        for row in plain:
            cols = _reference_columns(setup, index_of[row[0]], bin_of[row[1]])
            if cols is not None:
                want.append(row + cols)
        assert got == want, (alphabet, layout, [x for x in got if x not in want][:3], [x for x in want if x not in got][:3])
        assert "Verified: %d of %d candidate pairs" % (len(want), len(plain)) in se
        # the conditions that keep this test from passing on nothing
        assert len(plain) - len(got) >= 5 and len(got) >= 30, (alphabet, layout, len(plain), len(got))
        confirmed = {(r[0], r[1]): int(r[3]) for r in got}
        for n, b, _, e in setup["queries"]:
            if e is not None:  # the guarantee of -e survives: confirmed in its source bin, no further away than it was edited
                assert confirmed.get((n, setup["files"][b]), 99) <= e, (alphabet, layout, n)
            else:
                assert (n, setup["files"][b]) not in confirmed and any(r[0] == n for r in plain), (alphabet, layout, n)
        if setup["dna"]:
            assert {r[6] for r in got} == {"+", "-"}
    # without --counts, into a file
    dest = tmp_path / "out.tsv"
    rc, so, se = _run("search", "-e", str(EDITS), "--verify", "-o", str(dest), setup["indexes"]["default"], setup["qfile"])
    assert rc == 0 and so == "", se
    rows = [tuple(line.split("\t")) for line in dest.read_text().splitlines()]
    assert rows and all(len(r) == (6 if setup["dna"] else 5) for r in rows)


def test_cli_verify_small_text_cache(cli_setup):
    """TETREX_VERIFY_TEXT_MB is a bound, not a result: with room for one bin at a time (a fraction of a MiB: every bin
    pushes the one before it out) the rows are the same"""
    setup = cli_setup["peptide"]
    args = ("search", "-e", str(EDITS), "--verify", setup["indexes"]["flat"], setup["qfile"])
    rc, so, se = _run(*args)
    assert rc == 0, se
    r = subprocess.run([TETREX, *args], capture_output=True, text=True, timeout=600, env=dict(os.environ, TETREX_VERIFY_TEXT_MB="0.001", TXQ_EDIT_CHUNK="64"))
    assert r.returncode == 0 and r.stdout == so and so, r.stderr


def test_cli_verify_missing_bin_file(cli_setup, tmp_path):
    """a candidate bin whose file cannot be read: an error that names it, exit status 1"""
    import shutil
    setup = cli_setup["peptide"]
    d = tmp_path / "lib"
    d.mkdir()
    files = []
    for f in setup["files"][:6]:
        files.append(str(d / os.path.basename(f)))
        shutil.copy(f, files[-1])
    rc, so, se = _run("index", "-k", "6", "-i", str(d / "ix"), *files)
    assert rc == 0, se
    source = {b for _, b, _, e in setup["queries"] if b < 6}
    gone = files[min(source)]
    os.remove(gone)
    rc, so, se = _run("search", "-e", str(EDITS), "--verify", str(d / "ix.ibf"), setup["qfile"])
    assert rc == 1 and gone in se and "--verify" in se, se
