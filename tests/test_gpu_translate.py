"""GPU parity of six-frame translated search: txq_translate against the restatement of tests/translate_ref.py
bit for bit, txq_hit_list_device against numpy, and `tetrex search --translate` on indexes that `tetrex index` builds from
generated FASTA — against the restatement, against the q-gram lemma, and against plain `tetrex search` on the same peptides."""
import math
import os
import subprocess

import numpy as np
import pytest

import translate_ref as T
from search_ref import csr, unpack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TETREX = os.path.join(ROOT, "bin", "tetrex")


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


# ---- translation --------------------------------------------------------------------------------------------------------

def random_nt(rng, L, ambiguous=0.0):
    s = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=L)
    if ambiguous:
        s[rng.random(L) < ambiguous] = ord("N")
    return s.tobytes().decode()


@pytest.fixture(scope="module")
def batch():
    """5000 reads of 30..300 nt (1 % ambiguous bytes, some lower case, some with U), empty and short records, all-N and all-stop
    records, and one record of 2 x 10^6 nt between short ones; with every record's six frames as residue letters."""
    rng = np.random.default_rng(42)
    records = []
    for i in range(5000):
        s = random_nt(rng, int(rng.integers(30, 301)), 0.01)
        if i % 7 == 0:
            s = s.lower()
        if i % 11 == 0:
            s = s.replace("T", "U")
        records.append(s)
    special = ["", "A", "AC", "ACG", "ACGTACGTA", "N" * 100, "n" * 37, "TAA" * 40, "TAATAGTGA" * 13 + "T", "ACGT-acgu RYKM*" * 9, ""]
    for i, s in enumerate(special):
        records.insert(1 + 450 * i, s)
    records.insert(2500, random_nt(rng, 2_000_000, 0.0005))
    records += ["", "ACGTAC", ""]
    frames = [[T.translate_frame(s, f) for f in range(6)] for s in records]
    return records, frames


def restated(frames, k, reduction):
    from tetrex_amd import host
    qs = []
    for six in frames:
        for residues in six:
            parts = [host.record_values_array(seg, k, dna=False, reduction=reduction) for seg in residues.split("*") if len(seg) >= k]
            qs.append(np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64))
    return csr(qs)


@pytest.mark.parametrize("reduction", [0, 1, 2])
@pytest.mark.parametrize("k", [3, 6, 12])
def test_translate_equals_restatement(capi, batch, k, reduction):
    from tetrex_amd import host
    records, frames = batch
    want_v, want_o = restated(frames, k, reduction)
    got_v, got_o = capi.translate(records, k, host.peptide_codes(reduction))
    assert got_o.size == 6 * len(records) + 1
    assert np.array_equal(got_o, want_o)
    assert np.array_equal(got_v, want_v)
    assert int(want_o[-1]) <= capi.translate_bound(np.concatenate([[0], np.cumsum([len(r) for r in records])]), k)
    # the host's restatement, record by record, agrees too
    at = 0
    for r, s in enumerate(records):
        hv, ho = host.translated_values(s, k, reduction)
        assert np.array_equal(ho, want_o[6 * r:6 * r + 7] - want_o[6 * r]), r
        assert np.array_equal(hv, want_v[at:at + hv.size]), r
        at += hv.size
    assert at == want_v.size


def test_translate_small_and_empty_batches(capi):
    from tetrex_amd import host
    codes = host.peptide_codes(0)
    v, o = capi.translate([], 6, codes)
    assert v.size == 0 and np.array_equal(o, [0])
    v, o = capi.translate(["", "", ""], 6, codes)
    assert v.size == 0 and np.array_equal(o, np.zeros(19))
    rng = np.random.default_rng(3)
    for k in (1, 2, 5, 12):
        records = [random_nt(rng, L, 0.02) for L in list(range(0, 3 * k + 8)) + [191, 192, 193, 194, 195, 383, 384, 385, 767, 768, 769, 1000]]
        want_v, want_o = T.translate_records(records, k)
        got_v, got_o = capi.translate(records, k, codes)
        assert np.array_equal(got_o, want_o), k
        assert np.array_equal(got_v, want_v), k
    # records that do not start at byte 0 of the buffer, at every alignment
    body = random_nt(rng, 700, 0.01)
    want_v, want_o = T.translate_records([body[:300], body[300:]], 4)
    for pad in range(0, 17):
        seq = np.frombuffer(("G" * pad + body).encode(), dtype=np.uint8)
        rec = np.array([pad, pad + 300, pad + 700], dtype=np.uint64)
        got_v, got_o = capi.translate((seq, rec), 4, codes)
        assert np.array_equal(got_o, want_o) and np.array_equal(got_v, want_v), pad


def test_translate_device_entry_point(capi):
    """txq_translate_device on the caller's device buffers, offsets in the form txq_count_device takes"""
    from tetrex_amd import host
    rng = np.random.default_rng(5)
    records = [random_nt(rng, int(rng.integers(0, 400)), 0.01) for _ in range(300)]
    seq, rec = capi._records(records)
    k = 6
    bound = capi.translate_bound(rec, k)
    d_seq, d_rec = capi.DeviceBuffer.from_numpy(seq), capi.DeviceBuffer.from_numpy(rec)
    d_codes = capi.DeviceBuffer.from_numpy(host.peptide_codes(1))
    guard = 64
    d_val = capi.DeviceBuffer.from_numpy(np.full(bound + guard, 0xABABABABABABABAB, dtype=np.uint64))
    d_off = capi.DeviceBuffer(8 * (6 * len(records) + 1))
    capi.check(capi.lib().txq_translate_device(d_seq.ptr, d_rec.ptr, len(records), k, d_codes.ptr, d_val.ptr, d_off.ptr, None))
    capi.synchronize()
    want_v, want_o = T.translate_records(records, k, 1)
    assert np.array_equal(d_off.to_numpy(np.uint64, (6 * len(records) + 1,)), want_o)
    got = d_val.to_numpy(np.uint64, (bound + guard,))
    assert np.array_equal(got[:want_v.size], want_v)
    assert (got[bound:] == np.uint64(0xABABABABABABABAB)).all()  # nothing behind the bound was touched
    for b in (d_seq, d_rec, d_codes, d_val, d_off):
        b.free()


def test_translate_device_sequence_that_is_not_16_byte_aligned(capi):
    """txq_translate_device on a sequence that begins 1, 7 and 15 bytes behind a 16-byte boundary: records of 50 and 7 bytes,
    k = 3.  The 16-byte blocks at either end of the sequence are staged from byte loads."""
    from tetrex_amd import host
    rng = np.random.default_rng(8)
    records = [random_nt(rng, 50, 0.02), random_nt(rng, 7)]
    seq, rec = capi._records(records)
    k = 3
    bound = capi.translate_bound(rec, k)
    want_v, want_o = T.translate_records(records, k)
    assert want_v.size > 50
    d_rec, d_codes = capi.DeviceBuffer.from_numpy(rec), capi.DeviceBuffer.from_numpy(host.peptide_codes(0))
    results = {}
    for at in (0, 1, 7, 15):
        around = np.full(at + seq.size + 33, ord("A"), dtype=np.uint8)
        around[at:at + seq.size] = seq
        d_seq = capi.DeviceBuffer.from_numpy(around)
        assert d_seq.ptr % 16 == 0
        d_val = capi.DeviceBuffer.from_numpy(np.full(bound + 8, 0xABABABABABABABAB, dtype=np.uint64))
        d_off = capi.DeviceBuffer(8 * (6 * len(records) + 1))
        capi.check(capi.lib().txq_translate_device(d_seq.ptr + at, d_rec.ptr, len(records), k, d_codes.ptr, d_val.ptr, d_off.ptr, None))
        capi.synchronize()
        results[at] = (d_val.to_numpy(np.uint64, (bound + 8,)), d_off.to_numpy(np.uint64, (6 * len(records) + 1,)))
        for b in (d_seq, d_val, d_off):
            b.free()
    for at in (1, 7, 15):
        assert np.array_equal(results[at][0], results[0][0]) and np.array_equal(results[at][1], results[0][1]), at
    assert np.array_equal(results[0][1], want_o)
    assert np.array_equal(results[0][0][:want_v.size], want_v)
    assert (results[0][0][bound:] == np.uint64(0xABABABABABABABAB)).all()
    d_rec.free()
    d_codes.free()


# ---- hit list -----------------------------------------------------------------------------------------------------------

def numpy_list(hits, counts):
    bits = unpack(hits)
    q, b = np.nonzero(bits)  # row-major: (query, bin) order
    c = counts[q, b] if counts is not None else np.zeros(q.size, dtype=np.uint32)
    return np.stack([q, b, c], axis=1).astype(np.uint32) if q.size else np.zeros((0, 3), dtype=np.uint32)


def random_hits(rng, n, W, density):
    bits = rng.random((n, 64 * W)) < density
    return np.packbits(bits, axis=1, bitorder="little").view("<u8").reshape(n, W).copy()


@pytest.mark.parametrize("W", [1, 16, 141])
@pytest.mark.parametrize("density", [0.0, 0.001, 0.3, 1.0], ids=["empty", "sparse", "dense", "full"])
def test_hit_list_equals_numpy(capi, W, density):
    rng = np.random.default_rng(W * 1000 + int(density * 100))
    n = 300 if W < 100 else 61
    hits = random_hits(rng, n, W, density)
    counts = rng.integers(0, 1 << 32, size=(n, 64 * W), dtype=np.uint64).astype(np.uint32)
    for with_counts in (True, False):
        want = numpy_list(hits, counts if with_counts else None)
        rows, total = capi.hit_list(hits, counts if with_counts else None, guard=8)
        assert total == want.shape[0]
        assert np.array_equal(rows[:total], want)
        assert (rows[total:] == 0xFFFFFFFF).all()
        # a capacity below the total: the total is still reported, the prefix is right, nothing is written behind it
        for cap in sorted({0, 1, total // 2, max(total - 1, 0)}):
            if cap >= total:
                continue
            rows, got_total = capi.hit_list(hits, counts if with_counts else None, capacity=cap, guard=16)
            assert got_total == total
            assert np.array_equal(rows[:cap], want[:cap])
            assert (rows[cap:] == 0xFFFFFFFF).all()


def test_hit_list_one_bit_and_no_queries(capi):
    for W, q, b in ((1, 0, 0), (1, 4, 63), (16, 17, 64 * 15 + 63), (141, 2, 64 * 77 + 5)):
        hits = np.zeros((20, W), dtype=np.uint64)
        hits[q, b // 64] = np.uint64(1) << np.uint64(b % 64)
        counts = np.arange(20 * 64 * W, dtype=np.uint32).reshape(20, 64 * W)
        rows, total = capi.hit_list(hits, counts, guard=4)
        assert total == 1 and rows[0].tolist() == [q, b, int(counts[q, b])]
        assert (rows[1:] == 0xFFFFFFFF).all()
    rows, total = capi.hit_list(np.zeros((0, 3), dtype=np.uint64), None, capacity=0, guard=4)
    assert total == 0 and (rows == 0xFFFFFFFF).all()


def test_hit_list_of_a_count_call(capi, oracle):
    """the list of txq_count's own output on an index: counts of the listed bins reach the thresholds, in order"""
    from helpers import random_words, splitmix64
    bins, rows_, h = 1000, 1031, 3
    ix = capi.Index.upload_ibf(bins, rows_, h, random_words(bins, rows_, 0.5, 9))
    values, offsets = csr([splitmix64(i, n) for i, n in enumerate([0, 1, 64, 300, 2000, 7])])
    thr = np.array([1, 1, 8, 40, 260, 2], dtype=np.uint32)
    hits, counts = ix.count(values, offsets, thr, counts=True)
    rows, total = capi.hit_list(hits, counts)
    assert np.array_equal(rows[:total], numpy_list(hits, counts))
    assert (rows[:total, 2] >= thr[rows[:total, 0]]).all() and total > 0
    ix.free()


# ---- the command line ---------------------------------------------------------------------------------------------------

AMINO = "ACDEFGHIKLMNPQRSTVWY"
ALPHABETS = {"peptide": (6, [], 0), "murphy": (5, ["-r", "murphy"], 1)}  # name: (k, index flags, reduction)
LAYOUTS = {"flat": ["-i"], "default": [], "sized": ["--layout", "sized"]}
EDITS = 2
CODONS_OF = {}
for _codon, _aa in T.CODON.items():
    CODONS_OF.setdefault(_aa, []).append(_codon)


def _run(*args):
    r = subprocess.run([TETREX, *args], capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


def _edit(seq, e, rng):
    """e residue-level substitutions or indels (never a stop: the source frame stays stop-free)"""
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


@pytest.fixture(scope="module")
def cli_setup(tmp_path_factory):
    """For each alphabet: 70 peptide bins of generated FASTA, their three indexes, 40 reads (a 60-residue slice of a bin with
    up to EDITS residue edits, back-translated with random synonymous codons, 0..2 random nucleotides in front and behind,
    every other one reverse-complemented), a read shorter than 3 k and an all-N read; and the edited peptides as a peptide
    query file for plain `tetrex search`."""
    root = tmp_path_factory.mktemp("translate_cli")
    out = {}
    for name, (k, flags, red) in ALPHABETS.items():
        rng = np.random.default_rng(10 + len(name))
        d = root / name
        d.mkdir()
        files, seqs = [], []
        for b in range(70):
            recs = ["".join(rng.choice(list(AMINO), size=int(rng.integers(150, 400)))) for _ in range(2)]
            seqs.append(recs)
            p = d / ("bin%02d.fa" % b)
            p.write_text("".join(">b%d_%d\n%s\n" % (b, i, r) for i, r in enumerate(recs)))
            files.append(str(p))
        reads = []  # (name, source bin, source frame index, nucleotides, edited peptide)
        for q in range(40):
            b = int(rng.integers(0, 70))
            rec = seqs[b][int(rng.integers(0, 2))]
            at = int(rng.integers(0, len(rec) - 60))
            pep = _edit(rec[at:at + 60], int(rng.integers(0, EDITS + 1)), rng)
            cds = "".join(CODONS_OF[a][int(rng.integers(0, len(CODONS_OF[a])))] for a in pep)
            front, behind = random_nt(rng, int(rng.integers(0, 3))), random_nt(rng, int(rng.integers(0, 3)))
            nt = front + cds + behind
            frame = len(front)
            if q % 2:
                nt = T.reverse_complement(nt)
                frame += 3
            assert T.translate_frame(nt, frame) == pep
            reads.append(("r%d_b%d" % (q, b), b, frame, nt, pep))
        reads.append(("tiny", -1, -1, random_nt(rng, 3 * k - 1), ""))
        reads.append(("all_n", -1, -1, "N" * (3 * k + 6), ""))
        qf = d / "reads.fa"
        qf.write_text("".join(">%s some comment\n%s\n" % (n, s) for n, _, _, s, _ in reads))
        pf = d / "peptides.fa"
        pf.write_text("".join(">%s\n%s\n" % (n, p) for n, b, _, _, p in reads if b >= 0))
        indexes = {}
        for lay, lflags in LAYOUTS.items():
            rc, so, se = _run("index", "-k", str(k), *flags, *lflags, str(d / lay), *files)
            assert rc == 0 and os.path.exists(d / (lay + ".ibf")), se
            indexes[lay] = str(d / (lay + ".ibf"))
        out[name] = dict(files=[os.path.abspath(f) for f in files], reads=reads, qfile=str(qf), pfile=str(pf), indexes=indexes, k=k, red=red)
    return out


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("alphabet", list(ALPHABETS))
def test_cli_search_translate(oracle, cli_setup, tmp_path, alphabet, layout):
    setup = cli_setup[alphabet]
    k, path = setup["k"], setup["indexes"][layout]
    records = [(n, s) for n, _, _, s, _ in setup["reads"]]
    rc, so, se = _run("search", "--translate", "-e", str(EDITS), "--counts", "-v", path, setup["qfile"])
    assert rc == 0, se
    got = [tuple(line.split("\t")) for line in so.splitlines()]
    # (a) the restatement's rows, exactly
    want, skipped = T.expected_rows(oracle, path, records, k, setup["red"], lambda n: max(n - k * EDITS, 0))
    assert got == [(n, p, f, "%d/%d" % (c, m)) for n, p, f, c, m in want], (alphabet, layout)
    # (e) the records none of whose frames is searched are named on stderr, and only they
    assert {"tiny", "all_n"} <= set(skipped)
    for n, _ in records:
        assert (("[tetrex search] %s: no frame" % n) in se) == (n in skipped), n
    assert "Search time:" in se
    # (b) the q-gram lemma: every read is reported in its source bin with its source frame
    row_of = {(n, p, f): cn for n, p, f, cn in got}
    for n, b, frame, _, _ in setup["reads"]:
        if b >= 0:
            assert (n, setup["files"][b], T.FRAMES[frame]) in row_of, (alphabet, layout, n)
    # (c) count/n of that row is what plain `tetrex search` gives the same edited peptide as a peptide record
    rc, pso, pse = _run("search", "-e", str(EDITS), "--counts", path, setup["pfile"])
    assert rc == 0, pse
    plain = {(n, p): cn for n, p, cn in (line.split("\t") for line in pso.splitlines())}
    checked = 0
    for n, b, frame, _, _ in setup["reads"]:
        if b >= 0:
            assert row_of[(n, setup["files"][b], T.FRAMES[frame])] == plain[(n, setup["files"][b])], (alphabet, layout, n)
            checked += 1
    assert checked == 40
    # (d) --threshold, -o
    dest = tmp_path / ("%s_%s.tsv" % (alphabet, layout))
    rc, so, se = _run("search", "--translate", "--threshold", "0.6", "-o", str(dest), path, setup["qfile"])
    assert rc == 0 and so == "", se
    got = [tuple(line.split("\t")) for line in dest.read_text().splitlines()]
    want, skipped = T.expected_rows(oracle, path, records, k, setup["red"], lambda n: math.ceil(0.6 * n))
    assert got == [(n, p, f) for n, p, f, _, _ in want], (alphabet, layout)
    assert "tiny" in skipped and "[tetrex search] tiny: no frame" in se


def test_cli_translate_large_e_reports_nothing(cli_setup):
    """a threshold of 0 reports nothing under --translate (plain search reports every bin): every record gets its note"""
    setup = cli_setup["peptide"]
    rc, so, se = _run("search", "--translate", "-e", "1000", setup["indexes"]["default"], setup["qfile"])
    assert rc == 0 and so == ""
    assert se.count(": no frame") == len(setup["reads"])
