"""GPU parity of `tetrex search --translate --verify-frames`.

The kernel: txq_translate_frames against translate_frame of tests/translate_ref.py, bytes and offsets; the _device entry on
sequences and frame buffers at odd addresses between guard bytes, and with a capacity below the bound.

The command line: on indexes that `tetrex index` builds from generated FASTA, stdout must be exactly the rows that
tests/translate_ref.py (the candidates) and tests/edit_ref.py (Sellers' distance of the frame's letters to the bin's records,
classes A..Z) give.  Neither shares anything with the code under test."""
import os
import re
import subprocess

import numpy as np
import pytest

import edit_ref as E
import translate_ref as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TETREX = os.path.join(ROOT, "bin", "tetrex")


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


def random_nt(rng, L, ambiguous=0.0):
    s = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=L)
    if ambiguous:
        s[rng.random(L) < ambiguous] = ord("N")
    return s.tobytes().decode()


def reference_frames(records):
    """(uint8 frames back to back, uint64 offsets[6 n + 1]) by translate_ref.translate_frame"""
    frames = [T.translate_frame(s, f).encode() for s in records for f in range(6)]
    offsets = np.zeros(len(frames) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(x) for x in frames])
    return np.frombuffer(b"".join(frames), dtype=np.uint8), offsets


# ---- the kernel ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def batch():
    """2000 reads of 30..300 nt (1 % ambiguous bytes, every 7th lower case, every 11th with U), the special records of
    test_gpu_translate.py, every length 0..20, one record of 200 000 nt between short ones, empty records at the end"""
    rng = np.random.default_rng(77)
    records = []
    for i in range(2000):
        s = random_nt(rng, int(rng.integers(30, 301)), 0.01)
        if i % 7 == 0:
            s = s.lower()
        if i % 11 == 0:
            s = s.replace("T", "U").replace("t", "u")
        records.append(s)
    special = ["", "A", "AC", "ACG", "ACGTACGTA", "N" * 100, "n" * 37, "TAA" * 40, "TAATAGTGA" * 13 + "T", "ACGT-acgu RYKM*" * 9, ""]
    for i, s in enumerate(special):
        records.insert(1 + 170 * i, s)
    for L in range(21):
        records.insert(900 + 3 * L, random_nt(rng, L, 0.05))
    records.insert(1000, random_nt(rng, 200_000, 0.0005))
    records += ["", "ACGTAC", "", ""]
    return records, reference_frames(records)


def test_frames_equal_restatement(capi, batch):
    records, (want, want_o) = batch
    got, got_o = capi.translate_frames(records)
    assert got_o.size == 6 * len(records) + 1
    assert np.array_equal(got_o, want_o)
    assert got.size == want.size and np.array_equal(got, want), int(np.flatnonzero(got != want)[0])
    lengths = np.concatenate([[0], np.cumsum([len(r) for r in records])])
    assert capi.translate_frames_bound(lengths) == int(want_o[-1])
    # the call is deterministic
    again, again_o = capi.translate_frames(records)
    assert np.array_equal(again, got) and np.array_equal(again_o, got_o)


def test_frames_of_degenerate_batches(capi):
    f, o = capi.translate_frames([])
    assert f.size == 0 and np.array_equal(o, [0])
    f, o = capi.translate_frames([""])
    assert f.size == 0 and np.array_equal(o, np.zeros(7))
    f, o = capi.translate_frames(["", "A", "AC", "c", "", "GT"])
    assert f.size == 0 and np.array_equal(o, np.zeros(37))
    f, o = capi.translate_frames(["AC", "ATG", "g"])
    assert f.tobytes() == b"MH" and np.array_equal(o, [0] * 7 + [1, 1, 1, 2, 2, 2] + [2] * 6)
    with pytest.raises(capi.TxqError):  # the host twin refuses a buffer below the bound
        seq, rec = capi._records(["ATGATG"])
        capi.check(capi.lib().txq_translate_frames(seq.ctypes.data, rec.ctypes.data_as(capi.u64p), 1, np.zeros(8, np.uint8).ctypes.data, 5,
                                                   np.zeros(7, np.uint64).ctypes.data_as(capi.u64p)))


def test_frames_device_entry_at_odd_addresses(capi):
    """txq_translate_frames_device with the sequence 1, 5 and 15 bytes and the frames 0, 1, 5 and 15 bytes behind a 16-byte
    boundary, 64 guard bytes on either side of the frames: the guards stay, the contents are the restatement's.  With the
    capacity cut to about half, nothing at or behind it is written, what lies below is right, the offsets are complete."""
    rng = np.random.default_rng(12)
    records = [random_nt(rng, int(rng.integers(0, 400)), 0.01) for _ in range(150)]
    records.insert(70, random_nt(rng, 5000, 0.001))  # (several units)
    records += ["", "AC", ""]
    want, want_o = reference_frames(records)
    guard = 64
    for frames_at in (0, 1, 5, 15):
        for seq_at in (1, 5, 15):
            buf, off, bound = capi.translate_frames_device(records, seq_at=seq_at, frames_at=frames_at, guard=guard)
            assert bound == want.size and np.array_equal(off, want_o), (seq_at, frames_at)
            assert np.array_equal(buf[guard:guard + bound], want), (seq_at, frames_at)
            assert (buf[:guard] == 0xA5).all() and (buf[guard + bound:] == 0xA5).all(), (seq_at, frames_at)
        cap = want.size // 2 + frames_at
        buf, off, bound = capi.translate_frames_device(records, capacity=cap, seq_at=5, frames_at=frames_at, guard=guard)
        assert np.array_equal(off, want_o), frames_at
        assert np.array_equal(buf[guard:guard + cap], want[:cap]), frames_at
        assert (buf[:guard] == 0xA5).all() and (buf[guard + cap:] == 0xA5).all(), frames_at
    buf, off, bound = capi.translate_frames_device(records, capacity=0, guard=guard)
    assert np.array_equal(off, want_o) and (buf == 0xA5).all()


# ---- the command line ---------------------------------------------------------------------------------------------------

AMINO = "ACDEFGHIKLMNPQRSTVWY"
ALPHABETS = {"peptide": (6, [], 0), "murphy": (5, ["-r", "murphy"], 1)}  # name: (k, index flags, reduction)
LAYOUTS = {"flat": ["-i"], "sized": ["--layout", "sized"]}
EDITS = 2
CODES = E.letter_codes("ABCDEFGHIJKLMNOPQRSTUVWXYZ")
CODONS_OF = {}
for _codon, _aa in T.CODON.items():
    CODONS_OF.setdefault(_aa, []).append(_codon)


def _run(*args, env=None):
    r = subprocess.run([TETREX, *args], capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
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


def generate(name):
    """The bins and reads of one alphabet, without a GPU.  70 bins of two records of 150..400 residues, bin 0 with a record of
    800 and bin 1 with one of 4400.  Reads (name, source bin, source frame, nucleotides, edits planted or None for a read that
    must be dropped): 40 slices of 60 residues with up to EDITS edits; two with 3 adjacent substitutions (they pass the
    filter — at most k + 2 k-mers are lost, 2 k are allowed — and are 3 edits away); one unedited slice with one codon turned
    into a stop (one edit: a stop matches nothing); 600 residues of bin 0's long record (the long-pattern kernel) and 4200 of
    bin 1's (the host route) with up to EDITS edits; a read shorter than 3 k and an all-N read."""
    k = ALPHABETS[name][0]
    rng = np.random.default_rng(300 + len(name))
    pep = lambda n: "".join(rng.choice(list(AMINO), size=n))
    seqs = [[pep(int(rng.integers(150, 400))) for _ in range(2)] for _ in range(70)]
    seqs[0][0] = pep(800)
    seqs[1][0] = pep(4400)
    reads = []

    def plant(label, b, peptide, edits, stop_at=None):
        codons = [CODONS_OF[a][int(rng.integers(0, len(CODONS_OF[a])))] for a in peptide]
        if stop_at is not None:
            codons[stop_at] = "TAA"
        front, behind = random_nt(rng, int(rng.integers(0, 3))), random_nt(rng, int(rng.integers(0, 3)))
        nt, frame = front + "".join(codons) + behind, len(front)
        if len(reads) % 2:
            nt, frame = T.reverse_complement(nt), frame + 3
        want = peptide if stop_at is None else peptide[:stop_at] + "*" + peptide[stop_at + 1:]
        assert T.translate_frame(nt, frame) == want
        reads.append(("%s%d_b%d" % (label, len(reads), b), b, frame, nt, edits))

    def piece(b, rec, n):
        at = int(rng.integers(0, len(seqs[b][rec]) - n))
        return seqs[b][rec][at:at + n]

    for _ in range(40):
        b, e = int(rng.integers(0, 70)), int(rng.integers(0, EDITS + 1))
        plant("r", b, _edit(piece(b, int(rng.integers(0, 2)), 60), e, rng), e)
    for _ in range(2):
        b = int(rng.integers(2, 70))
        s = list(piece(b, 0, 60))
        for at in (29, 30, 31):
            s[at] = AMINO[(AMINO.index(s[at]) + 1 + int(rng.integers(0, len(AMINO) - 1))) % len(AMINO)]
        plant("sub3_", b, "".join(s), None)
    b = int(rng.integers(2, 70))
    plant("stop", b, piece(b, 1, 60), 1, stop_at=30)
    plant("long", 0, _edit(piece(0, 0, 600), EDITS, rng), EDITS)
    plant("huge", 1, _edit(piece(1, 0, 4200), EDITS, rng), EDITS)
    reads.append(("tiny", -1, -1, random_nt(rng, 3 * k - 1), None))
    reads.append(("all_n", -1, -1, "N" * (3 * k + 6), None))
    return seqs, reads


_distance_cache = {}


def reference_hit(alphabet, seqs, read, frame, b):
    """(distance, record, end) of frame `frame` of the read against bin b by edit_ref, NONE three times above EDITS"""
    key = (alphabet, read[0], frame, b)
    if key not in _distance_cache:
        letters = T.translate_frame(read[3], frame)
        _distance_cache[key] = E.search([letters], seqs[b], [0, len(seqs[b])], [(0, 0, EDITS)], CODES)[0].tolist()
    return _distance_cache[key]


@pytest.fixture(scope="module")
def cli_setup(tmp_path_factory):
    root = tmp_path_factory.mktemp("verify_frames_cli")
    out = {}
    for name, (k, flags, red) in ALPHABETS.items():
        seqs, reads = generate(name)
        d = root / name
        d.mkdir()
        files = []
        for b, recs in enumerate(seqs):
            p = d / ("bin%02d.fa" % b)
            p.write_text("".join(">b%d_%d some comment\n%s\n" % (b, i, r) for i, r in enumerate(recs)))
            files.append(str(p))
        qf = d / "reads.fa"
        qf.write_text("".join(">%s some comment\n%s\n" % (r[0], r[3]) for r in reads))
        indexes = {}
        for lay, lflags in LAYOUTS.items():
            rc, so, se = _run("index", "-k", str(k), *flags, *lflags, str(d / lay), *files)
            assert rc == 0 and os.path.exists(d / (lay + ".ibf")), se
            indexes[lay] = str(d / (lay + ".ibf"))
        out[name] = dict(files=[os.path.abspath(f) for f in files], seqs=seqs, reads=reads, qfile=str(qf), indexes=indexes, k=k, red=red)
    return out


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("alphabet", list(ALPHABETS))
def test_cli_verify_frames(oracle, cli_setup, tmp_path, alphabet, layout):
    setup = cli_setup[alphabet]
    k, path, seqs, reads = setup["k"], setup["indexes"][layout], setup["seqs"], setup["reads"]
    by_name = {r[0]: r for r in reads}
    bin_of = {p: b for b, p in enumerate(setup["files"])}
    # the reference: the filter's rows are the candidates, edit_ref confirms them
    candidates, skipped = T.expected_rows(oracle, path, [(r[0], r[3]) for r in reads], k, setup["red"], lambda n: max(n - k * EDITS, 0))
    want = []
    for n, p, f, c, m in candidates:
        d, rec, end = reference_hit(alphabet, seqs, by_name[n], T.FRAMES.index(f), bin_of[p])
        if d != E.NONE:
            assert d <= EDITS
            want.append((n, p, f, "%d/%d" % (c, m), str(d), "b%d_%d" % (bin_of[p], rec), str(end)))
    # conditions on the inputs: the adjacent substitutions pass the filter and are dropped, the planted reads are confirmed
    keys = {(n, p, f) for n, p, f, _, _ in candidates}
    dropped = [r for r in reads if r[0].startswith("sub3_")]
    assert len(dropped) == 2 and len(candidates) - len(want) >= 2 and len(want) >= 40
    for r in dropped:
        assert (r[0], setup["files"][r[1]], T.FRAMES[r[2]]) in keys, r[0]
        assert reference_hit(alphabet, seqs, r, r[2], r[1])[0] == E.NONE
    rc, so, se = _run("search", "--translate", "-e", str(EDITS), "--verify-frames", "--counts", "-v", path, setup["qfile"], env={"TETREX_TRACE": "1"})
    assert rc == 0, se
    got = [tuple(line.split("\t")) for line in so.splitlines()]
    assert got == want, (alphabet, layout)
    # every planted read within E edits is there with its source bin and frame, no further away than the edits planted
    row_of = {(n, p, f): int(d) for n, p, f, _, d, _, _ in got}
    for n, b, frame, _, edits in reads:
        if b >= 0 and edits is not None:
            assert row_of[(n, setup["files"][b], T.FRAMES[frame])] <= edits, (alphabet, layout, n)
        elif b >= 0:
            assert (n, setup["files"][b], T.FRAMES[frame]) not in row_of, (alphabet, layout, n)
    stop = next(r for r in reads if r[0].startswith("stop"))
    assert row_of[(stop[0], setup["files"][stop[1]], T.FRAMES[stop[2]])] == 1  # a stop matches nothing
    # notes and traces
    for n, _, _, _, _ in reads:
        assert (("[tetrex search] %s: no frame" % n) in se) == (n in skipped), n
    assert {"tiny", "all_n"} <= set(skipped)
    assert "Verified: %d of %d candidate pairs" % (len(want), len(candidates)) in se, se
    routes = re.search(r"verify routes: device (\d+), device-long (\d+), host (\d+)", se)
    assert routes and all(int(x) > 0 for x in routes.groups()), se
    assert sum(int(x) for x in routes.groups()) == len(candidates)
    # -o, without counts
    dest = tmp_path / ("%s_%s.tsv" % (alphabet, layout))
    rc, so2, se2 = _run("search", "--translate", "-e", str(EDITS), "--verify-frames", "-o", str(dest), path, setup["qfile"])
    assert rc == 0 and so2 == "", se2
    assert [tuple(line.split("\t")) for line in dest.read_text().splitlines()] == [w[:3] + w[4:] for w in want]
    assert "Verified:" not in se2 and "verify routes" not in se2
    # the host route for the frames, and one bin resident at a time: the same bytes
    for env in ({"TETREX_VERIFY_FRAMES": "host"}, {"TETREX_VERIFY_TEXT_MB": "0.001"}):
        rc, so3, se3 = _run("search", "--translate", "-e", str(EDITS), "--verify-frames", "--counts", path, setup["qfile"], env=dict(env, TETREX_TRACE="1"))
        assert rc == 0 and so3 == so, (env, se3)
        assert routes.group(0) in se3, (env, se3)


def test_cli_plain_translate_is_unchanged(oracle, cli_setup):
    """without the flag the rows are the filter's, as before: the candidates, every one of them"""
    setup = cli_setup["peptide"]
    k, path = setup["k"], setup["indexes"]["flat"]
    candidates, _ = T.expected_rows(oracle, path, [(r[0], r[3]) for r in setup["reads"]], k, setup["red"], lambda n: max(n - k * EDITS, 0))
    rc, so, se = _run("search", "--translate", "-e", str(EDITS), path, setup["qfile"])
    assert rc == 0, se
    assert [tuple(line.split("\t")) for line in so.splitlines()] == [(n, p, f) for n, p, f, _, _ in candidates]
