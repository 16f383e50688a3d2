"""GPU parity of txq_translate_windows (include/txq.h; `tetrex search --translate --frame-window`): the window
offsets, begins and lens against the brute-force restatement of tests/frame_window_ref.py, exactly; the values and offsets
against txq_translate's on the same records; begins and ends that never decrease; and the device arrays fed straight into
txq_count_windows_device, whose hits and counts must equal txq_count with every window written out as a query of its own.
Records: 0, 1, 2, 3k - 1 .. 3k + 2 bytes; frames of R = k - 1, k, W - 1, W, W + 1, W + S - 1, W + S, W + S + 1 residues at each
offset, random and stop-free; stops at the first and the last codon, on the windows' boundaries and all over one window;
lower case, U and ambiguous bytes; one record of 3 * 768 + 100 bytes (three units at the minimum chunk) that is stop-free
across the unit boundaries in frame +2; 300 records of 30 to 60 bytes in one unit.  k = 1, 6, 12; S = 1, W / 2, W."""
import numpy as np
import pytest

import frame_window_ref as F
from helpers import random_words, layout_hibf
from search_ref import csr

pytestmark = pytest.mark.gpu

W = 40
SENSE = ["GCT", "AAA", "GGC", "CTG", "TTC", "ACC", "CAG", "GAT"]


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


def random_nt(rng, L, junk=0.0):
    s = rng.choice(list("ACGT"), size=L)
    if junk:
        s = np.where(rng.random(L) < junk, rng.choice(list("NRYKM-* nx"), size=L), s)
    return "".join(s)


def planted(rng, R, o, stops=()):
    """a record whose frame +(o + 1) has R residues, stop-free but at the codons in `stops`"""
    codons = [SENSE[int(i)] for i in rng.integers(0, 8, size=R)]
    for c in stops:
        if 0 <= c < R:
            codons[c] = "TAG" if c % 2 else "TAA"
    return random_nt(rng, o) + "".join(codons)


_cases = {}


def case(k, S):
    """records and the restatement's arrays, computed once per (k, S) and left unchanged"""
    if (k, S) not in _cases:
        rng = np.random.default_rng(1000 * k + S)
        records = [random_nt(rng, L) for L in (0, 1, 2, 3 * k - 1, 3 * k, 3 * k + 1, 3 * k + 2)]
        for R in (k - 1, k, W - 1, W, W + 1, W + S - 1, W + S, W + S + 1):
            for o in range(3):
                records.append(random_nt(rng, 3 * R + o, 0.02))
                records.append(planted(rng, R, o))
                records.append(planted(rng, R, o, (0, R - 1)))
                records.append(planted(rng, R, o, (S, S - 1, W - k, W - k + 1, W, W - 1, R - W, R - k)))
        records.append(planted(rng, 3 * W, 1, range(S + k - 1, S + W, k) if k > 1 else range(S, S + W)))  # an empty window
        records.append(random_nt(rng, 200).lower())
        records.append(random_nt(rng, 200).replace("T", "U"))
        records.append(random_nt(rng, 300, 0.2))
        records.append("")
        records.append(planted(rng, (3 * 768 + 100) // 3, 1, (5, 400, 401)) + "AC"[:(3 * 768 + 100 - 1) % 3])
        assert len(records[-1]) == 3 * 768 + 100
        records.append(random_nt(rng, 3 * 768 + 100, 0.01))
        records += [random_nt(rng, int(rng.integers(30, 61)), 0.03) for _ in range(300)]
        want = F.translate_windows(records, k, W, S)
        for a in want:
            a.setflags(write=False)
        _cases[(k, S)] = (records, want)
    return _cases[(k, S)]


@pytest.mark.parametrize("S", [1, W // 2, W])
@pytest.mark.parametrize("k", [1, 6, 12])
def test_translate_windows_equals_restatement(capi, k, S):
    from tetrex_amd import host
    records, (want_off, want_woff, want_beg, want_len) = case(k, S)
    codes = host.peptide_codes(0)
    values, offsets, win_offsets, begins, lens = capi.translate_windows(records, k, codes, W, S)
    tv, to = capi.translate(records, k, codes)
    assert np.array_equal(offsets, to) and np.array_equal(values, tv)
    assert np.array_equal(offsets, want_off)
    assert np.array_equal(win_offsets, want_woff)
    assert begins.size == capi.translate_windows_bound(np.concatenate([[0], np.cumsum([len(r) for r in records])]), k, W, S)
    assert np.array_equal(begins, want_beg), np.flatnonzero(begins != want_beg)[:10]
    assert np.array_equal(lens, want_len), np.flatnonzero(lens != want_len)[:10]
    ends = begins + lens.astype(np.uint64)
    assert (np.diff(begins.astype(np.int64)) >= 0).all() and (np.diff(ends.astype(np.int64)) >= 0).all()
    assert int(ends.max()) <= values.size
    assert (lens == 0).any() and int(lens.max()) == W - k + 1  # (non-vacuity: empty windows and stop-free ones)


def test_translate_windows_small_batches_and_alignments(capi):
    from tetrex_amd import host
    codes = host.peptide_codes(1)
    v, o, wo, b, n = capi.translate_windows([], 6, codes, W, 10)
    assert v.size == 0 and np.array_equal(o, [0]) and np.array_equal(wo, [0]) and b.size == 0 and n.size == 0
    v, o, wo, b, n = capi.translate_windows(["", "AC", ""], 6, codes, W, 10)
    assert v.size == 0 and np.array_equal(wo, np.zeros(19)) and b.size == 0
    rng = np.random.default_rng(9)
    body = random_nt(rng, 900, 0.01)
    want = F.translate_windows([body[:400], body[400:]], 4, 9, 4)
    for pad in (0, 1, 5, 15, 16):  # records that do not start at byte 0 of the buffer
        seq = np.frombuffer(("G" * pad + body).encode(), dtype=np.uint8)
        rec = np.array([pad, pad + 400, pad + 900], dtype=np.uint64)
        got = capi.translate_windows((seq, rec), 4, codes, 9, 4)
        for g, w in zip(got[1:], want):
            assert np.array_equal(g, w), pad


def _device_windows(capi, records, k, codes, S):
    """txq_translate_windows_device on device buffers; returns the buffers, left on the device, and the window count"""
    seq, rec = capi._records(records)
    n = rec.size - 1
    bound, n_win = capi.translate_bound(rec, k), capi.translate_windows_bound(rec, k, W, S)
    d = dict(seq=capi.DeviceBuffer.from_numpy(np.concatenate([seq, np.zeros(16, dtype=np.uint8)])), rec=capi.DeviceBuffer.from_numpy(rec),
             codes=capi.DeviceBuffer.from_numpy(np.asarray(codes, dtype=np.uint8)), val=capi.DeviceBuffer(8 * bound + 8),
             off=capi.DeviceBuffer(8 * (6 * n + 1)), woff=capi.DeviceBuffer(8 * (6 * n + 1)), beg=capi.DeviceBuffer(8 * n_win + 8),
             len=capi.DeviceBuffer(4 * n_win + 8))
    capi.check(capi.lib().txq_translate_windows_device(d["seq"].ptr, d["rec"].ptr, n, k, d["codes"].ptr, W, S, d["val"].ptr, d["off"].ptr, d["woff"].ptr,
                                                       d["beg"].ptr, d["len"].ptr, None))
    return d, n_win


@pytest.mark.parametrize("kind", ["flat", "hibf"])
@pytest.mark.parametrize("k,S", [(6, W // 2), (12, 1)])
def test_device_arrays_go_straight_into_count_windows(capi, oracle, kind, k, S):
    from tetrex_amd import host
    records, _ = case(k, S)
    codes = host.peptide_codes(0)
    if kind == "flat":
        ix = capi.Index.upload_ibf(200, 257, 2, random_words(200, 257, 0.5, 11))
    else:
        ox, descs, tv = layout_hibf(oracle, 5, user_bins=900, tmax=64, n_values=30)
        ix = capi.Index.upload_hibf(900, descs)
    d, n_win = _device_windows(capi, records, k, codes, S)
    capi.synchronize()
    lens = d["len"].to_numpy(np.uint32, (n_win,))
    begins = d["beg"].to_numpy(np.uint64, (n_win,))
    n_values = int(d["off"].to_numpy(np.uint64, (6 * len(records) + 1,))[-1])
    values = d["val"].to_numpy(np.uint64, (n_values,))
    thr = np.maximum(1, lens // 4).astype(np.uint32)
    d_thr = capi.DeviceBuffer.from_numpy(thr)
    words = ix.shard_words
    d_hits, d_counts = capi.DeviceBuffer(8 * n_win * words), capi.DeviceBuffer(4 * n_win * words * 64)
    ix.count_windows_device(d["val"].ptr, d["beg"].ptr, d["len"].ptr, n_win, d_thr.ptr, d_hits.ptr, d_counts.ptr)
    capi.synchronize()
    hits = d_hits.to_numpy(np.uint64, (n_win, words))
    counts = d_counts.to_numpy(np.uint32, (n_win, words * 64))
    ev, eo = csr([values[int(b):int(b) + int(n)] for b, n in zip(begins, lens)])
    want_hits, want_counts = ix.count(ev, eo, thr, counts=True)
    assert np.array_equal(hits, want_hits) and np.array_equal(counts, want_counts)
    if kind == "flat":
        assert hits.any() and not (hits[:, 0] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    # a sub-range of the windows, begins still absolute: the same rows
    j0, j1 = n_win // 3, n_win // 3 + 50
    ix.count_windows_device(d["val"].ptr, d["beg"].ptr + 8 * j0, d["len"].ptr + 4 * j0, j1 - j0, d_thr.ptr + 4 * j0, d_hits.ptr, d_counts.ptr)
    capi.synchronize()
    assert np.array_equal(d_hits.to_numpy(np.uint64, (j1 - j0, words)), want_hits[j0:j1])
    assert np.array_equal(d_counts.to_numpy(np.uint32, (j1 - j0, words * 64)), want_counts[j0:j1])
    for b in list(d.values()) + [d_thr, d_hits, d_counts]:
        b.free()
    ix.free()


def test_refusals(capi):
    """What the library refuses, before anything is launched: every call returns -1 and leaves the buffers alone."""
    from tetrex_amd import host
    L = capi.lib()
    u64p, u32p = capi.u64p, capi.u32p
    codes = np.ascontiguousarray(host.peptide_codes(0), dtype=np.uint8)
    seq, rec = capi._records(["ACGT" * 100, "GATTACA" * 30])

    def call(k=6, window=W, step=10, rec=rec, codes=codes, with_offsets=True, with_win_offsets=True, with_begins=True, with_lens=True):
        values = np.full(2000, 0xABCD, dtype=np.uint64)
        offsets = np.full(13, 0xABCD, dtype=np.uint64)
        woff = np.full(13, 0xABCD, dtype=np.uint64)
        beg = np.full(2000, 0xABCD, dtype=np.uint64)
        ln = np.full(2000, 0xABCD, dtype=np.uint32)
        rc = L.txq_translate_windows(seq.ctypes.data, rec.ctypes.data_as(u64p) if rec is not None else None, 2, k,
                                     codes.ctypes.data if codes is not None else None, window, step, values.ctypes.data_as(u64p),
                                     offsets.ctypes.data_as(u64p) if with_offsets else None, woff.ctypes.data_as(u64p) if with_win_offsets else None,
                                     beg.ctypes.data_as(u64p) if with_begins else None, ln.ctypes.data_as(u32p) if with_lens else None)
        capi.synchronize()
        untouched = all((a == 0xABCD).all() for a in (values, offsets, woff, beg, ln))
        assert untouched or rc == 0
        return rc

    assert call() == 0
    assert call(k=0) == -1 and call(k=13) == -1
    assert call(window=5) == -1                      # window < k
    assert call(step=0) == -1 and call(step=W + 1) == -1
    assert call(rec=None) == -1 and call(codes=None) == -1
    assert call(with_offsets=False) == -1 and call(with_win_offsets=False) == -1
    assert call(with_begins=False) == -1 and call(with_lens=False) == -1
    assert call(rec=np.array([0, 400, 300], dtype=np.uint64)) == -1  # descending record offsets
    d = capi.DeviceBuffer(256)
    for args in [(d.ptr, d.ptr, 1, 6, d.ptr, 5, 1, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, None),       # window < k
                 (d.ptr, d.ptr, 1, 6, d.ptr, 40, 41, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, None),     # step > window
                 (d.ptr, d.ptr, 1, 13, d.ptr, 40, 10, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, None),    # k
                 (d.ptr, d.ptr, 1, 6, d.ptr, 40, 10, d.ptr, d.ptr, None, d.ptr, d.ptr, None),      # no window offsets
                 (d.ptr, d.ptr, 1, 6, d.ptr, 40, 10, d.ptr, d.ptr, d.ptr, None, d.ptr, None),
                 (d.ptr, d.ptr, 1, 6, d.ptr, 40, 10, d.ptr, d.ptr, d.ptr, d.ptr, None, None)]:
        assert L.txq_translate_windows_device(*args) == -1
    d.free()
    with pytest.raises(capi.TxqError) as e:
        capi.translate_windows(["ACGT" * 30], 6, codes, 5, 1)
    assert e.value.code == -1
