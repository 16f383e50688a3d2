"""GPU parity of the windowed edit-distance call (include/txq.h txq_edit_windows / txq_edit_windows_device): every
(distance, record, end) against tests/edit_ref.py on the WRITTEN-OUT windows — the contract defines the result as what
txq_edit_search answers with window p written out as pattern p.  One small case holds every shape at which the kernel takes
another path: window lengths on either side of every word count, windows that overlap, repeat and lie at the first and the
last byte of the letter buffer, runs of compatible pairs of 1 .. 9 that begin at every i % K and are broken by a change of
group, of word count and by refused pairs, caps that change inside a run, a group of no records and empty records around
records; run at every bundle size and chunk."""
import numpy as np
import pytest

import edit_cases
import edit_ref as E

pytestmark = pytest.mark.gpu

LENGTHS = [1, 63, 64, 65, 128, 129, 256, 257, 512]
RUNS = [1, 3, 4, 5, 9, 2, 1]  # K - 1, K, K + 1 and 2 K + 1 for K = 4 and K = 2, and 1
REFUSED = [E.NONE, 0xFFFFFFFE, 0xFFFFFFFE]
LETTERS = "ACDEFGHIKLMNPQRSTVWY"


def words_of(m):
    return 1 if m <= 64 else 2 if m <= 128 else 4 if m <= 256 else 8


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


def _caps(m):
    return [0, 3, m - 1, 0, 3, m, 0, 3, m + 5]


@pytest.fixture(scope="module")
def case():
    """letters, windows, records, groups, the pair list without refused pairs (for the host-buffer call) and with them (for
    the _device call), and the reference results of both, computed once"""
    rng = np.random.default_rng(190)
    codes = E.letter_codes(LETTERS)
    A, B, C = (edit_cases.random_text(rng, LETTERS, n, junk=0.01) for n in (1500, 700, 900))
    empty = np.zeros(0, np.uint8)
    records = [empty, A, empty, empty, B, empty, C, empty, empty]
    groups = [0, 6, 7, 7, 9]  # group 2 has no records, group 3 two empty ones
    # the letters: stretches of A, C and B with about one edit in 40 letters, and random letters between them
    parts = [edit_cases.edited(rng, LETTERS, A[100:800], 17), edit_cases.random_text(rng, LETTERS, 550, junk=0.01), edit_cases.edited(rng, LETTERS, C[50:650], 15),
             edit_cases.random_text(rng, LETTERS, 560, junk=0.01), edit_cases.edited(rng, LETTERS, B[0:600], 15)]
    letters = np.concatenate(parts)
    L = letters.size
    win_begin, win_len, of_len = [], [], {}
    for m in LENGTHS:
        step = max(1, m // 3)  # (they overlap)
        begins = [0] + [int(b) for b in rng.integers(0, L - m, size=6)] + [L - m]  # the first and the last byte of the buffer
        begins += [begins[1] + step, begins[1] + 2 * step, begins[1]]             # overlapping neighbours, and one twice
        begins = [min(b, L - m) for b in begins]
        of_len[m] = list(range(len(win_begin), len(win_begin) + len(begins)))
        win_begin += begins
        win_len += [m] * len(begins)
    n_good = len(win_begin)
    bad_windows = {"leaves the letters": (L - 3, 4), "no letters": (5, 0), "too long": (0, 513), "begins behind the letters": (L + 1, 1)}
    win_begin += [b for b, _ in bad_windows.values()]
    win_len += [n for _, n in bad_windows.values()]
    # the pairs: for each length runs of RUNS compatible pairs over its windows; a run ends with a breaker — a change of group
    # (the next run is of group 1), a change of word count (a pair of another length) or, in `with_refused`, a refused pair
    pairs, with_refused = [], []
    for li, m in enumerate(LENGTHS):
        caps, at = _caps(m), 0
        other = of_len[LENGTHS[(li + 3) % len(LENGTHS)]][0]
        assert words_of(win_len[other]) != words_of(m)
        for ri, n in enumerate(RUNS):
            group = ri % 2  # (a change of group between runs)
            for _ in range(n):
                pair = (of_len[m][at % len(of_len[m])], group, caps[at % len(caps)])
                pairs.append(pair), with_refused.append(pair)
                at += 1
                if n == 9 and _ == 4:  # in the middle of the long run: a refused pair, which cuts the run for the _device call only
                    with_refused.append((n_good + ri % 4, group, 3))
            if ri % 3 == 1:  # same group on either side: a change of word count is what ends the run
                breaker = (other, group, 3)
                pairs.append(breaker), with_refused.append(breaker)
            if ri % 3 == 2:
                with_refused += [(of_len[m][0], 9, 3), (n_good + 4, 0, 3)]  # a group and a window out of range
        for g in (2, 3):  # a group of no records, a group of empty records: nothing but the empty match where m <= e
            for e in (3, m + 5):
                pairs.append((of_len[m][1], g, e)), with_refused.append((of_len[m][1], g, e))
    written = [letters[b:b + n].tobytes() for b, n in zip(win_begin[:n_good], win_len[:n_good])]
    want = E.search(written, records, groups, pairs, codes)
    ok = [i for i, (p, g, _) in enumerate(with_refused) if p < n_good and g < len(groups) - 1]
    want_refused = np.tile(np.array(REFUSED, dtype=np.uint32), (len(with_refused), 1))
    want_refused[ok] = E.search(written, records, groups, [with_refused[i] for i in ok], codes)
    return dict(letters=letters, win_begin=win_begin, win_len=win_len, n_good=n_good, records=[r.tobytes() for r in records], groups=groups, codes=codes,
                pairs=pairs, want=want, with_refused=with_refused, want_refused=want_refused)


def _differing(got, want, pairs):
    bad = np.flatnonzero((got != want).any(axis=1))
    return [(i, tuple(pairs[i]), got[i].tolist(), want[i].tolist()) for i in bad[:6]], bad.size


def test_the_case_holds_the_shapes(case):
    """what the generator promises, checked on the pair list itself (no device): runs of 1, K - 1, K, K + 1 and 2 K + 1
    compatible pairs for K = 2 and 4, a run that begins at i % K = K - 1, hits and non-hits in thirds"""
    pairs, wl = case["pairs"], case["win_len"]
    runs, start = [], 0
    for i in range(1, len(pairs) + 1):
        if i == len(pairs) or pairs[i][1] != pairs[i - 1][1] or words_of(wl[pairs[i][0]]) != words_of(wl[pairs[i - 1][0]]):
            runs.append((start, i - start))
            start = i
    assert {1, 2, 3, 4, 5, 9} <= {n for _, n in runs}
    assert any(s % 4 == 3 and n >= 2 for s, n in runs) and any(s % 2 == 1 and n >= 2 for s, n in runs)
    want = case["want"]
    hits = int((want[:, 0] != E.NONE).sum())
    assert hits * 3 >= len(pairs) and (len(pairs) - hits) * 3 >= len(pairs), (hits, len(pairs))
    assert {wl[p] for p, _, _ in pairs} == set(LENGTHS)
    refused = case["want_refused"][:, 1] == 0xFFFFFFFE
    assert refused.sum() >= 20 and (case["want_refused"][~refused, 0] != E.NONE).sum() * 3 >= len(refused)


@pytest.mark.parametrize("chunk", [None, "64", "16"])
@pytest.mark.parametrize("bundle", [None, "1", "2", "4"])
def test_parity_with_written_out_windows(capi, case, monkeypatch, bundle, chunk):
    if chunk:
        monkeypatch.setenv("TXQ_EDIT_CHUNK", chunk)
    if bundle:
        monkeypatch.setenv("TXQ_EDIT_WINDOWS_BUNDLE", bundle)
    n = case["n_good"]
    got = capi.edit_windows(case["letters"], case["win_begin"][:n], case["win_len"][:n], case["records"], case["groups"], case["pairs"], case["codes"])
    assert _differing(got, case["want"], case["pairs"]) == ([], 0)


def test_agrees_with_edit_search(capi, case):
    """the contract's own words: txq_edit_search with window p written out as pattern p"""
    n = case["n_good"]
    written = [case["letters"][b:b + m].tobytes() for b, m in zip(case["win_begin"][:n], case["win_len"][:n])]
    plain = capi.edit_search(written, case["records"], case["groups"], case["pairs"], case["codes"])
    got = capi.edit_windows(case["letters"], case["win_begin"][:n], case["win_len"][:n], case["records"], case["groups"], case["pairs"], case["codes"])
    assert np.array_equal(got, plain)


def _device_call(capi, case, pairs, stream=None, text_at=0):
    """txq_edit_windows_device on torch's buffers; the text begins text_at bytes behind a 16-byte boundary, letters around it"""
    import torch
    let, wb, wl, txt, ro, go, pr, cd = capi.edit_windows_arrays(case["letters"], case["win_begin"], case["win_len"], case["records"], case["groups"], pairs, case["codes"])
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).to(dev) for x in (let, wb, wl, ro, go, pr, cd)]
    around = torch.full((text_at + txt.size + 33,), ord("A"), dtype=torch.uint8, device=dev)
    text = around[text_at:text_at + txt.size]
    text.copy_(torch.from_numpy(txt.copy()).to(dev))
    assert text.data_ptr() % 16 == text_at
    out = torch.zeros(pr.shape[0] * 12, dtype=torch.uint8, device=dev)
    work = torch.empty(capi.edit_windows_workspace_bytes(pr.shape[0]) // 8, dtype=torch.int64, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(st):
        capi.check(capi.lib().txq_edit_windows_device(t[0].data_ptr(), let.size, t[1].data_ptr(), t[2].data_ptr(), wb.size, text.data_ptr(), t[3].data_ptr(),
                                                       ro.size - 1, txt.size, t[4].data_ptr(), go.size - 1, t[5].data_ptr(), pr.shape[0], t[6].data_ptr(),
                                                       out.data_ptr(), work.data_ptr(), st.cuda_stream))
    st.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(-1, 3)


@pytest.mark.parametrize("bundle", ["1", "2", "4"])
def test_device_call_on_a_stream_with_refused_pairs(capi, case, monkeypatch, bundle):
    """the _device call on a stream of torch's making: a refused pair — a window that leaves the letters, has none, too many,
    begins behind them, or an index out of range — gets the marker, in the middle of a run too, and its neighbours their answers"""
    import torch
    monkeypatch.setenv("TXQ_EDIT_WINDOWS_BUNDLE", bundle)
    monkeypatch.setenv("TXQ_EDIT_CHUNK", "64")
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    stream.wait_stream(torch.cuda.current_stream(torch.device("cuda:0")))
    got = _device_call(capi, case, case["with_refused"], stream=stream)
    assert _differing(got, case["want_refused"], case["with_refused"]) == ([], 0)


def test_text_that_is_not_16_byte_aligned(capi, case, monkeypatch):
    """the text 1, 7 and 15 bytes behind a 16-byte boundary, chunks of 16 bytes: the blocks at either end of the text are
    assembled from byte loads, and the bytes around the text are letters, so a block that took them in would change the answer"""
    monkeypatch.setenv("TXQ_EDIT_CHUNK", "16")
    for at in (0, 1, 7, 15):
        got = _device_call(capi, case, case["with_refused"], text_at=at)
        assert _differing(got, case["want_refused"], case["with_refused"]) == ([], 0), at


def test_refusals_leave_the_library_usable(capi, case):
    n = case["n_good"]
    args = (case["letters"], case["win_begin"], case["win_len"], case["records"], case["groups"])
    good = case["pairs"][:40]
    want = case["want"][:40]
    for bad in [(n, 0, 3), (n + 1, 0, 3), (n + 2, 0, 3), (n + 3, 0, 3), (n + 4, 0, 3), (0, 4, 3), (0xFFFFFFFF, 0xFFFFFFFF, 1)]:
        with pytest.raises(capi.TxqError) as e:
            capi.edit_windows(*args, good[:20] + [bad] + good[20:], case["codes"])
        assert e.value.code == -1, bad
        assert np.array_equal(capi.edit_windows(*args, good, case["codes"]), want), bad
    # what the _device call can see before it launches: no workspace
    let, wb, wl, txt, ro, go, pr, cd = capi.edit_windows_arrays(*args, good, case["codes"])
    bufs = [capi.DeviceBuffer.from_numpy(x) for x in (let, wb, wl, txt, ro, go, pr, cd)]
    out = capi.DeviceBuffer(len(good) * 12)
    try:
        assert capi.lib().txq_edit_windows_device(bufs[0].ptr, let.size, bufs[1].ptr, bufs[2].ptr, wb.size, bufs[3].ptr, bufs[4].ptr, ro.size - 1, txt.size,
                                                  bufs[5].ptr, go.size - 1, bufs[6].ptr, len(good), bufs[7].ptr, out.ptr, None, None) == -1
    finally:
        for b in bufs + [out]:
            b.free()
    assert np.array_equal(capi.edit_windows(*args, good, case["codes"]), want)
