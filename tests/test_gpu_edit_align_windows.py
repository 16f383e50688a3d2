"""GPU parity of window alignments (include/txq.h txq_edit_align_windows / txq_edit_align_windows_device): every
word of every answer against tetrex_amd.host.edit_align (txh_edit_align) on the windows WRITTEN OUT as patterns and the views'
records as the groups of one text, which is how the header defines the result; a sample against the full matrix of
tests/edit_align_ref.py.  The triples come from tetrex_amd.host.edit_search on the written-out windows, with the record index
counted inside the view as the call takes it."""
import numpy as np
import pytest

import edit_align_ref as A
import edit_cases
import edit_ref as E

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 63, 64, 65, 511, 512]  # either side of a block of 64 rows, and the 512 rows of the one instance
DISTANCES = [0, 1, 5, 31]
MAX_ERRORS = 31
STRIDE = 2 * MAX_ERRORS + 3
FILL = 0xA5A5A5A5
NONE3 = [E.NONE] * 3
MARKER = [0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFE]


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def host():
    from tetrex_amd import host as h
    return h


def _substituted(letters, p, d):
    """d substitutions at evenly spaced places: distance d to p unless chance offers less"""
    s = bytearray(p)
    for at in (np.arange(d) * len(p) // max(d, 1)).tolist():
        s[at] = ord(letters[(letters.index(chr(s[at]).upper()) + 1) % len(letters)])
    return bytes(s)


def _written(letters, wb, wl):
    return [bytes(letters[int(b):int(b) + int(n)]) for b, n in zip(wb, wl)]


def _flat(texts):
    """the views' records as the groups of one text: (records, group offsets)"""
    records, groups = [], [0]
    for t in texts:
        records += list(t)
        groups.append(len(records))
    return records, groups


def _triples(host, letters, wb, wl, texts, pairs, codes):
    """what a search answers for every (window, view), r counted inside the view; and the same with r counted over all records"""
    records, groups = _flat(texts)
    flat = host.edit_search(_written(letters, wb, wl), records, groups, pairs, codes, threads=8)
    local = flat.copy()
    for i, (_, g, _) in enumerate(pairs):
        if flat[i, 0] != E.NONE:
            local[i, 1] -= groups[g]
    return local, flat


def _want(host, letters, wb, wl, texts, pairs, flat, codes, max_errors):
    records, groups = _flat(texts)
    return host.edit_align(_written(letters, wb, wl), records, groups, pairs, flat, codes, max_errors, threads=8, raw=True)


def _build(alphabet, m, seed):
    """One letter buffer and three views for windows of m letters.
    Letters: m + 1 random letters — windows a at 0 and a' at 1 overlap in all but one letter —, then windows b, c, e, f of m letters
    each, f ending exactly at the buffer's end; the window arrays list them in DESCENDING order of their begin.
    View 0: ONE record, a copy of f under 5 substitutions at its very end (the match ends at the last text byte).
    View 1: SEVEN records: two empty ones in front of the target, which holds the exact copy of a at byte 0 of the text (the band is
    clipped there), then copies of a' (1 substitution, inside), b (5, inside), c (31 substitutions, at its end) and e (a mix of 31
    edits).
    View 2: NO records; its pairs carry "none".
    Every window meets views 0 and 1 — the same window in two pairs against two views — and view 2."""
    letters = edit_cases.ALPHABETS[alphabet]
    rng = np.random.default_rng(seed)
    text = lambda n: edit_cases.random_text(rng, letters, n, junk=0).tobytes()
    buf = text(m + 1) + b"".join(text(m) for _ in range(4))
    begins = [0, 1] + [m + 1 + q * m for q in range(4)]
    wb, wl = begins[::-1], [m] * 6  # f, e, c, b, a', a
    f, e, c, b, a1, a = _written(buf, wb, wl)
    mixed = lambda p, d: edit_cases.edited(rng, letters, np.frombuffer(p, np.uint8), min(d, m)).tobytes()
    side = lambda: text(int(rng.integers(1, 80))) if m > 2 else b""  # (no letters around a copy of one or two letters: they would hold it by chance)
    view0 = [side() + _substituted(letters, f, min(5, m))]
    # (behind the copy of a a letter that a' does not end with: a', which is a without its first letter and one more, is 1 edit away)
    other = letters[(letters.index(chr(buf[m]).upper()) + 1) % len(letters)].encode()
    view1 = [b"", b"", a + other + side(), side() + _substituted(letters, a1, min(1, m)) + side(), side() + _substituted(letters, b, min(5, m)) + side(),
             side() + _substituted(letters, c, min(31, m)), side() + mixed(e, 31) + side()]
    texts = [view0, view1, []]
    pairs = [(w, g, 31) for w in range(6) for g in (1, 0)] + [(w, 2, 31) for w in range(6)]  # (cap 31: what the device aligns)
    return buf, wb, wl, texts, pairs, E.letter_codes(letters)


@pytest.fixture(scope="module")
def parity_cases(host):
    """inputs, triples and the host twin's words, computed once per (alphabet, m)"""
    out = {}
    for alphabet in edit_cases.ALPHABETS:
        for m in LENGTHS:
            buf, wb, wl, texts, pairs, codes = case = _build(alphabet, m, seed=7 * m + len(alphabet))
            assert len(texts[0]) == 1 and len(texts[1]) == 7 and len(texts[2]) == 0 and wb[0] + wl[0] == len(buf) and wb == sorted(wb, reverse=True)
            local, flat = _triples(host, buf, wb, wl, texts, pairs, codes)
            out[alphabet, m] = (case, local, _want(host, buf, wb, wl, texts, pairs, flat, codes, MAX_ERRORS))
    return out


def _differing(got, want, pairs, results):
    bad = np.flatnonzero((got != want).any(axis=1))
    return [(tuple(pairs[i]), results[i].tolist(), got[i, :8].tolist(), want[i, :8].tolist()) for i in bad[:4]], bad.size


@pytest.mark.parametrize("m", LENGTHS)
@pytest.mark.parametrize("alphabet", list(edit_cases.ALPHABETS))
def test_parity_with_host_twin(capi, parity_cases, alphabet, m):
    (buf, wb, wl, texts, pairs, codes), results, want = parity_cases[alphabet, m]
    got = capi.edit_align_windows(buf, wb, wl, texts, pairs, results, codes, MAX_ERRORS, raw=True)
    assert _differing(got, want, pairs, results) == ([], 0)
    # the _device form: letters and every text at odd offsets behind a 16-byte boundary, the answers between guard bytes
    dev = capi.edit_align_windows_device(buf, wb, wl, texts, pairs, results, codes, MAX_ERRORS, letters_at=3, text_at=5, guard=64)
    assert (dev[:64] == 0xA5).all() and (dev[-64:] == 0xA5).all()
    assert _differing(dev[64:-64].view(np.uint32).reshape(len(pairs), STRIDE), want, pairs, results) == ([], 0)
    starts, runs = capi.decode_alignments(got, MAX_ERRORS)
    written, seen = _written(buf, wb, wl), set()
    for (w, g, _), (d, r, j), start, rr in zip(pairs, results.tolist(), starts.tolist(), runs):
        if d == E.NONE:  # view 2 has no records; views 0 and 1 hold nothing within the cap for most windows that have no copy there
            assert start == E.NONE and rr == []
            continue
        assert g < 2
        assert d <= min(m, MAX_ERRORS) and start < capi.EDIT_ALIGN_DECLINED  # every pair was aligned on the device
        A.check_identities(m, d, j, start, rr)
        seen.add(d)
        if m <= 65:
            assert (d, j, start, rr) == A.align(written[w], texts[g][r], codes, j)
    # the copies as planted: a at byte 0 of view 1's text, f ending at view 0's last byte
    assert results[10].tolist() == [0, 2, m] and starts[10] == 0
    if m >= 63:
        assert results[1].tolist() == [5, 0, len(texts[0][0])]
    # every distance at every length that can have it (one or two letters match by chance; four letters seldom leave 31 edits 31
    # apart in 65 letters or fewer)
    assert set(d for d in DISTANCES if d == 0 or (m >= 63 and (d < 31 or m >= 511 or alphabet == "peptide"))) <= seen, seen


def _planted(m, d, alphabet="peptide", seed=3):
    """one window of m letters in a buffer of its own, one view whose one record holds it under d substitutions"""
    letters = edit_cases.ALPHABETS[alphabet]
    rng = np.random.default_rng(seed + m)
    p = edit_cases.random_text(rng, letters, m, junk=0).tobytes()
    return p, [b"WWW" + _substituted(letters, p, d) + b"YY"], E.letter_codes(letters)


def test_long_window_and_distance_32_are_declined(capi, host):
    """m = 513 and d = 32: the marker, and not one word more, from both forms; the host twin answers such a pair"""
    p513, rec513, codes = _planted(513, 3)
    p64, rec32, _ = _planted(64, 32)
    _, rec31, _ = _planted(64, 31)
    buf, wb, wl, texts = p513 + p64, [0, 513, 513], [513, 64, 64], [rec513, rec32, rec31]
    pairs = [(0, 0, 40), (1, 1, 40), (2, 2, 40)]
    local, flat = _triples(host, buf, wb, wl, texts, pairs, codes)
    assert local.tolist() == [[3, 0, 516], [32, 0, 67], [31, 0, 67]]
    want = _want(host, buf, wb, wl, texts, pairs, flat, codes, 40)
    assert want[:, 0].tolist() == [3, 3, 3]  # the host twin aligns all three
    declined = [capi.EDIT_ALIGN_DECLINED] + [FILL] * 82
    got = capi.edit_align_windows(buf, wb, wl, texts, pairs, local, codes, 40, raw=True)
    assert got[0].tolist() == declined and got[1].tolist() == declined and got[2].tolist() == want[2].tolist()
    dev = capi.edit_align_windows_device(buf, wb, wl, texts, pairs, local, codes, 40, guard=64)
    assert (dev[:64] == 0xA5).all() and (dev[-64:] == 0xA5).all()
    assert dev[64:-64].view(np.uint32).reshape(3, 83).tolist() == [declined, declined, want[2].tolist()]
    # "none" for a window above the limit is still "none"; d within the device's limit but above max_errors is declined
    got = capi.edit_align_windows(buf, wb, wl, texts, [(0, 0, 40), (2, 2, 40)], [NONE3, local[2].tolist()], codes, 30, raw=True)
    assert got.tolist() == [[E.NONE, 0] + [0] * 61, [capi.EDIT_ALIGN_DECLINED] + [FILL] * 62]


def test_refusals_markers_and_garbage_triples(capi, host):
    """Every refusal of the header — a window index or a view index out of range, an empty window, a window that leaves the
    letters by its length or by its begin —; "none" and the refusal marker passed on; triples that are no cell of the pair's
    matrix — r out of the view, offsets that leave the text or descend, j beyond the record, d > m, a wrong d —; the others are
    answered, the guard bytes stay, and the library is usable afterwards."""
    codes = E.letter_codes("ACGT")
    buf = "TTACGTACGTCC"
    wb, wl = [2, 2, 11, 13, 2 ** 64 - 3, 2], [8, 0, 2, 1, 8, 8]
    good_view = ["", "GGACGTACGTGG", "ACG"]
    leaves = (np.frombuffer(b"GGACGTACGTGG", np.uint8), np.array([0, 40], np.uint64))       # its one record ends beyond text_bytes
    descends = (np.frombuffer(b"GGACGTACGTGG", np.uint8), np.array([0, 12, 10, 12], np.uint64))
    texts = [good_view, leaves, descends, []]
    hit = [0, 1, 10]
    cases = [((0, 0, 2), hit, "good"), ((5, 0, 2), hit, "good"), ((0, 0, 2), NONE3, "none"), ((0, 0, 2), MARKER, "refused"),
             ((6, 0, 2), hit, "refused"), ((0xFFFFFFFF, 0, 2), hit, "refused"), ((0, 4, 2), hit, "refused"), ((0, 0xFFFFFFFF, 2), hit, "refused"),
             ((1, 0, 2), hit, "refused"), ((2, 0, 2), hit, "refused"), ((3, 0, 2), hit, "refused"), ((4, 0, 2), hit, "refused"),
             ((0, 0, 2), [0, 3, 10], "declined"), ((0, 0, 2), [0, 0xFFFFFFF0, 10], "declined"), ((0, 3, 2), [0, 0, 0], "declined"),
             ((0, 1, 2), [0, 0, 10], "declined"), ((0, 2, 2), [0, 1, 1], "declined"), ((0, 0, 2), [0, 1, 13], "declined"),
             ((0, 0, 2), [0, 1, 0xFFFFFFFF], "declined"), ((0, 0, 2), [9, 1, 10], "declined"), ((0, 0, 2), [1, 1, 10], "declined"),
             ((0, 0, 2), [0, 2, 3], "declined"), ((0, 0, 2), [3, 1, 10], "declined"), ((0, 3, 2), NONE3, "none"), ((0, 2, 2), [0, 0, 10], "good")]
    pairs, triples = [c[0] for c in cases], [c[1] for c in cases]
    buf_out = capi.edit_align_windows_device(buf, wb, wl, texts, pairs, triples, codes, 2, letters_at=1, text_at=7, guard=256)
    assert (buf_out[:256] == 0xA5).all() and (buf_out[-256:] == 0xA5).all()
    got = buf_out[256:-256].view(np.uint32).reshape(len(pairs), 7).tolist()
    words = {"good": [2, 1, 8 << 2, 0, 0, 0, 0], "none": [E.NONE, 0, 0, 0, 0, 0, 0], "refused": [E.NONE, 0xFFFFFFFE, 0, 0, 0, 0, 0],
             "declined": [capi.EDIT_ALIGN_DECLINED] + [FILL] * 6}
    assert [i for i, c in enumerate(cases) if got[i] != words[c[2]]] == []
    # the host twin says the same of the pairs it can be asked about: those of the view whose offsets are in order
    ask = [i for i, ((w, g, _), _, _) in enumerate(cases) if g == 0 and w in (0, 5)]
    want = _want(host, buf.encode(), [wb[0], wb[5]], [8, 8], [good_view], [(0 if cases[i][0][0] == 0 else 1, 0, 2) for i in ask],
                 np.array([[t[0], t[1], t[2]] for t in (triples[i] for i in ask)], dtype=np.uint32), codes, 2)
    assert want.tolist() == [got[i] for i in ask]
    # the host-buffer form refuses the whole call for what it can see, and nothing is launched
    starts, runs = capi.edit_align_windows(buf, wb, wl, [good_view], [(0, 0, 2)], [hit], codes, 2)
    assert starts.tolist() == [2] and runs == [[("=", 8)]]
    for bad in [(6, 0, 2), (0, 1, 2), (1, 0, 2), (2, 0, 2), (3, 0, 2), (4, 0, 2)]:
        with pytest.raises(capi.TxqError):
            capi.edit_align_windows(buf, wb, wl, [good_view], [bad], [hit], codes, 2)
    for bad_view in (leaves, descends):
        with pytest.raises(capi.TxqError):
            capi.edit_align_windows(buf, wb, wl, [good_view, bad_view], [(0, 0, 2)], [hit], codes, 2)
    with pytest.raises(capi.TxqError):
        capi.edit_align_windows(buf, wb, wl, [good_view], [(0, 0, 2)], [hit], codes, (1 << 24) + 1, raw=True)
    assert capi.lib().txq_edit_align_windows_device(None, 0, None, None, 0, None, 0, None, 1, None, None, 2, None, None, None) == -1  # TXQ_ERR_ARG


@pytest.mark.parametrize("n_pairs", [0, 1, 1300])
def test_grid(capi, parity_cases, n_pairs):
    """no pair, one pair, and more blocks than there are CUs, so that blocks queue behind one another: pair i of the call is pair
    i mod 18 of the parity case"""
    (buf, wb, wl, texts, pairs, codes), results, want = parity_cases["peptide", 65]
    rows = [i % len(pairs) for i in range(n_pairs)]
    dev = capi.edit_align_windows_device(buf, wb, wl, texts, [pairs[i] for i in rows], results[rows].reshape(-1, 3), codes, MAX_ERRORS, letters_at=9, text_at=15)
    assert (dev[:64] == 0xA5).all() and (dev[-64:] == 0xA5).all() and dev.size == 128 + 4 * STRIDE * n_pairs
    assert (dev[64:dev.size - 64].view(np.uint32).reshape(n_pairs, STRIDE) == want[rows].reshape(n_pairs, STRIDE)).all()
    if n_pairs:
        got = capi.edit_align_windows(buf, wb, wl, texts, [pairs[i] for i in rows], results[rows], codes, MAX_ERRORS, raw=True)
        assert (got == want[rows]).all()


def test_on_a_stream(capi, parity_cases):
    """the call queued on a stream of torch's making"""
    import torch
    (buf, wb, wl, texts, pairs, codes), results, want = parity_cases["dna", 512]
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    out = capi.edit_align_windows_device(buf, wb, wl, texts, pairs, results, codes, MAX_ERRORS, letters_at=7, text_at=11, stream=stream.cuda_stream)
    assert (out[:64] == 0xA5).all() and (out[-64:] == 0xA5).all()
    assert _differing(out[64:-64].view(np.uint32).reshape(len(pairs), STRIDE), want, pairs, results) == ([], 0)
