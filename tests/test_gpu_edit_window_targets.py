"""GPU parity of the per-record hit list of windows against a table of text views (include/txq.h txq_edit_window_targets /
txq_edit_window_targets_device).  The reference is never the code under test: every hit list is compared with
tetrex_amd.host.edit_search (txh_edit_search, which tests/test_edit_cpu.py holds to the O(mn) table) on the windows WRITTEN OUT as
patterns and every record of every view as a group of its own — tests/edit_targets_ref.py —, and the least hit of every pair
with what capi.edit_search answers for the written-out window on the view's records as one group."""
import numpy as np
import pytest

import edit_cases
import edit_ref as E
import edit_targets_ref as T

pytestmark = pytest.mark.gpu

# the smallest shapes at which the word count of a window changes (64 | 65, 128 | 129, 256 | 257), and the limits
LENGTHS = [1, 63, 64, 65, 128, 129, 256, 257, 512]
REFUSED = 0xFFFFFFFE
GRID = 256 * 16  # txq_edit_window_targets.hip: kGridBlocks, the waves of the persistent grid
PEPTIDE = "ACDEFGHIKLMNPQRSTVWY"


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def host():
    from tetrex_amd import host as h
    return h


def _bytes(x):
    return x.tobytes() if isinstance(x, np.ndarray) else (x.encode() if isinstance(x, str) else bytes(x))


def _reference(host, letters, wb, wl, texts, pairs, codes, valid=None):
    """the hit list of the pairs `valid` (default: all) from the host search: window written out, one-record groups; r counted
    inside the view, the pair numbered as in `pairs`"""
    letters = _bytes(letters)
    valid = list(range(len(pairs))) if valid is None else list(valid)
    records, groups = [], [0]
    for t in texts:
        records += [_bytes(r) for r in t]
        groups.append(len(records))
    patterns = [letters[int(wb[pairs[i][0]]):int(wb[pairs[i][0]]) + int(wl[pairs[i][0]])] for i in valid]
    written = [(k, pairs[i][1], pairs[i][2]) for k, i in enumerate(valid)]
    single_groups, single, owner = T.expand(groups, written)
    if not single:
        return np.zeros((0, 4), dtype=np.uint32)
    hits = T.hits_of(host.edit_search(patterns, records, single_groups, single, codes, threads=8), owner)
    first = np.asarray([groups[written[k][1]] for k in hits[:, 0].tolist()], dtype=np.uint32)
    hits[:, 2] -= first
    hits[:, 0] = np.asarray(valid, dtype=np.uint32)[hits[:, 0]]
    return hits


def _same(got, want, note=None):
    assert got.shape == want.shape, (note, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (note, bad.size, [(got[i].tolist(), want[i].tolist()) for i in bad[:6]])


def _rows(buf, n, guard=64):
    return buf[guard:guard + 16 * n].view(np.uint32).reshape(-1, 4)


def _windowed(case, rng):
    """a case of edit_cases.build as (letters, window begins, window lengths, texts, pairs, codes): the patterns back to back in
    one buffer with 0..2 letters between them, the windows listed in shuffled order, every group a view"""
    patterns, records, groups, pairs, codes = case
    order = rng.permutation(len(patterns))
    window_of = np.empty(len(patterns), dtype=np.int64)
    buf, wb, wl = bytearray(b"xx"), [0] * len(patterns), [0] * len(patterns)
    for p, raw in enumerate(patterns):
        w = int(np.flatnonzero(order == p)[0])
        window_of[p] = w
        wb[w], wl[w] = len(buf), len(raw)
        buf += _bytes(raw) + b"ac"[:int(rng.integers(0, 3))]
    texts = [[_bytes(r) for r in records[groups[g]:groups[g + 1]]] for g in range(len(groups) - 1)]
    return bytes(buf), wb, wl, texts, [(int(window_of[p]), g, e) for p, g, e in pairs], codes


@pytest.fixture(scope="module")
def parity_cases(host):
    """inputs and reference hit lists of the parity tests, computed once per alphabet, with the conditions that keep the tests
    from passing on nothing checked where the fixture is built"""
    out = {}
    for alphabet in edit_cases.ALPHABETS:
        built = edit_cases.build(LENGTHS, alphabet, seed=57 + len(alphabet), long_bytes=3000)
        case = _windowed(built, np.random.default_rng(5))
        want = _reference(host, *case)
        n = len(case[4])
        counts = T.per_pair_counts(want, n)
        assert (counts >= 1).sum() >= n / 3 and (counts >= 2).sum() >= n / 5 and (counts == 0).sum() >= n / 10, (alphabet, n, counts)
        assert (want[:, 2] > 0).sum() > want.shape[0] / 4  # (hits in later records of a view)
        out[alphabet] = (case, want, built)
    return out


@pytest.mark.parametrize("chunk", [None, "64", "16"])
@pytest.mark.parametrize("alphabet", list(edit_cases.ALPHABETS))
def test_parity(capi, parity_cases, monkeypatch, alphabet, chunk):
    """windows on either side of every word count, 37 views with records of 0, 1, m - 1, m and some thousand bytes, empty records
    between records that have bytes, a view of no records, caps 0 .. m + 5 (m <= e included); with the default chunk, one of 64
    bytes and one of 16"""
    if chunk:
        monkeypatch.setenv("TXQ_EDIT_CHUNK", chunk)
    case, want, built = parity_cases[alphabet]
    hits, total, status = capi.edit_window_targets(*case)
    assert total == want.shape[0] and not status.any(), (total, want.shape, status)
    _same(hits, want)
    # the consistency rule: the least hit of a pair is what the search kernel answers for the written-out window
    patterns, records, groups, pairs, codes = built
    search = capi.edit_search([_bytes(p) for p in patterns], [_bytes(r) for r in records], groups, pairs, codes)
    least = T.least(hits, len(pairs))
    found = least[:, 0] != T.NONE
    least[found, 1] += np.asarray([groups[g] for _, g, _ in pairs], dtype=np.uint32)[found]
    assert np.array_equal(least, search)


def test_device_call_places_refuses_and_answers(capi, host):
    """the device entry point on buffers placed by the test: letters 3 bytes behind a boundary; four views at addresses of their
    own, every text 5 bytes behind a 16-byte boundary — an odd address —, one of them in an allocation that ends with its last
    byte, one with no records; a view whose offsets leave its text_bytes and one whose ends descend, both refused; windows of 513
    and of 0 letters, one that leaves letters_bytes, window and view indices out of range: each refused between pairs that are
    answered, nothing outside the rows written — and the twin answers the good pairs alike"""
    rng = np.random.default_rng(77)
    codes = E.letter_codes(PEPTIDE)
    body = edit_cases.random_text(rng, PEPTIDE, 700, junk=0)
    letters = body.tobytes()
    wb = [10, 0, 100, 40, 690, 3, 188]
    wl = [30, 513, 0, 65, 11, 512, 512]  # (window 4 leaves the 700 letters by one)
    copy = lambda w, edits: edit_cases.edited(rng, PEPTIDE, body[wb[w]:wb[w] + wl[w]], edits).tobytes()
    noise = lambda n: edit_cases.random_text(rng, PEPTIDE, n).tobytes()
    view0 = [noise(40) + copy(0, 1) + noise(9), b"", copy(3, 2), noise(3) + copy(0, 0), copy(5, 3) + noise(20)]
    view1 = [b"", copy(6, 1) + noise(600), copy(3, 0) + copy(0, 2)]
    view2 = [copy(0, 2), noise(50), copy(5, 0)]
    texts = [view0, view1, [], view2]
    flat2 = (np.frombuffer(b"".join(view2), dtype=np.uint8), np.cumsum([0] + [len(r) for r in view2]).astype(np.uint64))
    leaves = (flat2[0], flat2[1], flat2[0].size - 1)                                   # view 4: the last offset is beyond text_bytes
    descends = (flat2[0], np.asarray([60, 40, 30, 20], dtype=np.uint64), flat2[0].size)  # view 5: its ends descend
    pairs = [(0, 0, 2), (1, 0, 9), (3, 1, 2), (2, 0, 5), (0, 3, 2), (4, 0, 3), (5, 0, 4), (0, 4, 2), (6, 1, 1), (0, 2, 40), (9, 0, 1), (0, 5, 2),
             (3, 0, 2), (0, 6, 2), (0xFFFFFFFF, 0xFFFFFFFF, 1), (0, 1, 30), (5, 3, 0)]
    valid = [0, 2, 4, 6, 8, 9, 12, 15, 16]
    want = _reference(host, letters, wb, wl, texts, pairs, codes, valid)
    counts = T.per_pair_counts(want, len(pairs))
    # (every answered pair but the one on the view of no records has a hit; m <= e: every record of the view, the empty one included)
    assert all(counts[i] >= 1 for i in valid if i != 9) and counts[9] == 0 and counts[15] == 3 and counts[0] >= 2
    guard, all_texts = 64, texts + [leaves, descends]
    want_status = [0 if i in valid else REFUSED for i in range(len(pairs))]
    for capacity in (want.shape[0] + 4, 3):
        buf, total, status = capi.edit_window_targets_device(letters, wb, wl, all_texts, pairs, codes, capacity, letters_at=3, text_at=5, exact_end=(3,),
                                                             guard=guard)
        assert status.tolist() == want_status and total == want.shape[0], (status, total, want.shape)
        rows = min(capacity, want.shape[0])
        assert _rows(buf, rows).tolist() == want[:rows].tolist()
        assert (buf[:guard] == 0xA5).all() and (buf[guard + 16 * rows:] == 0xA5).all()
    # the twin checks first: every refusal is an error of the whole call, nothing launched ...
    for bad in (1, 3, 5, 10, 13, 14):
        with pytest.raises(capi.TxqError) as e:
            capi.edit_window_targets(letters, wb, wl, texts, [pairs[0], pairs[bad]], codes)
        assert e.value.code == -1
    with pytest.raises(capi.TxqError) as e:
        capi.edit_window_targets(letters, wb, wl, [view0, descends[:2]], [pairs[0]], codes)
    assert e.value.code == -1
    # ... and answers the good pairs as the device call did
    hits, total, status = capi.edit_window_targets(letters, wb, wl, texts, [pairs[i] for i in valid], codes)
    assert total == want.shape[0] and not status.any() and hits[:, 1:].tolist() == want[:, 1:].tolist()
    hits, total, status = capi.edit_window_targets(letters, wb, wl, texts, [], codes)
    assert total == 0 and hits.shape == (0, 4) and status.size == 0


def test_record_ends_in_chunks_on_chunk_and_unit_boundaries(capi, host, monkeypatch):
    """chunks of 16 bytes, units of 1024: records that end inside a chunk (1000), on a unit boundary (1024), on a chunk boundary
    (1024 + 48), empty ones there, one that fills a unit exactly, and windows cut from the last and first letters of each — a
    match that ends with its record, one that begins with it, and the letters on both sides of a boundary (no match)"""
    rng = np.random.default_rng(91)
    codes = E.letter_codes(PEPTIDE)
    sizes = (1000, 24, 48, 0, 0, 7, 969, 1024, 16, 0)
    records = [edit_cases.random_text(rng, PEPTIDE, n, junk=0).tobytes() for n in sizes]
    ends = np.cumsum(sizes).tolist()
    assert ends[0] % 16 and ends[1] == 1024 and ends[2] % 1024 and ends[2] % 16 == 0 and ends[6] == 2048 and ends[7] == 3072
    cuts = [records[0][-20:], records[1][-24:], records[2][:12], records[1][-8:] + records[2][:8], records[6][-30:], records[7][:40], records[7][-9:],
            records[8], records[7][-5:] + records[8][:5], records[5]]
    letters, wb, wl = b"".join(cuts), np.cumsum([0] + [len(c) for c in cuts])[:-1].tolist(), [len(c) for c in cuts]
    pairs = [(w, 0, e) for w in range(len(cuts)) for e in (0, 2)]
    want = _reference(host, letters, wb, wl, [records], pairs, codes)
    by = {(w, e): want[want[:, 0] == i][:, 1:].tolist() for i, (w, _, e) in enumerate(pairs)}
    assert by[0, 0] == [[0, 0, 1000]] and by[1, 0] == [[0, 1, 24]] and by[2, 0] == [[0, 2, 12]] and by[3, 2] == [] and by[4, 0] == [[0, 6, 969]]
    assert by[5, 0] == [[0, 7, 40]] and by[6, 0] == [[0, 7, 1024]] and by[7, 0] == [[0, 8, 16]] and by[8, 2] == [] and [0, 5, 7] in by[9, 0]
    for chunk in ("16", "64", None):
        if chunk:
            monkeypatch.setenv("TXQ_EDIT_CHUNK", chunk)
        else:
            monkeypatch.delenv("TXQ_EDIT_CHUNK")
        hits, total, status = capi.edit_window_targets(letters, wb, wl, [records], pairs, codes)
        assert total == want.shape[0] and not status.any()
        _same(hits, want, chunk)


def test_empty_records_and_caps_of_at_least_m(capi, host):
    """m <= e: every record of the view is a hit of distance at most m, an empty one the hit (m, r, 0); empty records first,
    between and last; and a view of no records"""
    codes = E.letter_codes("ACGT")
    p = "ACGTTGCAAC"
    records = ["", "", "GG" + p + "G", "", "TTTT", "", "", p[:6], ""]
    pairs = [(0, 0, 10), (0, 0, 11), (0, 0, 9), (0, 0, 4), (0, 1, 10), (0, 0, 0)]
    want = _reference(host, "tt" + p, [2], [10], [records, []], pairs, codes)
    first = want[want[:, 0] == 0][:, 1:].tolist()
    assert first == [[10, 0, 0], [10, 1, 0], [0, 2, 12], [10, 3, 0], [8, 4, 2], [10, 5, 0], [10, 6, 0], [4, 7, 6], [10, 8, 0]]
    assert (want[:, 0] == 4).sum() == 0 and want[want[:, 0] == 5][:, 1:].tolist() == [[0, 2, 12]]
    hits, total, status = capi.edit_window_targets("tt" + p, [2], [10], [records, []], pairs, codes)
    assert total == want.shape[0] and not status.any()
    _same(hits, want)


def test_capacity_and_slots(capi, parity_cases):
    """capacity below the total: the first rows and the true total; capacity 0 and capacity equal to the total; n_slots one
    short: the last pair that has records is refused, and what lies behind it; more slots than needed change nothing"""
    (letters, wb, wl, texts, pairs, codes), want, _ = parity_cases["dna"]
    pairs = pairs[:40] + pairs[-1:]  # (the last pair names the view of no records)
    want = want[want[:, 0] < 40]
    n = want.shape[0]
    assert n > 30
    fn = lambda pr, **kw: capi.edit_window_targets(letters, wb, wl, texts, pr, codes, **kw)
    for capacity in (n, n - 1, 7, 0):
        hits, total, status = fn(pairs, capacity=capacity)
        assert total == n and not status.any()
        _same(hits, want[:capacity], capacity)
    need = capi.edit_window_targets_slots(texts, pairs)
    assert need == sum(len(texts[g]) for _, g, _ in pairs)
    hits, total, status = fn(pairs, n_slots=need + 1000)
    assert total == n and not status.any()
    _same(hits, want)
    hits, total, status = fn(pairs, n_slots=need - 1)
    assert status.tolist() == [0] * 39 + [REFUSED, REFUSED]
    _same(hits, want[want[:, 0] < 39])
    assert total == (want[:, 0] < 39).sum()
    hits, total, status = fn(pairs[:40], n_slots=need - 1)
    assert status.tolist() == [0] * 39 + [REFUSED] and total == (want[:, 0] < 39).sum()
    _same(hits, want[want[:, 0] < 39])
    hits, total, status = fn(pairs, n_slots=0)
    assert total == 0 and hits.shape == (0, 4) and status.tolist() == [REFUSED] * 41


def test_device_call_on_a_stream(capi, parity_cases):
    """txq_edit_window_targets_device on a stream of torch's making, with the twin's result; nothing is waited for inside the call"""
    import torch
    (letters, wb, wl, texts, pairs, codes), _, _ = parity_cases["peptide"]
    pairs = pairs[40:120]
    hits, total, status = capi.edit_window_targets(letters, wb, wl, texts, pairs, codes)
    assert total > 40
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    buf, dev_total, dev_status = capi.edit_window_targets_device(letters, wb, wl, texts, pairs, codes, total + 5, stream=stream.cuda_stream)
    assert dev_total == total and not dev_status.any()
    assert _rows(buf, total).tolist() == hits.tolist()


def test_more_units_than_waves_and_more_pairs_than_a_block(capi, host, monkeypatch):
    """Chunks of 16 bytes: a view of 5 000 bytes is 5 units, so 1 100 pairs on ten such views are over 5 000 units — every wave of
    the 4 096 takes a second one, which belongs to a pair with another window and another view: Peq and the view's bounds are
    rebuilt between them — and the pairs are more than the 1 024 threads of a scan round and more than four plan blocks."""
    rng = np.random.default_rng(59)
    codes = E.letter_codes(PEPTIDE)
    lengths = [5, 64, 65, 128, 129, 256, 300, 512]
    windows = [edit_cases.random_text(rng, PEPTIDE, m, junk=0) for m in lengths]
    letters = b"".join(w.tobytes() for w in windows)
    wb, wl = np.cumsum([0] + lengths)[:-1].tolist(), lengths
    texts = []
    for g in range(10):
        n = int(rng.integers(1, 6))
        recs = [edit_cases.random_text(rng, PEPTIDE, int(rng.integers(4200, 5000)) // n) for _ in range(n)]
        for k in range(4):  # edited copies of four of the windows, each inside one record
            r = int(rng.integers(0, n))
            at = int(rng.integers(0, len(recs[r]) + 1))
            recs[r] = np.concatenate([recs[r][:at], edit_cases.edited(rng, PEPTIDE, windows[(g + 2 * k) % 8], (g + k) % 4), recs[r][at:]])
        texts.append([r.tobytes() for r in recs])
    pairs = [(int(rng.integers(0, 8)), int(rng.integers(0, 10)), int(rng.integers(0, 4))) for _ in range(1100)]
    units = np.array([-(-sum(len(r) for r in texts[g]) // (64 * 16)) for _, g, _ in pairs])
    assert units.sum() > GRID + 1000 and len(pairs) > 1024
    window_of_unit = np.repeat(np.array([w for w, _, _ in pairs]), units)
    assert float((window_of_unit[GRID:] != window_of_unit[:-GRID]).mean()) > 0.8  # a wave's next unit: another window
    want = _reference(host, letters, wb, wl, texts, pairs, codes)
    counts = T.per_pair_counts(want, len(pairs))
    late = np.unique(np.repeat(np.arange(len(pairs)), units)[GRID:])  # (pairs with units that are some wave's second one)
    assert (counts >= 1).sum() > len(pairs) // 5 and (counts == 0).sum() > len(pairs) // 5 and counts[late].sum() > 50 and counts[1024:].sum() > 10
    monkeypatch.setenv("TXQ_EDIT_CHUNK", "16")
    hits, total, status = capi.edit_window_targets(letters, wb, wl, texts, pairs, codes)
    assert total == want.shape[0] and not status.any()
    _same(hits, want)


def test_more_compaction_blocks_than_a_scan_round(capi, host):
    """a view of 2 700 records of 0 to 3 bytes and 100 pairs of windows of 1 to 8 letters on it: 270 000 slots, over 1 024
    blocks of 256 — the block prefix takes a second round of the one-workgroup scan — and hits in the blocks behind it"""
    rng = np.random.default_rng(61)
    codes = E.letter_codes("ACGT")
    records = [edit_cases.random_text(rng, "AC", int(rng.integers(0, 4)), junk=0).tobytes() for _ in range(2700)]
    letters = edit_cases.random_text(rng, "AC", 40, junk=0).tobytes()
    wb = [int(rng.integers(0, 32)) for _ in range(20)]
    wl = [int(rng.integers(1, 9)) for _ in range(20)]
    pairs = [(int(rng.integers(0, 20)), 0, int(rng.integers(0, 3))) for _ in range(100)]
    pairs = [(w, g, min(e, wl[w] - 1)) for w, g, e in pairs]  # (m > e: not every record a hit)
    assert len(pairs) * len(records) > 1024 * 256
    want = _reference(host, letters, wb, wl, [records], pairs, codes)
    counts = T.per_pair_counts(want, len(pairs))
    assert 1000 < want.shape[0] < 0.6 * len(pairs) * len(records) and counts[97:].sum() > 0, (want.shape, counts)
    hits, total, status = capi.edit_window_targets(letters, wb, wl, [records], pairs, codes)
    assert total == want.shape[0] and not status.any()
    _same(hits, want)
