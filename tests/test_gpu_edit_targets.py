"""GPU parity of the per-record hit list (include/txq.h txq_edit_targets / txq_edit_targets_long).  The
reference is never the code under test: every hit list is compared with tetrex_amd.host.edit_search (txh_edit_search, which
tests/test_edit_cpu.py holds to the O(mn) table) called with every record as a group of its own — tests/edit_targets_ref.py —,
and the least hit of every pair with what capi.edit_search / capi.edit_search_long answer on the real groups."""
import numpy as np
import pytest

import edit_cases
import edit_ref as E
import edit_targets_ref as T

pytestmark = pytest.mark.gpu

# the smallest shapes at which a word count (64 | 65, 128 | 129, 256 | 257), a group size (1024 | 1025, 2048 | 2049) or the
# kernel (512 | 513) changes
SHORT = [1, 64, 65, 128, 129, 256, 257, 512]
LONG = [513, 1024, 1025, 2048, 2049, 4095, 4096]
REFUSED = 0xFFFFFFFE


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


def _reference(host, case):
    """the hit list of a case from the search on one-record groups"""
    patterns, records, groups, pairs, codes = case
    single_groups, single, owner = T.expand(groups, pairs)
    if not single:
        return np.zeros((0, 4), dtype=np.uint32)
    return T.hits_of(host.edit_search(patterns, records, single_groups, single, codes, threads=8), owner)


@pytest.fixture(scope="module")
def parity_cases(host):
    """inputs and reference hit lists of the parity tests, computed once per kernel and alphabet, with the conditions that keep
    the tests from passing on nothing checked where the fixture is built"""
    out = {}
    for form, lengths in (("short", SHORT), ("long", LONG)):
        for alphabet in edit_cases.ALPHABETS:
            case = _raw(edit_cases.build(lengths, alphabet, seed=31 + len(alphabet), long_bytes=3000))
            want = _reference(host, case)
            counts = T.per_pair_counts(want, len(case[3]))
            n = len(case[3])
            assert (counts >= 1).sum() >= n / 3 and (counts >= 2).sum() >= n / 5 and (counts == 0).sum() >= n / 10, (form, alphabet, n, counts)
            out[form, alphabet] = (case, want)
    return out


def _same(got, want, note=None):
    assert got.shape == want.shape, (note, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (note, bad.size, [(got[i].tolist(), want[i].tolist()) for i in bad[:6]])


def _check(capi, fn, search, case, want, note=None):
    hits, total, status = fn(*case)
    assert total == want.shape[0] and not status.any(), (note, total, want.shape, status)
    _same(hits, want, note)
    # the consistency rule, against the search kernel on the same pairs
    assert np.array_equal(T.least(hits, len(case[3])), search(*case)), note


@pytest.mark.parametrize("chunk", [None, "64"])
@pytest.mark.parametrize("alphabet", list(edit_cases.ALPHABETS))
def test_short_parity(capi, parity_cases, monkeypatch, alphabet, chunk):
    """m on either side of every word count, records of 0, 1, m - 1, m and some thousand bytes, caps 0 .. m + 5, four groups per
    pattern and a group of no records; with the default chunk and with one shorter than every lead-in"""
    if chunk:
        monkeypatch.setenv("TXQ_EDIT_CHUNK", chunk)
    case, want = parity_cases["short", alphabet]
    _check(capi, capi.edit_targets, capi.edit_search, case, want)


@pytest.mark.parametrize("span", [None, "64", "16"])
@pytest.mark.parametrize("alphabet", list(edit_cases.ALPHABETS))
def test_long_parity(capi, parity_cases, monkeypatch, alphabet, span):
    if span:
        monkeypatch.setenv("TXQ_EDIT_LONG_SPAN", span)
    case, want = parity_cases["long", alphabet]
    _check(capi, capi.edit_targets_long, capi.edit_search_long, case, want)


@pytest.mark.parametrize("alphabet", list(edit_cases.ALPHABETS))
def test_short_patterns_on_the_long_kernel(capi, parity_cases, alphabet):
    case, want = parity_cases["short", alphabet]
    _check(capi, capi.edit_targets_long, capi.edit_search_long, case, want)


def _both(capi, monkeypatch, host, case, cuts=(None, "64", "16"), note=None):
    """a case of short patterns through both kernels, with the default cuts and with short ones"""
    want = _reference(host, case)
    for cut in cuts:
        if cut:
            monkeypatch.setenv("TXQ_EDIT_CHUNK", cut)
            monkeypatch.setenv("TXQ_EDIT_LONG_SPAN", cut)
        _check(capi, capi.edit_targets, capi.edit_search, case, want, (note, "short", cut))
        _check(capi, capi.edit_targets_long, capi.edit_search_long, case, want, (note, "long", cut))
    return want


def test_many_tiny_records(capi, host, monkeypatch):
    """a group of 300 records of 0 to 5 bytes: many flushes inside one chunk"""
    rng = np.random.default_rng(7)
    codes = E.letter_codes("ACGT")
    records = [edit_cases.random_text(rng, "AC", int(rng.integers(0, 6)), junk=0).tobytes() for _ in range(300)]
    patterns = ["A", "AC", "CAC", "ACCA", "AAAAA"]
    pairs = [(p, 0, e) for p in range(len(patterns)) for e in (0, 1, 2, len(patterns[p]))] + [(0, 1, 0)]
    want = _both(capi, monkeypatch, host, (patterns, records, [0, 300, 300], pairs, codes))
    counts = T.per_pair_counts(want, len(pairs))
    assert counts.max() == 300 and 0 < counts[0] < 300 and counts[-1] == 0 and np.unique(counts).size > 6, counts


def test_one_long_record_hit_from_several_units(capi, host, monkeypatch):
    """one record of 20 000 bytes; cuts of 100 letters with 0..3 substitutions inside that end on, one before and one behind
    multiples of 512 and 4096 (of chunks and spans, then, whatever their size here): one slot lowered from several units"""
    rng = np.random.default_rng(41)
    codes = E.letter_codes("ACGT")
    text = edit_cases.random_text(rng, "ACGT", 20_000, junk=0)
    swap = bytes.maketrans(b"ACGTacgt", b"CATGcatg")
    patterns, ends = [], []
    for base in (512, 4096, 4096 * 4, 512 * 9):
        for delta in (-1, 0, 1):
            end = base + delta
            cut = bytearray(text[end - 100:end].tobytes())
            for at in rng.integers(10, 90, size=int(rng.integers(0, 4))):
                cut[at:at + 1] = bytes(cut[at:at + 1]).translate(swap)
            patterns.append(bytes(cut))
            ends.append(end)
    pairs = [(i, 0, 3) for i in range(len(patterns))] + [(0, 0, 100), (1, 0, 0)]
    want = _both(capi, monkeypatch, host, (patterns, [text.tobytes()], [0, 1], pairs, codes), cuts=(None, "64"))
    assert want[:len(ends), 3].tolist() == ends and want.shape[0] >= len(ends) + 1 and (want[:, 2] == 0).all()


GRID = 256 * 16  # txq_edit.hip, txq_edit_long.hip, txq_edit_targets.hip: kGridBlocks, the waves of every persistent grid


def test_more_units_than_waves(capi, host, monkeypatch):
    """Chunks and spans of 16 bytes, 120 groups of 2 to 4 KiB, each paired with eight patterns of 5 to 512 letters (every word
    count of the short kernels) at three caps, pattern after pattern in shuffled order: about 9000 units of 1024 bytes for targets_kernel and
    edit_kernel and sixteen times as many of 64 bytes for targets_long_kernel<16> and edit_long_kernel<16>, so every wave of
    the 4096 takes a second and a third unit, and that unit belongs to a pair with another pattern: the pattern's match
    vectors in LDS are rebuilt between them."""
    letters = "ACDEFGHIKLMNPQRSTVWY"
    rng = np.random.default_rng(53)
    codes = E.letter_codes(letters)
    patterns = [edit_cases.random_text(rng, letters, m, junk=0) for m in (5, 64, 65, 128, 129, 256, 300, 512)]
    records, groups, pairs = [], [0], []
    for g in range(120):
        n = int(rng.integers(1, 6))
        recs = [edit_cases.random_text(rng, letters, int(rng.integers(2100, 4000)) // n) for _ in range(n)]
        for k, p in enumerate((g % 8, (g + 3) % 8, (g + 5) % 8)):  # edited copies of three of the patterns, each inside one record
            r = int(rng.integers(0, n))
            at = int(rng.integers(0, len(recs[r]) + 1))
            recs[r] = np.concatenate([recs[r][:at], edit_cases.edited(rng, letters, patterns[p], (g + k) % 4), recs[r][at:]])
        records += recs
        groups.append(len(records))
        pairs += [(int(p), g, e) for e in (0, 1, 3) for p in rng.permutation(len(patterns))]  # (in an order of its own: no period that 4096 units could fall in step with)
    size = [sum(len(r) for r in records[groups[g]:groups[g + 1]]) for g in range(120)]
    for per_unit in (64 * 16, (64 // 16) * 16):  # txq_text.hpp units_of(bytes, 64 lanes, chunk); txq_edit_long_plan.hpp long_units: 64 / G groups of one span, G = 16 up to 1024 letters
        units = np.array([-(-size[g] // per_unit) for _, g, _ in pairs])
        total = int(units.sum())
        assert total > 2 * GRID, (per_unit, total)  # edit_kernel, targets_kernel, ..._long_kernel: u < total, u += gridDim.x
        pattern_of_unit = np.repeat(np.array([p for p, _, _ in pairs]), units)  # pair_of_unit
        other = float((pattern_of_unit[GRID:] != pattern_of_unit[:-GRID]).mean())
        assert other > 0.8, other  # a wave's next unit: another pattern
    case = ([p.tobytes() for p in patterns], [r.tobytes() for r in records], groups, pairs, codes)
    want = _both(capi, monkeypatch, host, case, cuts=("16",))
    counts = T.per_pair_counts(want, len(pairs))
    assert (counts >= 1).sum() > len(pairs) // 5 and (counts == 0).sum() > len(pairs) // 5, counts
    late = np.repeat(np.arange(len(pairs)), units)[GRID:]  # (pairs with units that are some wave's second or later one)
    assert counts[np.unique(late)].sum() > 100


def test_records_that_begin_at_a_chunk_start(capi, host, monkeypatch):
    """chunks and spans of 64 bytes, records of 64, 128, 64, 0, 192, 0, 0 and 64 bytes: every record begins where a lane does"""
    rng = np.random.default_rng(43)
    codes = E.letter_codes("ACDEFGHIKLMNPQRSTVWY")
    records = [edit_cases.random_text(rng, "ACDEFGHIKLMNPQRSTVWY", n, junk=0).tobytes() for n in (64, 128, 64, 0, 192, 0, 0, 64)]
    # a record's first letters, its last ones, a whole record, the end of one with the start of the next (no match)
    patterns = [records[1][:20], records[4][-30:], records[2], records[0][-10:] + records[1][:10], records[7][:64], records[4][:1]]
    pairs = [(p, 0, e) for p in range(len(patterns)) for e in (0, 2, 9)]
    want = _both(capi, monkeypatch, host, (patterns, records, [0, 8], pairs, codes), cuts=("64",))
    by = {(p, e): want[want[:, 0] == i][:, 1:].tolist() for i, (p, _, e) in enumerate(pairs)}
    assert by[0, 0] == [[0, 1, 20]] and by[1, 0] == [[0, 4, 192]] and by[2, 0] == [[0, 2, 64]] and by[3, 9] == [] and by[4, 2] == [[0, 7, 64]]


def test_empty_records_and_caps_of_at_least_m(capi, host, monkeypatch):
    """m <= e: every record of the group is a hit of distance at most m, an empty one the hit (m, r, 0); empty records first,
    between and last; and a group of no records"""
    codes = E.letter_codes("ACGT")
    p = "ACGTTGCAAC"
    records = ["", "", "GG" + p + "G", "", "TTTT", "", "", p[:6], ""]
    groups = [0, 9, 9]  # (group 1 has no records)
    pairs = [(0, 0, 10), (0, 0, 11), (0, 0, 9), (0, 0, 4), (0, 1, 10), (0, 0, 0)]
    want = _both(capi, monkeypatch, host, ([p], records, groups, pairs, codes))
    first = want[want[:, 0] == 0][:, 1:].tolist()
    assert first == [[10, 0, 0], [10, 1, 0], [0, 2, 12], [10, 3, 0], [8, 4, 2], [10, 5, 0], [10, 6, 0], [4, 7, 6], [10, 8, 0]]
    assert want[want[:, 0] == 2][:, 1:].tolist() == [[0, 2, 12], [8, 4, 2], [4, 7, 6]] and want[want[:, 0] == 3][:, 1:].tolist() == [[0, 2, 12], [4, 7, 6]]
    assert (want[:, 0] == 4).sum() == 0 and want[want[:, 0] == 5][:, 1:].tolist() == [[0, 2, 12]]


@pytest.mark.parametrize("form", ["short", "long"])
def test_capacity_and_slots(capi, parity_cases, form):
    """capacity below the total: the first rows and the true total; capacity 0; n_slots one short: the last pair that has
    records is refused, the others are answered; more slots than needed change nothing"""
    fn = capi.edit_targets if form == "short" else capi.edit_targets_long
    (patterns, records, groups, pairs, codes), want = parity_cases[form, "dna"]
    pairs = pairs[:40] + pairs[-1:]  # (the last pair names the group of no records)
    want = want[want[:, 0] < 40]
    n = want.shape[0]
    assert n > 30
    for capacity in (n - 1, 7, 0):
        hits, total, status = fn(patterns, records, groups, pairs, codes, capacity=capacity)
        assert total == n and not status.any()
        _same(hits, want[:capacity], capacity)
    need = capi.edit_targets_slots(groups, pairs)
    assert need == sum(groups[g + 1] - groups[g] for _, g, _ in pairs)
    hits, total, status = fn(patterns, records, groups, pairs, codes, n_slots=need + 1000)
    assert total == n and not status.any()
    _same(hits, want)
    hits, total, status = fn(patterns, records, groups, pairs, codes, n_slots=need - 1)
    assert status.tolist() == [0] * 39 + [REFUSED, REFUSED]  # (what lies behind the pair that does not fit is refused with it)
    _same(hits, want[want[:, 0] < 39])
    assert total == (want[:, 0] < 39).sum()
    # ... and with the pair that does not fit the last one: that pair, and only it
    hits, total, status = fn(patterns, records, groups, pairs[:40], codes, n_slots=need - 1)
    assert status.tolist() == [0] * 39 + [REFUSED] and total == (want[:, 0] < 39).sum()
    _same(hits, want[want[:, 0] < 39])
    hits, total, status = fn(patterns, records, groups, pairs, codes, n_slots=0)
    assert total == 0 and hits.shape == (0, 4) and status.tolist() == [REFUSED] * 41


@pytest.mark.parametrize("form", ["short", "long"])
def test_device_call_refuses_what_its_buffers_do_not_hold(capi, host, form):
    """the device entry point cannot read its buffers before it launches: the kernels refuse a pair whose pattern or group is
    out of range, whose pattern is empty or too long — and only it —, nothing outside the rows is written, and the library
    stays usable"""
    long = form == "long"
    limit = capi.EDIT_LONG_MAX_PATTERN if long else capi.EDIT_MAX_PATTERN
    codes = E.letter_codes("ACGT")
    records, groups = ["ACGTACGT", "", "TTTT", "TACG"], [0, 2, 4]
    patterns = ["ACGT", "A" * (limit + 1), "", "T" * limit]
    pairs = [(0, 0, 1), (1, 0, 5000), (2, 0, 5), (7, 0, 1), (0, 9, 1), (0, 1, 4), (3, 1, limit), (0xFFFFFFFF, 0xFFFFFFFF, 1), (0, 0, 4)]
    valid = [0, 5, 6, 8]
    want = _reference(host, (patterns, records, groups, [pairs[i] for i in valid], codes))
    want[:, 0] = np.asarray(valid, dtype=np.uint32)[want[:, 0]]
    assert want.tolist() == [[0, 0, 0, 4], [5, 3, 2, 1], [5, 1, 3, 4], [6, limit - 4, 2, 4], [6, limit - 1, 3, 1], [8, 0, 0, 4], [8, 4, 1, 0]]
    guard = 64
    for capacity in (16, 3):
        buf, total, status = capi.edit_targets_device(patterns, records, groups, pairs, codes, capacity, long=long, guard=guard)
        assert status.tolist() == [0, REFUSED, REFUSED, REFUSED, REFUSED, 0, 0, REFUSED, 0] and total == want.shape[0]
        rows = min(capacity, want.shape[0])
        assert buf[guard:guard + 16 * rows].view(np.uint32).reshape(-1, 4).tolist() == want[:rows].tolist()
        assert (buf[:guard] == 0xA5).all() and (buf[guard + 16 * rows:] == 0xA5).all()
    # the host-buffer call checks first
    fn = capi.edit_targets_long if long else capi.edit_targets
    for bad in ([pairs[1]], [pairs[2]], [pairs[3]], [pairs[4]], [pairs[7]]):
        with pytest.raises(capi.TxqError) as e:
            fn(patterns, records, groups, bad, codes)
        assert e.value.code == -1
    hits, total, status = fn(patterns, records, groups, [pairs[i] for i in valid], codes)
    assert total == want.shape[0] and not status.any() and hits[:, 1:].tolist() == want[:, 1:].tolist()
    hits, total, status = fn(patterns, records, groups, [], codes)
    assert total == 0 and hits.shape == (0, 4) and status.size == 0


def test_device_call_on_a_stream(capi, host):
    """txq_edit_targets_device on a stream of torch's making; nothing is waited for inside the call"""
    import torch
    case = _raw(edit_cases.build([5, 70, 300], "peptide", seed=3, long_bytes=900))
    want = _reference(host, case)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    buf, total, status = capi.edit_targets_device(*case, want.shape[0] + 5, stream=stream.cuda_stream)
    assert total == want.shape[0] and not status.any()
    assert buf[64:64 + 16 * total].view(np.uint32).reshape(-1, 4).tolist() == want.tolist()
