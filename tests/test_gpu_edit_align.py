"""GPU parity of alignments (include/txq.h txq_edit_align / txq_edit_align_device): every word of every answer
against tetrex_amd.host.edit_align (txh_edit_align), which tests/test_edit_align_cpu.py holds to the full matrix of
tests/edit_align_ref.py; where m <= 40 against that yardstick directly.  The triples come from capi.edit_search (m <= 512) and
capi.edit_search_long."""
import numpy as np
import pytest

import edit_align_ref as A
import edit_cases
import edit_ref as E

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 63, 64, 65, 512, 513, 1025, 4096]  # either side of a block of 64 rows, of the two instances' 512 rows, and the limit
DISTANCES = [0, 1, 5, 31]
MAX_ERRORS = 31
FILL = 0xA5A5A5A5
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


def _substituted(letters, p, d):
    """d substitutions at evenly spaced places: distance d to p unless chance offers less"""
    s = bytearray(p)
    for at in (np.arange(d) * len(p) // max(d, 1)).tolist():
        s[at] = ord(letters[(letters.index(chr(s[at]).upper()) + 1) % len(letters)])
    return bytes(s)


def _build(alphabet, seed):
    """For every length and distance three groups — the copy at the very start of its record (the window is clipped), inside
    it, at its very end —, the copy made by substitutions where where = 0, 1 and by a mix of edits where it is 2; the target
    is the third record of its group, behind a record of no bytes and one of seven; text with bytes of no class.  Patterns
    of one and two letters have no letters around their copy."""
    letters = edit_cases.ALPHABETS[alphabet]
    rng = np.random.default_rng(seed)
    patterns, records, groups, pairs = [], [], [0], []
    for m in LENGTHS:
        for d in [d for d in DISTANCES if d <= m]:
            for where in range(3):
                p = edit_cases.random_text(rng, letters, m, junk=0).tobytes()
                copy = _substituted(letters, p, d) if where < 2 else edit_cases.edited(rng, letters, np.frombuffer(p, np.uint8), d).tobytes()
                left = b"" if where == 0 else edit_cases.random_text(rng, letters, int(rng.integers(1, 80))).tobytes()
                right = b"" if where == 2 else edit_cases.random_text(rng, letters, int(rng.integers(1, 80))).tobytes()
                if m <= 2:  # no letters around the copy, which would hold the pattern by chance; d = m: the empty match in the empty record
                    records += [b"", b"#######", copy, b""]
                else:
                    records += [b"", edit_cases.random_text(rng, letters, 7).tobytes(), left + copy + right, b""]
                groups.append(len(records))
                pairs.append((len(patterns), len(groups) - 2, 40))
                patterns.append(p)
    return patterns, records, groups, pairs, E.letter_codes(letters)


def _search(capi, patterns, records, groups, pairs, codes):
    """the triples: patterns of up to 512 letters from the one-lane kernel, the others from the long-pattern kernel"""
    short = [i for i, (p, _, _) in enumerate(pairs) if len(patterns[p]) <= capi.EDIT_MAX_PATTERN]
    long_ = [i for i in range(len(pairs)) if i not in set(short)]
    out = np.zeros((len(pairs), 3), dtype=np.uint32)
    if short:
        out[short] = capi.edit_search(patterns, records, groups, [pairs[i] for i in short], codes)
    if long_:
        out[long_] = capi.edit_search_long(patterns, records, groups, [pairs[i] for i in long_], codes)
    return out


def _differing(got, want, pairs, results):
    bad = np.flatnonzero((got != want).any(axis=1))
    return [(tuple(pairs[i]), results[i].tolist(), got[i, :8].tolist(), want[i, :8].tolist()) for i in bad[:4]], bad.size


@pytest.fixture(scope="module")
def parity_cases(capi, host):
    """inputs, the device's triples and the host twin's words, computed once per alphabet"""
    out = {}
    for alphabet in edit_cases.ALPHABETS:
        case = _build(alphabet, seed=61 + len(alphabet))
        results = _search(capi, *case)
        assert (results == host.edit_search(*case, threads=8)).all()
        out[alphabet] = (case, results, host.edit_align(*case[:4], results, case[4], MAX_ERRORS, threads=8, raw=True))
    return out


@pytest.mark.parametrize("alphabet", list(edit_cases.ALPHABETS))
def test_parity_with_host_twin(capi, parity_cases, alphabet):
    (patterns, records, groups, pairs, codes), results, want = parity_cases[alphabet]
    got = capi.edit_align(patterns, records, groups, pairs, results, codes, MAX_ERRORS, raw=True)
    assert _differing(got, want, pairs, results) == ([], 0)
    starts, runs = capi.decode_alignments(got, MAX_ERRORS)
    seen, by_length = set(), {}
    for (p, _, _), (d, r, j), start, rr in zip(pairs, results.tolist(), starts.tolist(), runs):
        m = len(patterns[p])
        assert d <= MAX_ERRORS and start < capi.EDIT_ALIGN_DECLINED  # every pair was aligned on the device
        A.check_identities(m, d, j, start, rr)
        seen.update(c for c, _ in rr)
        by_length.setdefault(m, set()).add(d)
        if m <= 40:
            assert (d, j, start, rr) == A.align(patterns[p], records[r], codes, j)
    assert seen == set("=XID")
    # every distance at every length that can have it (four letters seldom leave 31 edits 31 apart in 65 letters or fewer)
    assert all(set(d for d in DISTANCES if d <= m and (d < 31 or m >= 512 or alphabet == "peptide")) <= by_length[m] for m in LENGTHS), by_length
    assert (starts == 0).sum() >= len(LENGTHS)  # copies at the very start of their record


@pytest.mark.parametrize("m", [64, 513, 4096])
def test_distance_32_is_declined(capi, host, m):
    """d = 32: the marker, and not one word more; the host twin answers the pair"""
    letters = edit_cases.ALPHABETS["peptide"]
    rng = np.random.default_rng(m)
    p = edit_cases.random_text(rng, letters, m, junk=0).tobytes()
    records = [b"WWW" + _substituted(letters, p, 32) + b"YY", b"WWWW" + _substituted(letters, p, 31) + b"Y"]
    groups, pairs, codes = [0, 1, 2], [(0, 0, 40), (0, 1, 40)], E.letter_codes(letters)
    results = _search(capi, [p], records, groups, pairs, codes)
    assert results.tolist() == [[32, 0, 3 + m], [31, 1, 4 + m]]
    got = capi.edit_align([p], records, groups, pairs, results, codes, 40, raw=True)
    want = host.edit_align([p], records, groups, pairs, results, codes, 40, raw=True)
    assert got[0].tolist() == [capi.EDIT_ALIGN_DECLINED] + [FILL] * 82
    assert got[1].tolist() == want[1].tolist() and want[1, :2].tolist() == [4, 62]
    assert want[0, :2].tolist() == [3, 64]
    # d within the device's limit but above max_errors: declined as well
    got = capi.edit_align([p], records, groups, pairs[1:], results[1:], codes, 30, raw=True)
    assert got.tolist() == [[capi.EDIT_ALIGN_DECLINED] + [FILL] * 62]


@pytest.mark.parametrize("pat_at,text_at", [(0, 0), (3, 0), (1, 5), (15, 9)])
def test_placed_buffers_and_guard_bytes(capi, host, pat_at, text_at):
    """txq_edit_align_device with the pattern and text arenas 0 .. 15 bytes behind a 16-byte boundary; the first match's window
    is clipped at offset 0 of the text buffer (with text_at = 0 the first byte of its allocation: no load in front of it); the
    bytes around the arenas are letters, the bytes around the answers a fill that must survive"""
    letters = edit_cases.ALPHABETS["dna"]
    rng = np.random.default_rng(5)
    codes = E.letter_codes(letters)
    patterns = [edit_cases.random_text(rng, letters, m, junk=0).tobytes() for m in (70, 600, 33)]
    records = [patterns[0][2:30] + patterns[0][31:] + b"GATTACA", b"", b"AC" + _substituted(letters, patterns[1], 3), patterns[2][1:]]
    groups, pairs = [0, 1, 4], [(0, 0, 5), (1, 1, 5), (2, 1, 5), (2, 0, 2)]
    want_results = host.edit_search(patterns, records, groups, pairs, codes)
    assert want_results.tolist() == [[3, 0, 67], [3, 2, 602], [1, 3, 32], [E.NONE] * 3]
    want = host.edit_align(patterns, records, groups, pairs, want_results, codes, 5, raw=True)
    assert want[0, 0] == 0 and want[2, 0] == 0  # both begin at their record's first byte
    for long in (False, True):
        results, buf = capi.edit_align_device(patterns, records, groups, pairs, codes, 5, long=long, pat_at=pat_at, text_at=text_at, guard=64)
        triples, words = want_results.tolist(), want.tolist()
        if not long:  # the one-lane kernel refuses the pattern of 600 letters, and the align call passes its marker on
            triples[1], words[1] = REFUSED, [E.NONE, 0xFFFFFFFE] + [0] * 11
        assert results.tolist() == triples
        assert (buf[:64] == 0xA5).all() and (buf[-64:] == 0xA5).all()
        assert buf[64:-64].view(np.uint32).reshape(4, 13).tolist() == words


def test_markers_and_garbage_triples(capi, host):
    """"none" and the refusal marker are passed on; triples that are no cell of their pair's matrix — a record out of range or
    outside the group, an end beyond the record, d > m, a distance the cell does not have — are marked, the others answered,
    the guard bytes intact, and the library usable afterwards"""
    codes = E.letter_codes("ACGT")
    patterns, records, groups = ["ACGTACGT", "A" * 600, "ACGT" * 200], ["", "GGACGTACGTGG", "TT" + "ACGT" * 200, "ACG"], [0, 2, 4]
    pairs = [(0, 0, 2)] * 10 + [(1, 1, 9), (2, 1, 9), (2, 1, 9), (2, 1, 9), (7, 0, 2), (0, 5, 2), (0, 0, 2)]
    triples = [[0, 1, 10], [E.NONE] * 3, REFUSED, [0, 7, 10], [0, 0xFFFFFFF0, 10], [0, 2, 10], [0, 1, 13], [0, 1, 0xFFFFFFFF], [9, 1, 10], [1, 1, 10],
               [601, 2, 5], [0, 2, 802], [0, 2, 803], [0, 3, 802], [0, 1, 10], [0, 1, 10], [0, 1, 10]]
    results, buf = capi.edit_align_device(patterns, records, groups, pairs, codes, 2, results=triples, guard=256)
    assert results.tolist() == triples
    assert (buf[:256] == 0xA5).all() and (buf[-256:] == 0xA5).all()
    got = buf[256:-256].view(np.uint32).reshape(len(pairs), 7).tolist()
    good, declined = [2, 1, 8 << 2, 0, 0, 0, 0], [capi.EDIT_ALIGN_DECLINED] + [FILL] * 6
    assert got[0] == good and got[16] == good
    assert got[1] == [E.NONE, 0, 0, 0, 0, 0, 0] and got[2] == [E.NONE, 0xFFFFFFFE, 0, 0, 0, 0, 0]
    for i in list(range(3, 11)) + [12, 13]:
        assert got[i] == declined, i
    assert got[11] == [2, 1, 800 << 2, 0, 0, 0, 0]
    assert got[14] == got[2] and got[15] == got[2]  # a pattern, a group out of range: this call's own refusal
    # the host twin says the same of every pair it can be asked about (its checks refuse pairs 14 and 15 outright)
    want = host.edit_align(patterns, records, groups, pairs[:14], triples[:14], codes, 2, raw=True)
    assert want.tolist() == got[:14]
    starts, runs = capi.edit_align(patterns, records, groups, pairs[:1], triples[:1], codes, 2)
    assert starts.tolist() == [2] and runs == [[("=", 8)]]
    with pytest.raises(capi.TxqError):
        capi.edit_align(patterns, records, groups, [(7, 0, 2)], triples[:1], codes, 2)
    with pytest.raises(capi.TxqError):
        capi.edit_align(patterns, records, groups, pairs[:1], triples[:1], codes, (1 << 24) + 1, raw=True)


def test_queued_behind_the_search_call_on_a_stream(capi, parity_cases):
    """txq_edit_search*_device and txq_edit_align_device back to back on a stream of torch's making: the align call reads the
    triples on the device, nothing is read back or waited for in between"""
    import torch
    (patterns, records, groups, pairs, codes), results, want = parity_cases["peptide"]
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    for long in (False, True):
        rows = [i for i, (p, _, _) in enumerate(pairs) if long or len(patterns[p]) <= capi.EDIT_MAX_PATTERN]
        got_results, buf = capi.edit_align_device(patterns, records, groups, [pairs[i] for i in rows], codes, MAX_ERRORS, long=long, pat_at=7, text_at=11,
                                                  stream=stream.cuda_stream)
        assert got_results.tolist() == results[rows].tolist()
        got = buf[64:-64].view(np.uint32).reshape(len(rows), 2 * MAX_ERRORS + 3)
        assert _differing(got, want[rows], [pairs[i] for i in rows], results[rows]) == ([], 0)
        assert (buf[:64] == 0xA5).all() and (buf[-64:] == 0xA5).all()
