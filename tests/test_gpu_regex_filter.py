"""GPU parity of the record filter (include/txq.h txq_regex_filter): capi.regex_filter against the host twin
host.regex_filter — the same automaton blobs through the same inline interpreter — bit for bit, with TXQ_REGEX_CHUNK=16 and
with the default chunk; and a call of more units than the persistent grids have workgroups."""
import numpy as np
import pytest

from tetrex_amd import host

pytestmark = pytest.mark.gpu

MOTIFS = ["(LMAEGLYN)", "(^M.K)", "(GT$)", "(A(C+|G+)T)", "(A.{12}C)", "(C.{2,4}C.{3}[LIVMFYWC])", "(A|)", "(^MAEG$)",
          "(A.{9}C)", "(A.{11}C)", "(A.{9}C+T)"]
INSTANCE = ["LMAEGLYN", "MWK", "GT", "ACCCT", "AWWWWWWWWWWWWC", "CWWCWWWL", "", "MAEG",
            "AWWWWWWWWWC", "AWWWWWWWWWWWC", "AWWWWWWWWWCCT"]
LDS, L2 = 0, 4  # a small automaton and the one above 64 KiB
MIDDLE = (8, 9, 10)  # tables of 9 536, 37 184 and 14 400 bytes: the tier between (64 KiB of LDS); the last one is unbounded
BOUNDARY = 256  # a multiple of both chunks the tests run


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def automata():
    blobs = [host.regex_automaton(rx, True) for rx in MOTIFS]
    assert len(blobs[L2]) > 65536 and all(len(b) <= 8192 for i, b in enumerate(blobs) if i != L2 and i not in MIDDLE)
    assert all(8192 < len(blobs[i]) <= 65536 for i in MIDDLE)  # each of the three table tiers is there
    return blobs


@pytest.fixture(scope="module")
def case(automata):
    """records, groups, pairs and the host twin's answer, computed once.  Filler letters occur in no motif, so a record matches
    only what was planted in it."""
    rng = np.random.default_rng(5)
    filler = lambda n: "".join(rng.choice(list("WYQ"), size=n)) if n else ""
    recs, expect = [], {}  # expect[(automaton, record)] = the answer the construction intends
    size = lambda: sum(len(r) for r in recs)

    def planted(a, tail_at):
        """a record with INSTANCE[a] in it, the instance's last byte at text offset = tail_at modulo BOUNDARY"""
        inst = INSTANCE[a]
        lead = (tail_at - (size() + len(inst) - 1)) % BOUNDARY
        recs.append(filler(lead) + inst + filler(7))
        expect[(a, len(recs) - 1)] = True

    # group 0: matches that straddle a chunk boundary, end exactly on one, begin exactly on one
    for a in (0, 3, 4, 5) + MIDDLE:
        planted(a, len(INSTANCE[a]) // 2 - 1)          # the boundary in the middle of the match
        planted(a, BOUNDARY - 1)                       # the match's last byte is a chunk's last byte
        planted(a, len(INSTANCE[a]) - 1)               # its first byte is a chunk's first byte
        planted(a, 17 + len(INSTANCE[a]) // 2 - 1)     # the same at a 16-byte boundary that is no 256-byte boundary
        planted(a, 15)
    # `^` at a record start that is no chunk start, `$` at a record end in mid-chunk; and the same letters where they must not match
    recs.append(filler((5 - size()) % 16))  # the next record starts 5 bytes behind a 16-byte boundary and ends 2 in front of one
    recs.append("MWK" + filler(20) + "GT"); expect[(1, len(recs) - 1)] = True; expect[(2, len(recs) - 1)] = True
    recs.append("W" + "MWK" + filler(9) + "GT" + "W"); expect[(1, len(recs) - 1)] = False; expect[(2, len(recs) - 1)] = False
    recs.append("MAEG"); expect[(7, len(recs) - 1)] = True
    recs.append("MAEGW"); expect[(7, len(recs) - 1)] = False
    # records of 0, 1, 15, 16, 17 and about 5 000 bytes
    for n in (0, 1, 15, 16, 17):
        recs.append(filler(n)); expect[(6, len(recs) - 1)] = True; expect[(0, len(recs) - 1)] = False
    long = filler(5003)
    recs.append(long[:3000] + "LMAEGLYN" + long[3000:]); expect[(0, len(recs) - 1)] = True; expect[(4, len(recs) - 1)] = False
    recs.append(long[:4990] + "AWWWWWWWWWWWWC"); expect[(4, len(recs) - 1)] = True; expect[(0, len(recs) - 1)] = False
    recs.append(long); expect[(0, len(recs) - 1)] = False
    n0 = len(recs)
    # group 1: no records.  group 2: 70 records, a bitmap of three words
    for i in range(70):
        body = filler(int(rng.integers(0, 60)))
        if i % 3 == 0:
            a = int(rng.integers(len(MOTIFS)))
            body = (INSTANCE[a] + body) if a in (1, 7) and i % 2 else body[:len(body) // 2] + INSTANCE[a] + body[len(body) // 2:]
        recs.append(body)
    recs.append(filler(11))  # group 3: one record; the text's size is no multiple of 16
    groups = [0, n0, n0, n0 + 70, n0 + 71]
    recs = [r.encode() for r in recs]
    assert sum(len(r) for r in recs) % 16 != 0 and sum(len(r) for r in recs) < 1_000_000
    # every automaton on groups 0 and 2 (several pairs on one group, one automaton on several groups), some on the others
    pairs = [(a, g) for g in (0, 2) for a in range(len(MOTIFS))] + [(LDS, 1), (L2, 1), (LDS, 3), (L2, 3), (3, 3), (MIDDLE[1], 1), (MIDDLE[1], 3), (MIDDLE[2], 3)]
    want = host.regex_filter(automata, recs, groups, pairs)
    for (a, r), answer in expect.items():
        assert want[pairs.index((a, 0))][r] == answer, (MOTIFS[a], r, recs[r][:40])
    assert len(want[pairs.index((LDS, 2))]) == 70 and want[pairs.index((LDS, 1))].size == 0
    return recs, groups, pairs, want


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.tolist() == w.tolist(), (i, np.flatnonzero(g != w)[:8].tolist() if g.size == w.size else (g.size, w.size))


@pytest.mark.parametrize("chunk", [None, "16"])
def test_parity_with_host_twin(capi, automata, case, monkeypatch, chunk):
    """bounded matches across, at and behind chunk boundaries; ^ and $ off the boundaries; records of 0, 1, 15, 16, 17 and 5 000
    bytes; groups of 0, 1 and 70 records; a text whose size is no multiple of 16; all three table tiers in one call (tables
    of at most 8 KiB, of at most 64 KiB — regex_kernel<kLargeLds>, MIDDLE — and above, read from L2)"""
    if chunk:
        monkeypatch.setenv("TXQ_REGEX_CHUNK", chunk)
    recs, groups, pairs, want = case
    got, status = capi.regex_filter(automata, recs, groups, pairs, return_status=True)
    assert status.tolist() == [0] * len(pairs)
    _same(got, want)


@pytest.mark.parametrize("chunk", [None, "16"])
def test_unbounded_automaton_and_serial_cap(capi, automata, monkeypatch, chunk):
    """A(C+|G+)T with TXQ_REGEX_MAX_SERIAL=256: a record of 300 bytes is flagged whether or not it holds a match, records of
    255 and 256 bytes are answered exactly; the bounded automaton beside it does not know the cap.  A.{9}C+T, unbounded with a
    table of the middle tier, is capped and answered in the same way."""
    monkeypatch.setenv("TXQ_REGEX_MAX_SERIAL", "256")
    if chunk:
        monkeypatch.setenv("TXQ_REGEX_CHUNK", chunk)
    recs = []
    for n in (255, 256, 300):
        recs += [b"W" * n, b"W" * (n - 9) + b"AGGGGGGGT", b"ACT" + b"W" * (n - 3), b"W" * (n - 120) + b"A" + b"C" * 118 + b"T"]
    recs.append(b"W" * 290 + b"LMAEGLYN" + b"WW")
    pairs = [(3, 0), (LDS, 0), (MIDDLE[2], 0)]
    want = host.regex_filter(automata, recs, [0, len(recs)], pairs, max_serial=256)
    assert want[0].tolist() == [False, True, True, True] * 2 + [True] * 5 and want[1].tolist() == [False] * 12 + [True]
    assert want[2].tolist() == [False, False, False, True] * 2 + [True] * 5  # only A C{118} T holds A.{9}C+T
    _same(capi.regex_filter(automata, recs, [0, len(recs)], pairs), want)


def test_text_that_is_not_16_byte_aligned(capi, automata, monkeypatch):
    """txq_regex_filter_device on a text that begins 1, 7 and 15 bytes behind a 16-byte boundary: records of 40, 0 and 150 bytes,
    a bounded and an unbounded automaton, chunks of 16 bytes.  The 16-byte blocks at either end of the text are assembled from
    byte loads; the byte in front of the text would complete ACCT and the byte behind it LMAEGLYN, were they taken in."""
    import torch
    monkeypatch.setenv("TXQ_REGEX_CHUNK", "16")
    rng = np.random.default_rng(6)
    filler = lambda n: "".join(rng.choice(list("WYQ"), size=n))
    recs = ["CCT" + filler(9) + "LMAEGLYN" + filler(20), "", filler(60) + "AGGGT" + filler(78) + "LMAEGLY"]
    assert [len(r) for r in recs] == [40, 0, 150]
    recs, groups, pairs = [r.encode() for r in recs], [0, 3], [(0, 0), (1, 0)]
    blobs = [automata[LDS], automata[3]]  # (LMAEGLYN), bounded; (A(C+|G+)T), unbounded
    want, want_status = host.regex_filter(blobs, recs, groups, pairs, return_status=True)
    assert [w.tolist() for w in want] == [[True, False, False], [False, False, True]] and want_status.tolist() == [0, 0]
    arena, ao, txt, ro, go, pr, oo, n_words = host.regex_filter_arrays(blobs, recs, groups, pairs)
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).to(dev) for x in (arena, ao, txt, ro, go, pr, oo)]
    work = torch.empty(capi.regex_workspace_bytes(len(pairs)) // 8, dtype=torch.int64, device=dev)
    results = {}
    for at in (0, 1, 7, 15):
        around = torch.full((at + txt.size + 33,), ord("N"), dtype=torch.uint8, device=dev)
        around[:at] = ord("A")
        shifted = around[at:at + txt.size]
        shifted.copy_(t[2])
        assert shifted.data_ptr() % 16 == at
        out = torch.full((n_words,), -1, dtype=torch.int32, device=dev)
        status = torch.full((len(pairs),), -1, dtype=torch.int32, device=dev)
        capi.check(capi.lib().txq_regex_filter_device(t[0].data_ptr(), t[1].data_ptr(), ao.size - 1, arena.size, shifted.data_ptr(), t[3].data_ptr(),
                                                       ro.size - 1, txt.size, t[4].data_ptr(), go.size - 1, t[5].data_ptr(), len(pairs), t[6].data_ptr(),
                                                       out.data_ptr(), n_words, status.data_ptr(), work.data_ptr(),
                                                       torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize(dev)
        results[at] = (out.cpu().numpy().view(np.uint32), status.cpu().numpy().view(np.uint32))
    for at in (1, 7, 15):
        assert results[at][0].tolist() == results[0][0].tolist() and results[at][1].tolist() == results[0][1].tolist(), at
    assert results[0][1].tolist() == want_status.tolist()
    _same(host.regex_filter_unpack(go, pr, oo, results[0][0], results[0][1]), want)


UNIT_LANES, SMALL_GRID, LARGE_GRID = 256, 256 * 8, 256 * 2  # txq_regex.hip: kBlock; regex_kernel<kSmallLds> and <0>: kCus * 8 workgroups, <kLargeLds>: kCus * 2


@pytest.fixture(scope="module")
def many_units(automata):
    """600 groups of one to three records, 4.2 to 9 KiB each: with chunks of 16 bytes a unit is 4096 bytes and a group two or
    three units.  Every group is paired with four automata — (LMAEGLYN) and A(C+|G+)T of the small tier, A.{11}C or A.{9}C (by
    the group's parity) of the 64 KiB tier, A.{12}C above it — pair after pair, so that neighbouring pairs never share a table.
    Filler letters occur in no motif and a group holds at most one instance: record r matches automaton a exactly if a's
    instance was planted in it."""
    rng = np.random.default_rng(7)
    unit = UNIT_LANES * 16
    recs, groups, pairs, planted, last_byte = [], [0], [], {}, {}  # planted[record] = automaton, last_byte[group] = the instance's last byte in the group
    for g in range(600):
        size = int(rng.integers(4300, 9200))
        body = bytearray("".join(rng.choice(list("WYQ"), size=size)).encode())
        autos = (LDS, 3, MIDDLE[1] if g % 2 == 0 else MIDDLE[0], L2)
        lo = hi = None
        if g % 4 != 3:  # three groups of four hold an instance
            a = autos[int(rng.integers(4))]
            inst = INSTANCE[a].encode()
            where = g % 3
            if where == 0:
                x = unit + len(inst) // 2 - 1           # the boundary between the group's first two units is inside the instance
            elif where == 1:
                x = unit * (1 + (size > 2 * unit)) - 1  # the instance's last byte is a unit's last byte
            else:
                x = int(rng.integers(len(inst), size))
            lo, hi = x - len(inst) + 1, x + 1
            body[lo:hi] = inst
            last_byte[g] = x
        cuts = sorted(int(c) for c in rng.integers(1, size, size=int(rng.integers(0, 3))))
        cuts = [lo if lo is not None and lo < c < hi else c for c in cuts]  # (no cut inside the instance)
        for b, e in zip([0] + cuts, cuts + [size]):
            if lo is not None and b <= lo and hi <= e:  # (true of one record: no cut falls inside the instance)
                planted[len(recs)] = a
            recs.append(bytes(body[b:e]))
        groups.append(len(recs))
        pairs += [(a, g) for a in autos]
    assert len(planted) == len(last_byte) == 450 and set(planted.values()) == {LDS, 3, MIDDLE[0], MIDDLE[1], L2}
    want = host.regex_filter(automata, recs, groups, pairs)
    return recs, groups, pairs, planted, last_byte, want


def test_more_units_than_workgroups(capi, automata, many_units, monkeypatch):
    """About 5300 units: every workgroup of the three persistent grids of regex_kernel walks over two or three units (about
    ten on the 512-workgroup grid of the 64 KiB tier), and the units it takes one after the other belong to pairs with other
    automata: the table in LDS is reloaded between them.  Instances planted in units from the 2048th on, some across the
    boundary between a group's units and some that end on a unit's last byte, are found; no other record is."""
    monkeypatch.setenv("TXQ_REGEX_CHUNK", "16")
    recs, groups, pairs, planted, last_byte, want = many_units
    unit = UNIT_LANES * 16  # txq_text.hpp units_of(bytes, lanes, chunk): per_unit = lanes * chunk
    group_bytes = [sum(len(r) for r in recs[groups[g]:groups[g + 1]]) for g in range(len(groups) - 1)]
    units = np.array([-(-group_bytes[g] // unit) for _, g in pairs])
    assert set(units.tolist()) == {2, 3}
    pref = np.concatenate([[0], np.cumsum(units)])  # regex_plan_kernel and scan_kernel: pref[i + 1] = units of pairs 0 .. i
    total = int(pref[-1])
    assert total > 2 * SMALL_GRID and total > 9 * LARGE_GRID, total  # regex_kernel: u < total, u += gridDim.x
    owner = np.repeat(np.arange(len(pairs)), units)  # pair_of_unit
    auto_of_unit = np.array([a for a, _ in pairs])[owner]
    tier = {LDS: 0, 3: 0, MIDDLE[0]: 1, MIDDLE[1]: 1, L2: 2}
    tier_of_unit = np.array([tier[a] for a in auto_of_unit.tolist()])
    for t, grid in ((0, SMALL_GRID), (1, LARGE_GRID)):  # the two kernels that keep the table in LDS
        changes = 0
        for block in range(grid):
            mine = np.arange(block, total, grid)
            mine = mine[tier_of_unit[mine] == t]  # (a unit of another tier is skipped)
            changes += int((auto_of_unit[mine][1:] != auto_of_unit[mine][:-1]).any())
        # workgroups that load one automaton's table over another's.  (A workgroup of the small grid walks over 2.6 units,
        # half of them of its tier: about one in ten takes two such units, of different automata.)
        assert changes >= 100, (t, changes)
    # where the planted instances lie, as (pair, unit) of the pair that looks for them
    late = straddle = unit_end = found = 0
    for i, (a, g) in enumerate(pairs):
        for r in range(groups[g], groups[g + 1]):
            if planted.get(r) == a:
                found += 1
                x = last_byte[g]
                u = int(pref[i]) + x // unit
                if u >= SMALL_GRID:
                    late += 1
                    straddle += (x - len(INSTANCE[a]) + 1) // unit != x // unit
                    unit_end += x % unit == unit - 1
    assert found == len(planted) and 3 * late >= found and straddle >= 20 and unit_end >= 20, (found, late, straddle, unit_end)
    expect = [np.array([planted.get(r) == a for r in range(groups[g], groups[g + 1])]) for a, g in pairs]
    _same(want, expect)
    got, status = capi.regex_filter(automata, recs, groups, pairs, return_status=True)
    assert status.tolist() == [0] * len(pairs)
    _same(got, want)
    _same(got, expect)


def test_refused_pairs_leave_their_neighbours_alone(capi, automata, case):
    """a pair that names an automaton or a group out of range, and an automaton with a broken header: status
    TXQ_REGEX_REFUSED, no bit set, the pairs around them answered.  (The kernels check every offset against the sizes passed
    before they use it.)"""
    recs, groups, _, _ = case
    broken = bytearray(automata[1])
    broken[8] = 0  # no classes
    blobs = [automata[LDS], bytes(broken), automata[L2]]
    pairs = [(0, 0), (3, 0), (2, 2), (0, 9), (1, 0), (0, 2), (0xFFFFFFFF, 0xFFFFFFFF), (2, 3)]
    want, want_status = host.regex_filter(blobs, recs, groups, pairs, return_status=True)
    R = capi.REGEX_REFUSED
    assert want_status.tolist() == [0, R, 0, R, R, 0, R, 0]
    got, status = capi.regex_filter(blobs, recs, groups, pairs, validate=False, return_status=True)
    assert status.tolist() == want_status.tolist()
    _same(got, want)
    with pytest.raises(capi.TxqError):  # the host-buffer call checks first and launches nothing
        capi.regex_filter(blobs, recs, groups, pairs)
    with pytest.raises(capi.TxqError):
        capi.regex_filter([automata[LDS]], recs, groups, [(0, 9)])


def test_no_pairs_and_no_records(capi, automata):
    assert capi.regex_filter(automata, [b"ACGT"], [0, 1], []) == []
    got = capi.regex_filter(automata, [], [0, 0], [(6, 0)])
    assert got[0].size == 0
    got = capi.regex_filter(automata, [b"", b"", b"MWK"], [0, 2, 3], [(6, 0), (0, 0), (1, 1)])  # a group of empty records only
    assert [g.tolist() for g in got] == [[True, True], [False, False], [True]]
