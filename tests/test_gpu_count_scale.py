"""txq_count where a workgroup takes more than one work item and where a launcher cuts a call into several device calls: the
persistent grids of count_flat_kernel and count_hibf_level_kernel carry LDS counters from one item to the next ("cleared when
read"), and count_flat / count_hibf cut large calls (csrc/txq_count.hip, csrc/txq_count_plan.hpp).  Every case first asserts,
from its shape and the launch arithmetic restated here in plain Python, that it reaches the path it is written for — a later
change of a grid constant makes the case fail instead of testing nothing — and then compares every hit mask and every count
with the numpy restatement of tests/search_ref.py.

Wide indexes: flat_search is too slow there (0.1 ms per value at 8200 bins), so a wide case draws every query's values with
repetition from a domain of 256 values, takes the domain's masks from the oracle once, and gets the expected counts as the
integer product (multiplicity of value d in query q) x (bit b of value d): the same restatement, summed in another order.  The
product runs in float64, where sums of integers below 2^53 are exact."""
import numpy as np
import pytest

from helpers import random_words, oracle_ibf_from_words, layout_hibf, splitmix64
from search_ref import TreeRef, flat_search, csr, unpack, pack
from test_gpu_search import thresholds_for

pytestmark = pytest.mark.gpu

# the launch arithmetic of csrc/txq_count_plan.hpp and csrc/txq_count.hip, restated
SEG_MIN, TARGET_UNITS, COUNT_GRID = 512, 8192, 4096  # txq_count_plan.hpp: kSegMin, kTargetUnits, kCountGrid
TILE_CHUNKS = 64                                     # txq_count.hip: kTileChunks (16-byte chunks of a column tile)
ACC_BYTES = 256 << 20                                # txq_count_plan.hpp: kCountAccBytes
CAP_ITEMS = 1 << 24                                  # txq_count_plan.hpp: kHibfCapItems


def seg_len(n):
    """txq_count_plan.hpp seg_len"""
    return max(SEG_MIN, -(-n // TARGET_UNITS))


def flat_items(words, n_values):
    """(units, column tiles) of count_flat_kernel: n_units = ceil(n / seg) (count_flat_kernel), chunks = stride / 2 with the
    row stride the word count rounded up to even (txq_hibf_plan.hpp row_stride), n_tiles = ceil(chunks / 64) (count_flat)"""
    seg = seg_len(n_values)
    chunks = 1 if words <= 1 else (words + 1) // 2
    return -(-n_values // seg), -(-chunks // TILE_CHUNKS)


def per_call(nq, words):
    """txq_count_plan.hpp count_flat_per_call: queries per device call of a flat call without counts"""
    return max(1, min(nq, ACC_BYTES // (words * 64 * 4)))


def hibf_chunk(nq, max_level_width):
    """txq_count_plan.hpp count_hibf_chunk"""
    return min(max(1, CAP_ITEMS // max_level_width), nq)


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


def hits_of(counts, thr, bins):
    """hit = count >= threshold on the user bins (what flat_search does with its counts)"""
    h = counts >= np.asarray(thr, dtype=np.int64)[:, None]
    h[:, bins:] = False
    return pack(h)


def at_counts(counts, bins):
    """a threshold for every query that is exactly its count in one bin (bin q mod bins): a count off by one flips the hit"""
    q = np.arange(counts.shape[0])
    return counts[q, q % bins].astype(np.uint32)


def some_but_not_all(hits, bins):
    bits = unpack(hits)[:, :bins]
    return bool(bits.any()) and not bool(bits.all())


def check_against(capi, bins, rows, h, words, values, offsets, rounds, shards=(1,), with_counts=(True, False)):
    """rounds: (thresholds, expected hits, expected counts).  Every shard of every sharding, with and without counts."""
    for R in shards:
        ixs = [capi.Index.upload_ibf(bins, rows, h, words, shard_rank=r, n_shards=R) for r in range(R)]
        for thr, want_hits, want_counts in rounds:
            assert some_but_not_all(want_hits, bins)
            got_h, got_c = [], []
            for r, ix in enumerate(ixs):
                w0, W = int(ix.info.shard_word0), ix.shard_words
                if True in with_counts:
                    hits, counts = ix.count(values, offsets, thr, counts=True)
                    assert np.array_equal(counts, want_counts[:, 64 * w0:64 * (w0 + W)]), (bins, R, r)
                    assert np.array_equal(hits, want_hits[:, w0:w0 + W]), (bins, R, r)
                    got_c.append(counts)
                if False in with_counts:
                    hits = ix.count(values, offsets, thr)
                    assert np.array_equal(hits, want_hits[:, w0:w0 + W]), (bins, R, r, "without counts")
                got_h.append(hits)
            assert np.array_equal(np.concatenate(got_h, axis=1), want_hits)
            if got_c:
                assert np.array_equal(np.concatenate(got_c, axis=1), want_counts)
        for ix in ixs:
            ix.free()


# ---- narrow flat IBF: restated in full -----------------------------------------------------------------------------------

NARROW = (40, 4099, 2)  # bins, rows, hash functions: the index of test_flat_long_query_spreads_over_waves


def narrow_rounds(oracle, values, offsets):
    bins, rows, h = NARROW
    words = random_words(bins, rows, 0.4, 5)
    ox = oracle_ibf_from_words(oracle, bins, rows, h, words)
    thr = thresholds_for(offsets, 2)
    want_hits, want_counts = flat_search(ox, bins, values, offsets, thr)
    tight = at_counts(want_counts, bins)
    return words, [(thr, want_hits, want_counts), (tight, hits_of(want_counts, tight, bins), want_counts)]


def test_flat_second_work_item_one_tile(capi, oracle):
    """About 4400 queries of 300 .. 700 values: more than 4096 units on one column tile, short and long queries (seg = 512)
    mixed in every unit; a workgroup's second unit starts on the counters its first one left."""
    bins, rows, h = NARROW
    rng = np.random.default_rng(41)
    lens = rng.integers(300, 701, size=4400)
    total = int(lens.sum())
    seg = seg_len(total)
    n_units, n_tiles = flat_items(1, total)
    assert seg == SEG_MIN and n_tiles == 1 and n_units * n_tiles > COUNT_GRID, (seg, n_units, n_tiles)  # count_flat_kernel: work < n_units * n_tiles, work += gridDim.x
    assert (lens <= seg).sum() > 1000 and (lens > seg).sum() > 1000
    values = splitmix64(41, total)
    offsets = np.zeros(lens.size + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    words, rounds = narrow_rounds(oracle, values, offsets)
    check_against(capi, bins, rows, h, words, values, offsets, rounds)


def seg_edge_lengths(total, rng):
    """lengths seg - 1, seg, seg + 1, 1, 0, 0, 2 seg + 3, 64 and filler in turn, `total` values in all; about every 13th
    query is moved (by one more short query in front of it) to begin at most 3 values before a nominal unit boundary"""
    seg = seg_len(total)
    cycle = [seg - 1, seg, seg + 1, 1, 0, 0, 2 * seg + 3, 64]
    lens, s, i = [], 0, 0
    while s < total:
        if i % 13 == 12:
            to, k = (-s) % seg, int(rng.integers(0, 4))
            if to > k and s + to - k < total:
                lens.append(to - k)
                s += to - k
        n = cycle[i % 11] if i % 11 < 8 else int(rng.integers(200, 800))
        n = min(n, total - s)
        lens.append(n)
        s += n
        i += 1
    return np.array(lens, dtype=np.int64)


def test_flat_seg_above_512(capi, oracle):
    """Exactly 4 300 800 values: seg = 525, 8192 units.  Query lengths at seg - 1, seg, seg + 1 and 2 seg + 3, empty runs,
    queries that begin 0 .. 3 values before a nominal unit boundary (unit_start hands them whole to the unit before)."""
    bins, rows, h = NARROW
    total = 4_300_800
    seg = seg_len(total)
    n_units, n_tiles = flat_items(1, total)
    assert seg == 525 and seg > SEG_MIN and n_units == TARGET_UNITS and n_units > COUNT_GRID  # seg_len: ceil(n / kTargetUnits) above kSegMin
    lens = seg_edge_lengths(total, np.random.default_rng(43))
    assert int(lens.sum()) == total
    offsets = np.zeros(lens.size + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    begin = offsets[:-1].astype(np.int64)
    before = (lens > 0) & (lens <= seg) & ((-begin) % seg <= 3) & (begin % seg != 0) & (begin // seg != (begin + lens - 1) // seg)
    assert before.sum() > 100  # short queries across a nominal boundary that begin at most 3 values before it
    for n in (seg - 1, seg, seg + 1, 2 * seg + 3, 0, 1):
        assert (lens == n).sum() > 100, n
    values = splitmix64(43, total)
    words, rounds = narrow_rounds(oracle, values, offsets)
    check_against(capi, bins, rows, h, words, values, offsets, rounds)


@pytest.mark.parametrize("reverse", [False, True])
def test_flat_boundary_at_default_seg(capi, oracle, reverse):
    """seg = 512: queries of 511, 512 and 513 values, 1024 and 1025, short queries that begin inside the unit before."""
    bins, rows, h = 1000, 1031, 3
    lens = [511, 512, 513, 0, 1, 512, 512, 1024, 1025, 3, 0]
    lens = np.array(lens[::-1] if reverse else lens, dtype=np.int64)
    total = int(lens.sum())
    seg = seg_len(total)
    assert seg == SEG_MIN and {seg - 1, seg, seg + 1} <= set(lens.tolist())
    offsets = np.zeros(lens.size + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    begin = offsets[:-1].astype(np.int64)
    crossing = (lens > 0) & (lens <= seg) & (begin % seg != 0) & (begin // seg != (begin + lens - 1) // seg)
    assert crossing.any()  # a short query across a nominal unit boundary
    values = splitmix64(47 + reverse, total)
    words = random_words(bins, rows, 0.5, 47)
    ox = oracle_ibf_from_words(oracle, bins, rows, h, words)
    rounds = []
    for shift in range(5):
        thr = thresholds_for(offsets, shift)
        rounds.append((thr,) + flat_search(ox, bins, values, offsets, thr))
    tight = at_counts(rounds[0][2], bins)
    rounds.append((tight, hits_of(rounds[0][2], tight, bins), rounds[0][2]))
    check_against(capi, bins, rows, h, words, values, offsets, rounds)


# ---- wide flat IBF: values from a small domain ---------------------------------------------------------------------------

def domain_rounds(oracle, bins, rows, h, seed, lens, shift):
    """index words, values, offsets and the expected answer of queries drawn from a 256-value domain"""
    words = random_words(bins, rows, 0.5, seed)
    ox = oracle_ibf_from_words(oracle, bins, rows, h, words)
    rng = np.random.default_rng(seed)
    domain = splitmix64(seed, 256)
    lens = np.asarray(lens, dtype=np.int64)
    idx = rng.integers(0, domain.size, size=int(lens.sum()))
    offsets = np.zeros(lens.size + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    mult = np.zeros((lens.size, domain.size), dtype=np.float64)
    np.add.at(mult, (np.repeat(np.arange(lens.size), lens), idx), 1.0)
    bit = unpack(ox.probe(domain)).astype(np.float64)
    want_counts = np.rint(mult @ bit).astype(np.int64)  # (exact: integers far below 2^53)
    assert int(want_counts.max()) <= int(lens.max()) and np.array_equal(want_counts.sum(axis=1) == 0, (mult @ bit.sum(axis=1)) == 0)
    thr = thresholds_for(offsets, shift)
    return words, domain[idx], offsets, thr, hits_of(want_counts, thr, bins), want_counts


def test_flat_three_column_tiles(capi, oracle):
    """16 400 bins: 257 words, three column tiles, the third of one chunk.  1400 queries of 512 values are 1400 units x 3
    tiles on 4096 workgroups, and 4096 is no multiple of 3: a workgroup's second item is on another tile (other counters
    in use, another tile width) than its first.  Also on three column shards, joined."""
    bins, rows, h = 16400, 1031, 3
    lens = np.full(1400, 512)
    n_units, n_tiles = flat_items((bins + 63) // 64, int(lens.sum()))
    assert n_tiles == 3 and n_units == 1400 and n_units * n_tiles > COUNT_GRID and COUNT_GRID % n_tiles != 0  # count_flat_kernel: tile = work % n_tiles
    assert ((bins + 63) // 64 + 1) // 2 % TILE_CHUNKS == 1  # chunks of the last tile
    words, values, offsets, thr, want_hits, want_counts = domain_rounds(oracle, bins, rows, h, 53, lens, 3)
    check_against(capi, bins, rows, h, words, values, offsets, [(thr, want_hits, want_counts)], shards=(1, 3), with_counts=(True,))


def test_flat_second_per_call_chunk(capi, oracle):
    """9000 bins, 7500 queries, no counts: the scratch accumulators hold 7436 queries, so count_flat makes two device
    calls, the second on offsets that do not begin at 0.  A query of 600 and one of 5000 values (longer than seg: they need
    the accumulators) in either call, the last one the last query of all.  The same call with counts is one device call."""
    bins, rows, h = 9000, 1031, 3
    nq, W = 7500, (9000 + 63) // 64
    cut = per_call(nq, W)
    assert cut == 7436 and cut < nq  # count_flat: for (q0 = 0; q0 < nq; q0 += per_call)
    lens = np.random.default_rng(59).integers(1, 4, size=nq)
    lens[[5, 2000, 7, cut + 3]] = 0
    lens[100], lens[4000], lens[cut + 10], lens[nq - 1] = 600, 5000, 600, 5000
    assert seg_len(int(lens[:cut].sum())) == SEG_MIN and seg_len(int(lens[cut:].sum())) == SEG_MIN
    words, values, offsets, thr, want_hits, want_counts = domain_rounds(oracle, bins, rows, h, 59, lens, 1)
    for q in (100, 4000, cut + 10, nq - 1):  # the long queries: the median of their counts, so about half of the bins pass
        thr[q] = int(np.median(want_counts[q, :bins]))
    want_hits = hits_of(want_counts, thr, bins)
    for q in (100, 4000, cut + 10, nq - 1):
        assert some_but_not_all(want_hits[q:q + 1], bins), q
    check_against(capi, bins, rows, h, words, values, offsets, [(thr, want_hits, want_counts)], with_counts=(False, True))


# ---- HIBF ----------------------------------------------------------------------------------------------------------------

def tree_queries(values, seed, n):
    """n queries made as test_gpu_search.tree_batch makes them (all of a user bin's values, or a part, plus noise; every
    21st random), every 50th empty"""
    rng = np.random.default_rng(seed)
    qs = []
    for i in range(n):
        if i % 50 == 49:
            qs.append(np.zeros(0, dtype=np.uint64))
        elif i % 21 == 20:
            qs.append(rng.integers(0, 1 << 20, size=70, dtype=np.uint64))
        else:
            v = values[int(rng.integers(0, len(values)))]
            take = v if rng.random() < 0.5 else v[: max(1, len(v) // 2)]
            qs.append(np.concatenate([take, rng.integers(0, 1 << 20, size=int(rng.integers(0, 6)), dtype=np.uint64)]))
    return csr(qs)


TREES = {"layout": dict(seed=5, user_bins=900, tmax=64, n_values=30), "layout_4_levels": dict(seed=6, user_bins=400, tmax=16, n_values=30, direct=3)}


def make_tree(oracle, name):
    kw = dict(TREES[name])
    return layout_hibf(oracle, kw.pop("seed"), **kw)


@pytest.mark.parametrize("name", list(TREES))
def test_hibf_more_queries_than_waves(capi, oracle, name):
    """5000 queries: level 0 has more than 4096 (query, root) items, and a deeper level more than 4096 (query, IBF) pairs,
    so a wave of count_hibf_level_kernel counts a second item on the counters its first one cleared."""
    ox, descs, values = make_tree(oracle, name)
    user_bins = len(values)
    ref = TreeRef(oracle, user_bins, descs)
    v, off = tree_queries(values, len(name), 5000)
    shards = {1: [capi.Index.upload_hibf(user_bins, descs)]}
    if name == "layout":
        shards[2] = [capi.Index.upload_hibf(user_bins, descs, shard_rank=r, n_shards=2) for r in range(2)]
    for shift in (0, 3):
        thr = thresholds_for(off, shift)
        want_hits, want_counts = ref.search(v, off, thr)
        # count_hibf_level_kernel: item < count, item += gridDim.x; count_hibf: grid = lvl ? kCountGrid : min(nq, kCountGrid)
        assert ref.level_pairs[0] == 5000 > COUNT_GRID and max(ref.level_pairs[1:]) > COUNT_GRID, ref.level_pairs
        assert some_but_not_all(want_hits, user_bins)
        for R, ixs in shards.items():
            got = [ix.count(v, off, thr, counts=True) for ix in ixs]
            assert np.array_equal(np.concatenate([g[0] for g in got], axis=1), want_hits), (name, shift, R)
            assert np.array_equal(np.concatenate([g[1] for g in got], axis=1), want_counts), (name, shift, R)
            assert np.array_equal(np.concatenate([ix.count(v, off, thr) for ix in ixs], axis=1), want_hits), (name, shift, R)
    for ixs in shards.values():
        for ix in ixs:
            ix.free()


def level_widths(descs):
    """IBFs on every level of the tree (txq_hibf_plan.hpp: max_level_width is the largest)"""
    widths, level = [], [0]
    while level:
        widths.append(len(level))
        level = [int(c) for i in level for c, u in zip(descs[i]["next_ibf_id"], descs[i]["tb_to_user"]) if int(u) == 0xFFFFFFFFFFFFFFFF]
    return widths


def test_hibf_second_chunk(capi, oracle):
    """chunk + 60 queries on the 4-level tree: count_hibf makes two device calls.  The first `chunk` queries are single
    values at threshold 1 (the probe's masks, from the oracle), the last 60 a batch with rotating thresholds (the
    restatement of those 60 alone): queries are independent, so the two references are the call's answer."""
    ox, descs, values = make_tree(oracle, "layout_4_levels")
    user_bins = len(values)
    widths = level_widths(descs)
    chunk = hibf_chunk(1 << 30, max(widths))
    assert len(widths) >= 3 and chunk == CAP_ITEMS // max(widths) and chunk < 600_000, widths  # count_hibf: for (q0 = 0; q0 < nq; q0 += chunk)
    rng = np.random.default_rng(61)
    own = np.concatenate(values)
    singles = np.concatenate([own[rng.integers(0, own.size, size=chunk // 2)], rng.integers(0, 1 << 20, size=chunk - chunk // 2, dtype=np.uint64)])
    tv, toff = tree_queries(values, 61, 60)
    v = np.concatenate([singles, tv])
    off = np.concatenate([np.arange(chunk, dtype=np.uint64), toff + np.uint64(chunk)])
    nq = off.size - 1
    assert nq == chunk + 60 and hibf_chunk(nq, max(widths)) == chunk < nq
    tail_thr = thresholds_for(toff, 2)
    thr = np.concatenate([np.ones(chunk, dtype=np.uint32), tail_thr])
    want_head = ox.probe(singles)
    want_tail_hits, want_tail_counts = TreeRef(oracle, user_bins, descs).search(tv, toff, tail_thr)
    assert some_but_not_all(want_head, user_bins) and some_but_not_all(want_tail_hits, user_bins)
    ix = capi.Index.upload_hibf(user_bins, descs)
    hits, counts = ix.count(v, off, thr, counts=True)
    assert np.array_equal(hits[chunk:], want_tail_hits)
    assert np.array_equal(counts[chunk:], want_tail_counts)
    assert np.array_equal(hits[:chunk], want_head)
    head_bits = unpack(want_head)
    for a in range(0, chunk, 1 << 16):  # (one value: a bin's count is not 0 where its bit is set; a split bin may count it twice)
        b = min(a + (1 << 16), chunk)
        assert np.array_equal(counts[a:b] > 0, head_bits[a:b] > 0), a
    assert np.array_equal(ix.count(v, off, thr), hits)
    ix.free()
