"""The four kernels that build a sized HIBF (tetrex_amd/csrc/txq_build.hip), each called directly at the edges that the
well-formed input of a whole `tetrex index --layout sized` build never reaches: every register rank up to 53 and the clamp
above it, totals that a double cannot hold, both sides of the switch to linear counting, windows between 1 and n_bins, the
16 x 16 pair tile's edges, every guard of the tree insertion, and the chunked streaming of include/txq.h.  Everything is
compared by equality with the numpy restatement (tests/sized_hibf_ref.py; its helpers are checked on the CPU in
tests/test_sized_hibf_ref.py) or, for inserted bits, with the CPU oracle's emplace."""
import numpy as np
import pytest

from sized_hibf_ref import M, chunk_csr, craft, estimate, inv_fmix, part_of, registers, sketch_slices, union_table

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


def _csr(bins):
    offsets = np.zeros(len(bins) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(v) for v in bins])
    return np.concatenate([np.asarray(v, dtype=np.uint64) for v in bins]), offsets


def _random(rng, n):
    return rng.integers(0, 1 << 64, size=n, dtype=np.uint64, endpoint=False)


def _three_chunks(offsets):
    """The cuts of a library streamed as three chunks; each lies strictly inside a bin."""
    total = int(offsets[-1])
    chunk = (total + 2) // 3
    cuts = [(g, min(total, g + chunk)) for g in range(0, total, chunk)]
    assert len(cuts) == 3
    for g, _ in cuts[1:]:
        assert g not in offsets.tolist(), "a cut on a bin boundary cuts no bin"
    return cuts


# ---- sketch_kernel / narrow_kernel ------------------------------------------------------------------------------------


def test_sketch_holds_every_rank(capi):
    """Ranks 31 .. 53, which random bins never produce: one bin with every rank 1 .. 53 in a register of its own (registers 0
    and 4095 among them), one with nothing but the rank-53 value (x << 12 == 0, the clz of zero), one whose register 5 is
    hit by ranks 3, 53 and 9 in that order, one with the same value 1000 times."""
    ranks = np.arange(1, 54)
    at = ranks * 70
    at[0], at[-1] = 0, M - 1
    bins = [inv_fmix(craft(at, ranks)), inv_fmix(craft([77], [53])), inv_fmix(craft([5, 5, 5], [3, 53, 9])),
            np.repeat(inv_fmix(craft([9], [31])), 1000)]
    want = np.zeros((4, M), dtype=np.uint8)
    want[0, at] = ranks
    want[1, 77] = 53
    want[2, 5] = 53
    want[3, 9] = 31
    got = capi.sketch(bins)
    assert np.array_equal(got, want)
    assert all(np.array_equal(registers(v), w) for v, w in zip(bins, want))  # the restatement says the same


def test_sketch_slice_edges(capi):
    """chunk = max(16384, ceil(len / 16)) and the early return at slice * chunk >= len: bins of 16384, 16385, 262144 and
    262145 values (one slice, 15 workgroups return; a second slice of one value; 16 slices of the least size; chunk =
    ceil(len / 16) = 16385 with a short last slice), behind a bin of 100 so that none begins at index 0.  The filler
    has ranks of 8 at most in registers below 2048; the first and the last value of every slice is a rank-53 marker in a
    register of its own, which nothing else can set: a value dropped at a slice boundary leaves its register at 0."""
    rng = np.random.default_rng(21)
    sizes = (16384, 16385, 262144, 262145)
    bins, marks = [_random(rng, 100)], [None]
    for n in sizes:
        v = inv_fmix(craft(rng.integers(0, 2048, size=n), rng.integers(1, 9, size=n)))
        idx = sorted({i for s in sketch_slices(n) for i in s})
        regs = 2048 + np.arange(len(idx))
        v[idx] = inv_fmix(craft(regs, np.full(len(idx), 53)))
        bins.append(v)
        marks.append(regs)
    assert [len(m) for m in marks[1:]] == [2, 3, 32, 32]
    got = capi.sketch(bins)
    for b in range(1, len(bins)):
        assert np.all(got[b, marks[b]] == 53), (sizes[b - 1], np.flatnonzero(got[b, marks[b]] != 53).tolist())
        assert got[b, :2048].max() <= 8 and not got[b, 2048 + len(marks[b]):].any()
    for b, v in enumerate(bins):
        assert np.array_equal(got[b], registers(v)), b


@pytest.mark.parametrize("cut", ["last bin cut", "last bin empty", "n_values on the last bin's offset"])
def test_sketch_counts_only_values_below_n_values(capi, cut):
    """n_values below offsets[n_bins] (hi = min(n_values, offsets[bin + 1])): the last bin cut after 120 of its 300 values;
    n_values below the last bin's offset, so that it stays empty and the bin in front of it is cut; n_values on that offset."""
    rng = np.random.default_rng(22)
    bins = [_random(rng, n) for n in (100, 0, 20_000, 300)]
    flat, offsets = _csr(bins)
    n_values = int(offsets[3]) + {"last bin cut": 120, "last bin empty": -50, "n_values on the last bin's offset": 0}[cut]
    got = capi.sketch_csr(flat, offsets, n_values)
    kept = [v[:max(0, min(n_values, int(offsets[b + 1])) - int(offsets[b]))] for b, v in enumerate(bins)]
    assert [len(v) for v in kept] == {"last bin cut": [100, 0, 20_000, 120], "last bin empty": [100, 0, 19_950, 0],
                                      "n_values on the last bin's offset": [100, 0, 20_000, 0]}[cut]
    for b, v in enumerate(kept):
        assert np.array_equal(got[b], registers(v)), b
    assert not np.array_equal(registers(bins[3]), registers(kept[3]))  # (the values cut off would have shown)


def test_sketch_does_not_depend_on_the_chunking(capi):
    """One CSR of 12 bins (empty first, middle and last; 1 value; 40 000 values) sketched in one call and as three chunks cut
    as index_build.cpp upload_chunk cuts them (chunk_csr), the registers zeroed before the first only: narrow_kernel's max
    with what earlier chunks left, a bin cut in the middle (twice), bins empty in a chunk.  Repeating the last chunk changes
    nothing."""
    rng = np.random.default_rng(23)
    bins = [_random(rng, n) for n in (0, 1, 3000, 40_000, 0, 17_000, 5, 2500, 20_000, 64, 900, 0)]
    bins[7][:53] = inv_fmix(craft(100 + np.arange(53), np.arange(1, 54)))
    flat, offsets = _csr(bins)
    whole = capi.sketch_csr(flat, offsets, flat.size)
    for b, v in enumerate(bins):
        assert np.array_equal(whole[b], registers(v)), b
    cuts = _three_chunks(offsets)
    # the max with earlier registers decides in both directions: in a cut bin, some registers are higher in the earlier part
    # and some in the later one
    g = cuts[1][0] - int(offsets[3])
    early, late = registers(bins[3][:g]).astype(int), registers(bins[3][g:]).astype(int)
    assert (early > late).any() and (late > early).any()
    regs = None
    for g0, g1 in cuts:
        regs = capi.sketch_csr(*chunk_csr(flat, offsets, g0, g1), registers=regs)
    assert np.array_equal(regs, whole)
    assert np.array_equal(capi.sketch_csr(*chunk_csr(flat, offsets, *cuts[2]), registers=regs), whole)


# ---- union_kernel / pair_union_kernel ---------------------------------------------------------------------------------


def _raw(row):
    """(the estimate before linear counting, the exact integer total, the zero registers) of one row"""
    r = np.minimum(row.astype(np.int64), 53)
    total = sum(1 << (53 - int(k)) for k in r)
    return (0.7213 / (1.0 + 1.079 / M) * M * M) / (float(total) * 2.0 ** -53), total, int((r == 0).sum())


def _with(fill, at, v):
    """a row of `fill` with register `at` set to v"""
    r = np.full(M, fill, dtype=np.uint8)
    r[at] = v
    return r


@pytest.fixture(scope="module")
def rows():
    """40 hand-made register rows.  The asserts say which branch of the estimator each kind reaches; they fail if the rows
    stop reaching it."""
    rng = np.random.default_rng(31)
    rows = [rng.integers(1, 54, size=M) for _ in range(10)]           # 0 .. 9: uniform 1 .. 53
    rows += [rng.integers(0, 54, size=M) for _ in range(6)]           # 10 .. 15: uniform 0 .. 53
    rows += [rng.integers(0, 256, size=M) for _ in range(6)]          # 16 .. 21: uniform 0 .. 255, the min(r, 53) clamp
    rows += [np.full(M, k) for k in (0, 1, 255, 53, 2, 30, 52, 54)]   # 22 .. 29: all equal
    rows += [_with(20, 1000, 0), _with(0, 4095, 53)]                      # 30, 31
    rows += [rng.integers(0, 3, size=M), rng.integers(0, 2, size=M) * 53, _with(1, 0, 0)]  # 32 .. 34: few distinct values
    rows += [registers(_random(rng, n)) for n in (50, 5000, 200_000)]  # 35 .. 37: real sketches on either side of the switch
    rows += [np.where(rng.random(M) < 0.01, 0, rng.integers(40, 54, size=M)), rng.integers(50, 60, size=M)]  # 38, 39
    regs = np.stack([np.asarray(r, dtype=np.uint8) for r in rows])
    assert regs.shape == (40, M)
    raw = [_raw(r) for r in regs]
    # the promise of include/txq.h, "the exact integer sum ... rounded once": totals that no double holds
    inexact = [i for i, (_, total, _) in enumerate(raw) if int(float(total)) != total]
    assert set(range(10)) <= set(inexact), inexact
    small, large = (lambda i: raw[i][0] <= 2.5 * M), (lambda i: raw[i][0] > 2.5 * M)
    assert small(23) and raw[23][2] == 0 and 5900 < raw[23][0] < 5915     # all 1: small E, no zero register: E stays
    assert large(30) and raw[30][2] == 1 and 1.1e7 < raw[30][0] < 1.3e7   # all 20 but one 0: large E, a zero: E stays
    assert small(31) and raw[31][2] == M - 1                              # all 0 but one 53: linear counting, V = 4095
    assert small(22) and raw[22][2] == M and estimate(regs[22]) == 0.0    # all 0: linear counting, V = m
    assert small(35) and large(37) and raw[35][2] > 0 and raw[37][2] == 0
    assert regs[16:22].max() == 255 and (regs[16:22] > 53).mean() > 0.5
    assert raw[24][1] == raw[25][1] == raw[29][1] == M                    # all 255, all 53, all 54: 2^0 each
    return regs


@pytest.fixture(scope="module")
def estimates(rows):
    """estimate(max(rows[a], rows[b])), computed once per pair"""
    cache = {}

    def of(a, b):
        a, b = min(int(a), int(b)), max(int(a), int(b))
        if (a, b) not in cache:
            cache[(a, b)] = estimate(np.maximum(rows[a], rows[b]))
        return cache[(a, b)]
    return of


@pytest.mark.parametrize("window", [1, 7, 40])
def test_union_estimates_of_hand_made_registers(capi, rows, window):
    """union_kernel on the rows above in a shuffled order with one bin twice: registers above 53 (min(r, 53)), totals that
    need the one rounding of (double)th * 2^32 + (double)tl, each combination of E <= 2.5 m and V > 0 (small E without a
    zero register, large E with one, rows whose registers are all equal), and a window strictly between 1 and n_bins, whose
    entries with s + L > n_bins are 0.0 beside estimates."""
    B = rows.shape[0]
    order = np.random.default_rng(32).permutation(B).astype(np.uint32)
    order[11] = order[30]
    got = capi.union_estimates(rows, order, window)
    want = union_table(rows, order, window)
    assert got.shape == want.shape == (B, window)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
    if window == 7:
        assert all(want[s, L - 1] == 0.0 for s in range(B - 6, B) for L in range(B - s + 1, 8))
        assert np.count_nonzero(want[B - 6:]) >= 15  # (estimates beside the zeroes)
    if window == 1:
        assert got[:, 0].tolist() == [estimate(rows[int(b)]) for b in order]


@pytest.mark.parametrize("n", [15, 16, 17, 33, 48])
def test_pair_unions_at_the_tile_edges(capi, rows, estimates, n):
    """pair_union_kernel at n = 15, 16, 17, 33 and 48: one tile not full, one tile exactly, tiles with one row and one
    column (rows and columns past n load bin n - 1 and are never written; three of a wave's four rows idle), three tiles a
    side.  The ids are a permutation with repeats; the rows are those of the union test, so this kernel's min(r, 53), its
    one rounding of (double)th * 2^32 + (double)tl and its switch to linear counting see the same cases.  Equal to the
    restatement on max(regs[a], regs[b]), symmetric, and the diagonal is each bin's own estimate from union_kernel."""
    B = rows.shape[0]
    rng = np.random.default_rng(n)
    perm = rng.permutation(B)
    ids = (np.concatenate([perm, perm[:n - B]]) if n > B else np.concatenate([perm[:n - 2], perm[[0, 3]]])).astype(np.uint32)
    assert ids.size == n and np.unique(ids).size < n
    got = capi.pair_unions(rows, ids)
    want = np.array([[estimates(a, b) for b in ids] for a in ids])
    assert got.shape == (n, n)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
    assert np.array_equal(got, got.T)
    own = capi.union_estimates(rows, np.arange(B, dtype=np.uint32), 1)[:, 0]
    assert np.array_equal(np.diagonal(got), own[ids])


# ---- tree_insert_kernel -----------------------------------------------------------------------------------------------

# (bins, rows, hash functions): bin_words 1, 1, 3 and 4, every supported hash_funs at the ends of its range; IBF 4 has no
# rows and no matrix, IBF 5 is named only by entries that must be skipped
IBFS = [dict(bins=b, bin_size=m, hash_funs=h) for b, m, h in
        ((3, 61, 1), (64, 127, 3), (130, 1031, 5), (200, 4099, 2), (10, 0, 2), (3, 61, 1))]
N_IBF = len(IBFS)
SIZES = (0, 1, 300, 0, 5000, 700, 40, 600, 500, 200, 2000, 0)  # user bins: empty first, middle and last; 1 value; 5000
# each user bin's path as the kernel gets it ...
PATHS = [
    [(0, 0, 1)],
    [(0, 0, 1)],                                    # one entry
    [(0, 0, 1), (1, 5, 1)],                         # two entries, a leaf of one part
    [(0, 1, 1), (2, 7, 2)],
    [(0, 1, 1), (2, 0, 129)],                       # a leaf of 129 parts: technical bins 0 .. 128 of 130
    [(0, 2, 1), (1, 63, 1), (3, 10, 3)],            # three entries, a leaf of 3 parts; bit 63 of a word
    [(0, 1, 1), (2, 129, 1)],                       # the last bin of three words
    [(3, 198, 2)],                                  # a leaf of 2 parts, the last bins of four words
    [(1, 0, 2)],
    [(N_IBF, 0, 1), (3, 200, 1), (4, 0, 1), (5, 3, 1), (1, 20, 1)],  # ibf == n_ibf; tb == bins; no rows; tb == bins; a good one
    [(0, 2, 1), (5, 3, 1), (3, 190, 15)],           # parts 10 .. 14 lie at or beyond bin 200: those values are dropped
    [(2, 64, 1)],
]
# ... and what must come of it: the entries that are skipped as a whole are not here, the run of 15 is the run of 10 that fits
KEPT = {9: [(1, 20, 1)], 10: [(0, 2, 1), (3, 190, 15)]}
FITS = {(3, 190, 15): 10}


def _path_arrays(paths):
    po = np.zeros(len(paths) + 1, dtype=np.uint64)
    po[1:] = np.cumsum([len(p) for p in paths])
    return po, np.array([e for p in paths for e in p], dtype=np.uint64).reshape(-1, 3)


def _emplaced(oracle, ibfs, paths, bins, fits=()):
    """Every IBF's words by the oracle's emplace: all values of a bin in each entry of its path but the last, and in the
    last the part that part_of picks — left out where the part lies at or beyond `fits` parts."""
    ox = oracle.Index.hibf(len(bins))
    ids = {}
    for i, f in enumerate(ibfs):
        if f["bin_size"]:
            z = np.zeros(f["bins"], dtype=np.uint64)
            ids[i] = ox.add_ibf(f["bins"], f["bin_size"], f["hash_funs"], z, z)
    for v, steps in zip(bins, paths):
        if not len(v) or not steps:
            continue
        for (i, t, parts) in steps[:-1]:
            assert parts == 1
            ox.hibf_emplace(ids[i], v, t)
        i, t, parts = steps[-1]
        which = part_of(v, parts) if parts > 1 else np.zeros(len(v), dtype=np.uint64)
        for p in np.unique(which):
            if int(p) < dict(fits).get((i, t, parts), parts):
                ox.hibf_emplace(ids[i], v[which == p], t + int(p))
    return [ox.hibf_words(ids[i]) if i in ids else np.zeros(0, dtype=np.uint64) for i in range(len(ibfs))]


@pytest.fixture(scope="module")
def tree(oracle):
    rng = np.random.default_rng(41)
    bins = [_random(rng, n) for n in SIZES]
    kept = [KEPT.get(b, p) for b, p in enumerate(PATHS)]
    want = _emplaced(oracle, IBFS, kept, bins, FITS.items())
    which = part_of(bins[10], 15)
    assert (which < 10).sum() > 500 and (which >= 10).sum() > 200   # values on either side of the IBF's last bin
    assert np.unique(part_of(bins[4], 129)).size == 129              # every one of the 129 parts is hit
    assert all(w.any() for w in want[:4]) and want[4].size == 0 and not want[5].any()
    return bins, want


def _same_words(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (i, np.flatnonzero(g != w)[:8].tolist())


def test_tree_insert_paths_parts_and_skipped_entries(capi, tree):
    """tree_insert_kernel against the oracle's emplace, word for word: paths of 1, 2 and 3 entries; leaf runs of 1, 2, 3 and
    129 parts; bin_words of 1, 1, 3 and 4 with 1, 3, 5 and 2 hash functions; empty user bins.  "Entries outside an IBF's
    bins are skipped" (include/txq.h): an entry with ibf == n_ibf (`p.ibf >= n_ibf`), two whose first bin is the IBF's bin
    count (`tb >= f.bins`), one on a descriptor without rows or matrix (`f.bin_size == 0`) leave no bit, and the entry behind
    them in the same path is still inserted; of a run of 15 parts from bin 190 of 200 only the values of parts 10 .. 14 are
    dropped.  IBF 5, which only skipped entries name, stays zero.  (`tb / 64 >= f.bin_words` cannot be reached apart from
    `tb >= f.bins` with a descriptor whose bin_words fits its bins.)  A second call on the words of the first changes
    nothing."""
    bins, want = tree
    flat, offsets = _csr(bins)
    po, path = _path_arrays(PATHS)
    got = capi.tree_insert(flat, offsets, flat.size, po, path, IBFS)
    _same_words(got, want)
    assert got[4].size == 0 and not got[5].any()
    _same_words(capi.tree_insert(flat, offsets, flat.size, po, path, IBFS, words=got), want)


def test_tree_insert_ignores_values_outside_every_bin(capi, tree):
    """offsets[0] = 3 and n_values = offsets[n_bins] + 5 (`i < offsets[l] || i >= offsets[l + 1]`): the values in front of
    the first bin and behind the last set nothing."""
    bins, want = tree
    flat, offsets = _csr(bins)
    rng = np.random.default_rng(42)
    flat = np.concatenate([_random(rng, 3), flat, _random(rng, 5)])
    po, path = _path_arrays(PATHS)
    _same_words(capi.tree_insert(flat, offsets + np.uint64(3), flat.size, po, path, IBFS), want)


def test_tree_insert_does_not_depend_on_the_chunking(capi, tree):
    """The library as three chunks cut as index_build.cpp upload_chunk cuts them (two bins cut in the middle, bins empty in a
    chunk), each call ORing into the words the one before left; then the last chunk once more."""
    bins, want = tree
    flat, offsets = _csr(bins)
    po, path = _path_arrays(PATHS)
    cuts = _three_chunks(offsets)
    words = None
    for g0, g1 in cuts:
        words = capi.tree_insert(*chunk_csr(flat, offsets, g0, g1), po, path, IBFS, words=words)
    _same_words(words, want)
    _same_words(capi.tree_insert(*chunk_csr(flat, offsets, *cuts[2]), po, path, IBFS, words=words), want)


@pytest.mark.parametrize("front", [0, 3])
def test_tree_insert_with_one_user_bin(capi, oracle, front):
    """n_bins == 1: the search for a value's bin has nothing to halve; with offsets[0] = 3 as well."""
    rng = np.random.default_rng(43)
    v = _random(rng, 100)
    paths = [[(0, 2, 1), (2, 127, 3)]]
    ibfs = IBFS[:3]
    want = _emplaced(oracle, ibfs, paths, [v])
    assert want[0].any() and not want[1].any() and want[2].any()
    flat = np.concatenate([_random(rng, front), v, _random(rng, 2)])
    offsets = np.array([front, front + 100], dtype=np.uint64)
    po, path = _path_arrays(paths)
    _same_words(capi.tree_insert(flat, offsets, flat.size, po, path, ibfs), want)
