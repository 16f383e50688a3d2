"""The HIBF descent kernels (csrc/txq_hibf.hip) past their grids: a wave's or a workgroup's second and later k-mers, rows wider
than one sweep of lanes, a call cut into chunks, more groups than one phase.  Every case first asserts, from its tree, batch and
switches and the launch arithmetic restated in tests/hibf_descent_ref.py (held against csrc/txq_hibf_descent_plan.hpp by
tests/test_hibf_descent_plan.py, which also runs over CASES and LAYOUT_CASES below), that it reaches the kernel and the loop it is
written for — a later change of a grid constant makes the case fail instead of testing nothing — and then compares every mask row
and every alive bit of txq_probe_device with the CPU oracle, bit for bit.

Large batches are periodic: the k-mers are np.resize(base, n) with len(base) = 4099, a prime, so the same k-mer meets different
lanes, waves and rounds; the oracle probes `base` once and the expected row of k-mer i is want_base[i % 4099]."""
import numpy as np
import pytest

import hibf_descent_ref as ref
from helpers import MERGED, random_words, oracle_ibf_from_words, random_hibf, layout_hibf, regular_hibf, split_heavy_hibf, make_blob
from search_ref import unpack

pytestmark = pytest.mark.gpu

P = 4099  # the period (a prime)


# ---- trees ---------------------------------------------------------------------------------------------------------------

def wide_leaf(O, bins, seed, permuted):
    """A tree of ONE IBF of `bins` technical bins, each a user bin (permuted: in a random order, so that hits go through the
    technical-bin -> user-bin map; else identity-mapped: the row words are mask words), 509 rows: half of them random bits of
    density 0.3, half empty — a k-mer whose two rows are both full has about 9 % of the bins set, every other k-mer none."""
    rng = np.random.default_rng(seed)
    tbu = (rng.permutation(bins) if permuted else np.arange(bins)).astype(np.uint64)
    nxt = np.zeros(bins, dtype=np.uint64)
    words = random_words(bins, 509, 0.3, seed).reshape(509, -1)
    words[rng.random(509) < 0.5] = 0
    words = np.ascontiguousarray(words.reshape(-1))
    ox = O.Index.hibf(bins, dna=False, k=4)
    ox.add_ibf(bins, 509, 2, nxt, tbu, words=words)
    return ox, [dict(bins=bins, bin_size=509, hash_funs=2, words=words, next_ibf_id=nxt, tb_to_user=tbu)], None


def _regular(user_bins, children, per, h, mixed=False, fpr=0.05):
    def build(O):
        rng = np.random.default_rng(user_bins + h)
        return regular_hibf(O, user_bins, children, per, lambda b: rng.integers(0, 1 << 20, size=per, dtype=np.uint64), h=h, mixed=mixed, fpr=fpr)
    return build


# name -> (user bins, builder(oracle) -> (oracle index, upload descriptors, values per user bin or None[, ...]))
TREES = {
    "general300": (300, lambda O: random_hibf(O, 5, user_bins=300, tmax=128, levels=3)),
    "wide2048": (2500, lambda O: random_hibf(O, 31, user_bins=2500, tmax=2048, levels=3, n_values=8)),
    # (a tree as in test_gpu_probe.py test_hibf_stack_entries_...: values from a universe of 64, a k-mer reaches nearly every IBF; IBFs
    # of up to 128 bins, so that the tree has fewer IBFs than two per mask word: the output row has room for the stack's spill)
    "saturated": (12000, lambda O: layout_hibf(O, 4, user_bins=12000, tmax=128, n_values=20, value_bits=6)),
    "leaf4096": (4096, lambda O: wide_leaf(O, 4096, 11, True)),
    "leaf8192": (8192, lambda O: wide_leaf(O, 8192, 12, False)),
    "leaf16448": (16448, lambda O: wide_leaf(O, 16448, 13, True)),
    "deep16": (400, lambda O: layout_hibf(O, 6, user_bins=400, tmax=16, n_values=30, direct=3)),
    # (a false-positive rate of 0.001: at 0.05 every k-mer would be in some of the 66 560 bins)
    "reg130x512": (130 * 512, _regular(130 * 512, 130, 12, 2, fpr=0.001)),
    "reg33x256": (33 * 256, _regular(33 * 256, 33, 30, 3)),
    "reg33x256mixed": (33 * 256, _regular(33 * 256, 33, 30, 3, mixed=True)),
    "reg9x128": (9 * 128, _regular(9 * 128, 9, 30, 2)),
    "layout3000": (3000, lambda O: layout_hibf(O, 7, user_bins=3000, tmax=64)),
    "splitheavy": (None, lambda O: split_heavy_hibf(O, 3)),
}


def build_tree(O, name):
    """(user bins, oracle index, descriptors, values per user bin or None)"""
    ub, make = TREES[name]
    got = make(O)
    return (len(got[2]) if ub is None else ub), got[0], got[1], got[2]


def frontier_pairs(O, descs, kmers):
    """(k-mer, IBF) pairs on every level of the descent of `kmers`: what hibf_level_kernel's frontiers hold"""
    level, pairs = {0: np.arange(kmers.size)}, []
    while level:
        pairs.append(sum(len(q) for q in level.values()))
        nxt = {}
        for i, q in level.items():
            d = descs[i]
            bits = unpack(oracle_ibf_from_words(O, d["bins"], d["bin_size"], d["hash_funs"], d["words"]).probe(kmers[q]))
            for tb in np.flatnonzero(np.asarray(d["tb_to_user"], dtype=np.uint64) == np.uint64(MERGED)):
                if bits[:, tb].any():
                    nxt[int(d["next_ibf_id"][tb])] = q[bits[:, tb] > 0]
        level = nxt
    return pairs


PLANTED = {"deep16": 3600, "saturated": 64}  # k-mers of the base that are values of user bins (default: about half)


def two_chunks(sh):
    """the batch of the level path's second chunk: one k-mer more than a chunk holds and than mask_alive_kernel's grid covers"""
    return max((1 << 24) // sh["max_level_width"], 2048 * 256) + 1237


def batch_size(n, sh):
    return n(sh) if callable(n) else n


# ---- cases: (tree, shards, rank, switches, n) ------------------------------------------------------------------------------

NO_SMALL = {"TXQ_HIBF_SMALL": "0"}
FUSED_WAVES = [(t, 1, 0, dict(env, TXQ_HIBF_WAVES=str(w)), 1000) for t, env in (("general300", NO_SMALL), ("wide2048", {})) for w in (1, 3, 64)]
FUSED_WAVES += [("general300", 2, 1, dict(NO_SMALL, TXQ_HIBF_WAVES="3"), 1000), ("wide2048", 2, 1, {"TXQ_HIBF_WAVES": "3"}, 1000)]
FUSED_DEFAULT_GRID = [("general300", 1, 0, NO_SMALL, 2 * 16384 + 77)]
FUSED_SPILL = [("saturated", 1, 0, {"TXQ_HIBF_SMALL": "0", "TXQ_HIBF_STACK_LDS": "2", "TXQ_HIBF_WAVES": "3"}, 564)]
WIDE = {"leaf4096": (16, 1, 1), "leaf8192": (32, 1, 2), "leaf16448": (64, 2, 5)}  # fused G, fused w_iters, level w_iters
WIDE_FUSED = [(t, 1, 0, {"TXQ_HIBF_WAVES": "5"}, 9000) for t in WIDE]
WIDE_LEVELS = [(t, 1, 0, {"TXQ_HIBF_LEVELS": "1"}, 9000) for t in WIDE]
LEVEL_CHUNKS = [("deep16", 1, 0, {"TXQ_HIBF_LEVELS": "1"}, two_chunks)]
SMALL_GRID = [("general300", 1, 0, {}, 2048 * 256 + 300)]
PHASES = [("reg130x512", 1, 0, {}, n) for n in (1531, 1, 63, 257)] + [("reg130x512", 1, 0, {"TXQ_HIBF_STEPS_PER_GROUP": "1"}, 1531), ("reg130x512", 2, 1, {}, 1531)]
UNROLLS = [(t, 1, 0, {"TXQ_HIBF_UNROLL": str(u), "TXQ_HIBF_TILE": "64"}, n) for t in ("reg33x256", "reg33x256mixed") for u in (1, 2, 3, 4, 8) for n in (1, 193, 1531)]
UNROLLS += [("reg33x256", 1, 0, {"TXQ_HIBF_UNROLL": str(u), "TXQ_HIBF_TILE": "64", "TXQ_HIBF_LANE_HASH": "1"}, 1531) for u in (2, 3)]
ROOT_GRID = [("reg9x128", 1, 0, {"TXQ_HIBF_INTERLEAVE_PROBE": "0"}, (1 << 21) + 5003)]
CASES = FUSED_WAVES + FUSED_DEFAULT_GRID + FUSED_SPILL + WIDE_FUSED + WIDE_LEVELS + LEVEL_CHUNKS + SMALL_GRID + PHASES + UNROLLS + ROOT_GRID

TABLE_OFF = {"TXQ_KMER_TABLE_MB": "0"}
LAYOUT_WAYS = [{}, {"TXQ_HIBF_LAYOUT_DIRECT": "0"}, {"TXQ_HIBF_LAYOUT_FUSED": "0"}, {"TXQ_HIBF_WAVES": "7"}, {"TXQ_HIBF_LAYOUT_DIRECT": "0", "TXQ_HIBF_WAVES": "7"}]
LAYOUT_CASES = [(t, dict(TABLE_OFF, **way), 5003) for t in ("layout3000", "splitheavy", "leaf4096", "leaf16448") for way in LAYOUT_WAYS]


def case_id(c):
    return "-".join([c[0]] + (["shard%dof%d" % (c[2], c[1])] if len(c) == 5 and c[1] > 1 else []) +
                    ["%s=%s" % (k.replace("TXQ_HIBF_", "").replace("TXQ_", ""), v) for k, v in c[-2].items()] + ["n=%s" % (c[-1] if not callable(c[-1]) else "chunk+")])


# ---- fixtures ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def forest(capi, oracle):
    """Trees, their periodic base with the oracle's masks of it, and uploaded indexes: each built once for the module."""
    trees, uploaded = {}, {}

    def tree(name):
        if name not in trees:
            ub, ox, descs, values = build_tree(oracle, name)
            rng = np.random.default_rng(7919 + len(name))  # (no seed of a tree: the random k-mers are no bin's values)
            planted = np.zeros(0, dtype=np.uint64)
            if name == "saturated":  # (the whole universe of its values: k-mers that are nearly everywhere)
                planted = np.arange(64, dtype=np.uint64)
            elif values is not None:  # values of every few user bins
                take = PLANTED.get(name, P // 2)
                planted = np.concatenate([v[:-(-take // len(values[::max(1, ub // 1500)]))] for v in values[::max(1, ub // 1500)]])[:take]
            base = rng.permutation(np.concatenate([planted, rng.integers(0, 1 << 20, size=P - planted.size, dtype=np.uint64)]))
            want = ox.probe(base)
            assert base.size == P and want.any()
            trees[name] = (ub, ox, descs, base, want)
        return trees[name]

    def index(name, R=1, r=0):
        if (name, R, r) not in uploaded:
            ub, _, descs, _, _ = tree(name)
            uploaded[(name, R, r)] = capi.Index.upload_hibf(ub, descs, shard_rank=r, n_shards=R)
        return uploaded[(name, R, r)]

    yield tree, index
    for ix in uploaded.values():
        ix.free()


def plans(forest, monkeypatch, case):
    """(shape, switches, n) of a case, with its switches set in the environment"""
    name, R, r, env, n = case
    ub, _, descs, _, _ = forest[0](name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sh = ref.shape_of(ub, descs, r, R, interleave_probe=env.get("TXQ_HIBF_INTERLEAVE_PROBE") != "0")
    return sh, ref.knobs(env), batch_size(n, sh)


def probe_and_compare(capi, forest, case, n, windows=None):
    """txq_probe_device with an alive buffer on np.resize(base, n): all alive bits, and all mask rows (or the rows of `windows`:
    [(first, end)], read from the device at an offset) against the oracle's."""
    name, R, r = case[:3]
    _, _, _, base, want_base = forest[0](name)
    ix = forest[1](name, R, r)
    lo, nw = int(ix.info.shard_word0), ix.shard_words
    want_base = np.ascontiguousarray(want_base[:, lo:lo + nw])
    kmers = np.resize(base, n)
    period = np.arange(n) % P
    want_alive = want_base.any(axis=1)[period]
    if n >= 64:
        assert 0 < int(want_alive.sum()) < n  # both outcomes
    if capi is None:
        return
    dk = capi.DeviceBuffer.from_numpy(kmers)
    dm = capi.DeviceBuffer(n * nw * 8)
    da = capi.DeviceBuffer(((n + 63) // 64) * 8)
    ix.probe_device(dk.ptr, n, dm.ptr, da.ptr)
    capi.synchronize()
    alive = np.unpackbits(da.to_numpy(np.uint8, (((n + 63) // 64) * 8,)), bitorder="little")
    assert np.array_equal(alive[:n].astype(bool), want_alive), case_id(case)
    assert not alive[n:].any()
    for a, b in windows or [(0, n)]:
        got = dm.to_numpy(np.uint64, (b - a, nw), offset=a * nw * 8)
        assert np.array_equal(got, want_base[period[a:b]]), (case_id(case), a, b)
    for buf in (dk, dm, da):
        buf.free()


# ---- a. fused kernel, user order: a wave's second and later k-mers ---------------------------------------------------------

@pytest.mark.parametrize("case", FUSED_WAVES + FUSED_DEFAULT_GRID, ids=case_id)
def test_fused_wave_takes_further_kmers(capi, forest, monkeypatch, case):
    """hibf_fused_kernel: i += waves.  The wave's LDS row and stack are reused, the next k-mer is prefetched while this one descends."""
    sh, kn, n = plans(forest, monkeypatch, case)
    p = ref.plan_fused(sh, kn, n)
    assert ref.descent_path(sh, kn, n) == ref.FUSED and n > 2 * p["grid"] * p["waves_per_block"], p  # every wave takes a second k-mer, most a third
    if case[0] == "wide2048":
        assert p["G"] == 8
    if "TXQ_HIBF_WAVES" not in case[3]:
        assert p["grid"] * p["waves_per_block"] == ref.FUSED_WAVES
    probe_and_compare(capi, forest, case, n)


@pytest.mark.parametrize("case", FUSED_SPILL, ids=case_id)
def test_fused_spill_area_and_row_alternate_on_one_wave(capi, forest, monkeypatch, case):
    """Two stack entries in LDS, the rest in the k-mer's own output row, which the wave then overwrites with the finished row —
    and four waves for 564 k-mers: a wave's next k-mer spills into the next row while the last one's is final."""
    sh, kn, n = plans(forest, monkeypatch, case)
    p = ref.plan_fused(sh, kn, n)
    assert ref.descent_path(sh, kn, n) == ref.FUSED and n > 2 * p["grid"] * p["waves_per_block"]
    assert p["stack_lds"] == 2 and sh["n_ibf"] > 100, (p, sh)  # (the output row has the room: the stack is not kept whole in LDS)
    _, _, _, base, want = forest[0](case[0])
    bits = np.unpackbits(want[:64].view(np.uint8), axis=1).sum(axis=1)
    assert (bits > 12000 // 4).any()  # saturated: some k-mers are nearly everywhere, dozens of IBFs pending at once
    probe_and_compare(capi, forest, case, n)


# ---- b. IBFs wider than 2048 technical bins --------------------------------------------------------------------------------

@pytest.mark.parametrize("case", WIDE_FUSED, ids=case_id)
def test_fused_wide_ibf(capi, forest, monkeypatch, case):
    """hibf_fused_kernel<16>, <32> and <64> with two sweeps (w_iters = 2), on 5 waves (8 launched) for 9000 k-mers."""
    sh, kn, n = plans(forest, monkeypatch, case)
    p = ref.plan_fused(sh, kn, n)
    assert ref.descent_path(sh, kn, n) == ref.FUSED and (p["G"], p["w_iters"]) == WIDE[case[0]][:2], p
    assert n > 2 * p["grid"] * p["waves_per_block"]
    probe_and_compare(capi, forest, case, n)


@pytest.mark.parametrize("case", WIDE_LEVELS, ids=case_id)
def test_level_kernel_wide_ibf_in_rounds(capi, forest, monkeypatch, case):
    """hibf_level_kernel<64> with up to 5 sweeps over the row, and 9000 * 64 lanes on 2048 blocks: level 0 takes a second round."""
    sh, kn, n = plans(forest, monkeypatch, case)
    p = ref.plan_levels(sh, n)
    assert ref.descent_path(sh, kn, n) == ref.LEVELS and (p["G"], p["w_iters"]) == (64, WIDE[case[0]][2]), p
    assert p["chunk"] == n and p["blocks0"] == ref.LEVEL_BLOCKS and n * p["G"] > ref.LEVEL_BLOCKS * 256  # rounds > 1
    probe_and_compare(capi, forest, case, n)


# ---- c. level path in two chunks -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", LEVEL_CHUNKS, ids=case_id)
def test_level_path_second_chunk(capi, oracle, forest, monkeypatch, case):
    """hibf_probe cuts the batch at 2^24 / max_level_width k-mers: the second chunk starts at d_kmers + off and d_masks + off * w_out
    on counters reset for it, its frontier indexes count from the chunk's first k-mer; deeper levels take several rounds;
    mask_alive_kernel strides past its 2048 blocks."""
    sh, kn, n = plans(forest, monkeypatch, case)
    p = ref.plan_levels(sh, n)
    assert ref.descent_path(sh, kn, n) == ref.LEVELS and sh["shard_words"] <= 16 and sh["max_level_width"] >= 32 and sh["depth"] >= 3, sh
    assert p["chunk"] == (1 << 24) // sh["max_level_width"] < n <= 2 * p["chunk"], p  # two chunks
    assert n > ref.LEVEL_BLOCKS * 256 == p["alive_blocks"] * 256  # mask_alive_kernel: i += stride
    _, _, descs, base, _ = forest[0](case[0])
    pairs = frontier_pairs(oracle, descs, base)  # of one period; a chunk holds chunk // P whole periods
    assert max(pairs[1:]) * (p["chunk"] // P) > p["blocks_deeper"] * 256 // p["G"], pairs  # a deeper level's frontier: rounds > 1
    assert n * sh["shard_words"] * 8 < 80 << 20
    probe_and_compare(capi, forest, case, n)


# ---- d. small kernel past its grid ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", SMALL_GRID, ids=case_id)
def test_small_kernel_past_its_grid_with_alive_bits(capi, forest, monkeypatch, case):
    """hibf_small_kernel: base += gridDim.x * 256; the workgroup's LDS rows and stacks are reused, alive words are stored whole."""
    sh, kn, n = plans(forest, monkeypatch, case)
    assert ref.descent_path(sh, kn, n) == ref.SMALL and ref.small_blocks(n) == ref.SMALL_BLOCKS < -(-n // 256)
    assert n % 256 and n % 64  # a ragged last workgroup and a ragged last alive word
    probe_and_compare(capi, forest, case, n)


# ---- e. child-stationary ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", PHASES, ids=case_id)
def test_children_kernel_second_phase(capi, forest, monkeypatch, case):
    """130 children of 512 bins: 9 wave steps of 16 children (the last with 2), one step per group, 8 groups per phase — the
    ninth group is blockIdx.x / groups_per_phase / n_tiles = 1.  A column shard of 65 children has 5 steps, the last with one child."""
    sh, kn, n = plans(forest, monkeypatch, case)
    p = ref.plan_stationary(sh, kn, n)
    assert ref.descent_path(sh, kn, n) == ref.STATIONARY and p["uniform"] and p["children_per_step"] == 16, p
    if case[1] == 1:
        assert (p["n_steps"], p["steps_per_group"], p["n_groups"], p["groups_per_phase"], p["phases"]) == (9, 1, 9, 8, 2), p
        assert sh["n_children"] % p["children_per_step"] == 2 and p["grid"] == 16 * p["n_tiles"]
    else:
        assert p["n_steps"] == 5 and sh["n_children"] == 65, p
    probe_and_compare(capi, forest, case, n)


@pytest.mark.parametrize("tree", ["reg33x256", "reg33x256mixed"])
@pytest.mark.parametrize("unroll", [1, 2, 3, 4, 8])
def test_children_kernel_unrolls_and_tile_tails(capi, forest, monkeypatch, tree, unroll):
    """hibf_children_kernel<U, UNIFORM> for every U that exists, on tiles of 64 k-mers: a tile is 64 / (4 waves * U) rounds, and where
    that does not divide (U = 3, a last tile of 1 or 59 k-mers) the tail of a round repeats the tile's last k-mer.  Children of
    different rows and hash counts hash per lane, where U = 3 does not exist (4 runs); so does TXQ_HIBF_LANE_HASH=1 on equal children."""
    for case in [c for c in UNROLLS if c[0] == tree and c[3]["TXQ_HIBF_UNROLL"] == str(unroll)]:
        sh, kn, n = plans(forest, monkeypatch, case)
        p = ref.plan_stationary(sh, kn, n)
        lane_hash = "TXQ_HIBF_LANE_HASH" in case[3]
        assert ref.descent_path(sh, kn, n) == ref.STATIONARY and p["tile"] == 64 and p["n_tiles"] == -(-n // 64), p
        assert p["uniform"] == (tree == "reg33x256" and not lane_hash) and p["unroll"] == (unroll if p["uniform"] or unroll != 3 else 4), p
        if n > 64 and p["unroll"] > 1:
            assert (n % 64) % (4 * p["unroll"]) != 0  # the last tile ends inside a round
        probe_and_compare(capi, forest, case, n)
        monkeypatch.delenv("TXQ_HIBF_LANE_HASH", raising=False)


@pytest.mark.parametrize("case", ROOT_GRID, ids=case_id)
def test_root_pass_past_its_grid(capi, forest, monkeypatch, case):
    """hibf_root_kernel: i += gridDim.x * 256 beyond 8192 blocks, on the narrowest tree that takes the child-stationary path (9
    children of 128 bins, 18 mask words; its plain probes go to the interleaved children unless told otherwise).  All alive bits;
    the mask rows at both ends of the batch and around k-mer 2^21, where the root pass' second round begins."""
    sh, kn, n = plans(forest, monkeypatch, case)
    p = ref.plan_stationary(sh, kn, n)
    assert ref.descent_path(sh, kn, n) == ref.STATIONARY and sh["shard_words"] == 18 and p["uniform"], (sh, p)
    assert p["root_blocks"] == ref.ROOT_BLOCKS and n > ref.ROOT_BLOCKS * 256 == 1 << 21
    probe_and_compare(capi, forest, case, n, windows=[(0, 4096), ((1 << 21) - 4096, n)])


# ---- f. layout order: rows of plain k-mers through a session ---------------------------------------------------------------

@pytest.mark.parametrize("case", LAYOUT_CASES, ids=case_id)
def test_layout_order_rows_of_plain_kmers(capi, forest, monkeypatch, case):
    """One program per k-mer whose RESULT is that k-mer's mask: a session on a general tree computes the rows of its plain k-mers in
    layout order — hibf_fused_kernel<G, LAYOUT> writing the row directly (the default) or from LDS, on one wave per k-mer and on 8
    waves for all of them, and hibf_layout_level_kernel on three tiles, the last ragged — and turns the RESULT rows into user-bin
    order; split user bins are unified on the way.  The leaves of 4096 and 16 448 bins are G = 16 and G = 64 with two sweeps."""
    tree, env, n = case
    ub, ox, descs, base, want_base = forest[0](tree)
    ls = ref.layout_shape_of(ub, descs)
    assert ls is not None and ls["has_vnodes"]
    if tree in ("splitheavy", "layout3000"):
        assert ls["has_split"]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kn = ref.knobs(env)
    p, lv = ref.plan_fused_layout(ls, kn, n), ref.layout_level(ls, n)
    if env.get("TXQ_HIBF_LAYOUT_FUSED") == "0":
        assert not p["ok"] and lv["n_tiles"] == 3 and n % ref.LAYOUT_LEVEL_TILE and lv["grid"] == 24 * lv["phases"], (p, lv)
    else:
        assert p["ok"] and (p["row_lds_words"] == 0) == (env.get("TXQ_HIBF_LAYOUT_DIRECT") != "0"), p
        if "TXQ_HIBF_WAVES" in env:
            assert p["grid"] * p["waves_per_block"] == 8 and n > 600 * 8  # a wave takes some 625 k-mers
        if tree in WIDE:
            assert (p["G"], p["w_iters"]) == WIDE[tree][:2], p
    kmers = np.resize(base, n)
    blob = make_blob(kmers, [(3, [(i, 2, 1, 0)]) for i in range(n)])  # RESULT (slot 2) = ONES & M[k-mer i] | ZERO
    got = forest[1](tree).run_programs(blob, n)
    assert np.array_equal(got, want_base[np.arange(n) % P]), case_id(case)
