"""The executor (tetrex_amd/csrc/txq_exec.hip) beside helpers.SessionSimulator on hand-built version-4 sessions
(tests/blobs.py): inputs the frontier compiler never emits although include/txq_program.h allows them, internal state made
visible by observation twins (copy t of a program ends with RESULT = one of its slots or block entries), the raw alive answers
of every stage, and the refusals of validate_blob, plan_units and txq_session_stage.

tests/test_blobs.py shows on the CPU that every session used here is well-formed by the simulator's own checks and holds
every kind of op its cell is there for: a mismatch here is the device's."""
import numpy as np
import pytest

import blobs
from blobs import NO_KMER, DENSE_OP, dense_slot, dense_row, write_blob
from helpers import SessionSimulator

pytestmark = pytest.mark.gpu

KNOBS = ("TXQ_KMER_TABLE_MB", "TXQ_KMER_TABLE_MIN", "TXQ_DENSE_TREE", "TXQ_HIBF_LAYOUT_ORDER", "TXQ_FUSE_UNITS", "TXQ_SPARSE_STEPS")
ROWS = {"TXQ_KMER_TABLE_MB": "0"}  # dense steps take their rows from the index itself, not from its table of all k-mers' masks


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


_cells, _refs = {}, {}


def _cell(oracle, name):
    if name not in _cells:
        cell = blobs.build_cell(oracle, name)
        cell["meta"] = []
        cell["stages"] = blobs.cell_session(cell, cell["meta"])
        _cells[name] = cell
    return _cells[name]


def _reference(oracle, name, window=None):
    """The simulator's answers for a cell (on a column shard: window), computed once: (alive bytes per stage, final masks)."""
    key = (name, window)
    if key not in _refs:
        cell = _cell(oracle, name)
        sim = SessionSimulator(cell["ox"], len(cell["meta"]), dgram_index=cell.get("dg"), window=window)
        alive = [np.array(sim.stage(*st), dtype=np.uint8) for st in cell["stages"]]
        _refs[key] = (alive, np.stack([sim.result(p) for p in range(len(cell["meta"]))]))
    return _refs[key]


def _upload(capi, up, rank=0, shards=1):
    if up[0] == "ibf":
        return capi.Index.upload_ibf(*up[1:], shard_rank=rank, n_shards=shards)
    return capi.Index.upload_hibf(up[1], up[2], shard_rank=rank, n_shards=shards)


def _set(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _run(capi, oracle, monkeypatch, name, env, shards=1, alive_exact=True, dense=None):
    """Feeds the cell's session to a device session (per column shard) and compares, stage by stage, the alive bytes, and at
    the end every program's mask with the simulator's."""
    _set(monkeypatch, env)
    cell = _cell(oracle, name)
    meta, n = cell["meta"], len(cell["meta"])
    for r in range(shards):
        ix = _upload(capi, cell["upload"], r, shards)
        if dense is not None:
            assert ix.supports_dense() == dense
        aux = _upload(capi, cell["aux_upload"], r, shards) if "aux_upload" in cell else None
        window = None if shards == 1 else (int(ix.info.shard_word0), ix.shard_words)
        want_alive, want = _reference(oracle, name, window)
        s = ix.session(n)
        if aux is not None:
            s.set_aux_index(aux)
        for st, (blob, qp, qs) in enumerate(cell["stages"]):
            got = s.stage(blob, qp, qs, raw=True)
            assert got.dtype == np.uint8 and got.shape == want_alive[st].shape
            if alive_exact:
                bad = np.flatnonzero(got != want_alive[st])
            else:
                bad = np.flatnonzero(((got > 0) != (want_alive[st] > 0)) | (got < want_alive[st]))
            assert bad.size == 0, "%s shard %d stage %d: alive of program %d %r slot %d: device %d, simulator %d (%d answers differ)" % (
                name, r, st, qp[bad[0]], meta[qp[bad[0]]], qs[bad[0]], got[bad[0]], want_alive[st][bad[0]], bad.size)
        got = s.end()
        assert got.shape == want.shape
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, "%s shard %d: masks of %d programs differ, (kind, logical program, observed slot): %r" % (
            name, r, bad.size, [(int(p),) + tuple(meta[p]) for p in bad[:12]])
        if aux is not None:
            aux.free()
        ix.free()


FLAT_WAYS = {"default": {}, "units-not-fused": {"TXQ_FUSE_UNITS": "0"}, "steps-by-lane-groups": {"TXQ_SPARSE_STEPS": "0"}}


@pytest.mark.parametrize("way", sorted(FLAT_WAYS))
@pytest.mark.parametrize("bins", sorted(blobs.FLAT))
def test_flat_widths(capi, oracle, monkeypatch, bins, way):
    """W = 1, 2, 3 (narrow and wide lanes, by units), 32 (the last width stepped by units), 33 and 34 (sparse_kernel, narrow
    and wide), 141 (lanes loop over the mask); hash counts 1 to 5; tracked and untracked programs, big, small and empty ones
    in every stage."""
    _run(capi, oracle, monkeypatch, "flat-%d" % bins, dict(ROWS, **FLAT_WAYS[way]), dense=2)


def test_three_column_shards(capi, oracle, monkeypatch):
    """130 bins on three shards of one word: the simulator restricted to each shard's window; the last shard's ONES word is
    partly empty, and alive answers count the shard's bits only."""
    _run(capi, oracle, monkeypatch, "flat-130", ROWS, shards=3)


@pytest.mark.parametrize("mode", ["untracked", "tracked"])
@pytest.mark.parametrize("params", ["peptide3", "dna4", "reduced3", "peptide2"])
def test_dense_parameters(capi, oracle, monkeypatch, params, mode):
    """Peptide k = 3 (blocks of 400 entries), canonical DNA k = 4, a reduced alphabet of 10 codes at k = 3, and k = 2 — one
    suffix position: a step's destination entry is the rolled-in residue alone, the kernels' loops over the middle positions
    run zero times (pow_a[0] = 1, stride[0] = 1)."""
    _run(capi, oracle, monkeypatch, "%s-%s" % (params, mode), ROWS, dense=2)


@pytest.mark.parametrize("mode", ["untracked", "tracked"])
def test_rows_from_the_table_of_all_kmer_masks(capi, oracle, monkeypatch, mode):
    _run(capi, oracle, monkeypatch, "peptide3-%s" % mode, {"TXQ_KMER_TABLE_MIN": "1", "TXQ_KMER_TABLE_MB": "512"}, dense=2)


TREES = {"interleaved": ("16x64", {}), "tree": ("4x64", {"TXQ_DENSE_TREE": "1"}), "tree-by-lane": ("8x256-mixed", {"TXQ_DENSE_TREE": "2"})}


@pytest.mark.parametrize("mode", ["untracked", "tracked"])
@pytest.mark.parametrize("rows", sorted(TREES))
def test_rows_from_regular_trees(capi, oracle, monkeypatch, rows, mode):
    shape, env = TREES[rows]
    _run(capi, oracle, monkeypatch, "tree-%s-%s" % (shape, mode), dict(ROWS, **env), dense=2)


def test_descent_on_a_regular_tree(capi, oracle, monkeypatch):
    _run(capi, oracle, monkeypatch, "tree-16x64-untracked", dict(ROWS, TXQ_DENSE_TREE="0"), dense=1)


@pytest.mark.parametrize("mode", ["untracked", "tracked"])
def test_layout_order_tree(capi, oracle, monkeypatch, mode):
    """A general tree with split bins, masks in layout order (PathRows).  Until the session ends a mask there is a row over
    TECHNICAL bins: a user bin that is split over several technical bins has one bit per part (the parts are unified after
    every probe, so all of them carry the user bin's bit), and txq_session_end folds them into one.  The alive answers count
    the bits of that row, so they are compared as far as user-bin order defines them: zero exactly where the simulator's
    mask is empty, and never below the simulator's answer (every user bin with a bit has at least one technical bin with
    it).  Final masks — the twins' copies of internal slots and entries among them — are in user-bin order: bit-exact."""
    _run(capi, oracle, monkeypatch, "layout-%s" % mode, ROWS, alive_exact=False, dense=2)


def test_layout_tree_in_user_bin_order_descends(capi, oracle, monkeypatch):
    _run(capi, oracle, monkeypatch, "layout-untracked", dict(ROWS, TXQ_HIBF_LAYOUT_ORDER="0"), dense=1)


def test_tracked_programs_are_refused_where_steps_descend(capi, oracle, monkeypatch):
    _set(monkeypatch, dict(ROWS, TXQ_HIBF_LAYOUT_ORDER="0"))
    cell = _cell(oracle, "layout-tracked")
    ix = _upload(capi, cell["upload"])
    assert ix.supports_dense() != 2
    s = ix.session(len(cell["meta"]))
    with pytest.raises(capi.TxqError, match="tracked blocks need an index whose dense steps run fused") as e:
        s.stage(*cell["stages"][0])
    assert e.value.code == -6
    ix.free()


@pytest.mark.parametrize("way", ["default", "steps-by-lane-groups"])
def test_more_tracked_ops_in_a_level_than_one_launch_takes(capi, oracle, monkeypatch, way):
    """280 tracked programs with eight tiny blocks each: 2240 ZEROs and 1120 STEPs in one level, kMaxSparseGroups = 1024 groups a
    launch (run_sparse_groups cuts the level into several, each with its own counts and chunk prefix)."""
    _run(capi, oracle, monkeypatch, "many-tracked", dict(ROWS, **FLAT_WAYS[way]), dense=2)


def test_auxiliary_kmers(capi, oracle, monkeypatch):
    """The last n_aux_kmers entries of every stage's table are probed on a second flat IBF (same bins, other rows and hash
    count); ordinary ops take their k-mers from both halves."""
    cell = _cell(oracle, "aux")
    for blob, _, _ in cell["stages"]:
        n_main = cell["spec"]["n_kmers"]
        used = np.concatenate([ops[:, 0] for _, ops in blobs.host_programs(blob) if len(ops)])
        used = used[(used != NO_KMER) & (used != DENSE_OP)]
        assert (used < n_main).any() and (used >= n_main).any()
    _run(capi, oracle, monkeypatch, "aux", ROWS)


# ---- refusals -------------------------------------------------------------------------------------------------------------
# One valid version-4 blob of three programs (untracked blocks, tracked blocks, ordinary ops only); every malformed blob is
# this one with exactly one thing changed.  These cases stop on the host — no kernel is launched — but need an index handle.
P3 = blobs.PEPTIDE3
FULL = (1 << 20) - 1
T, NP = blobs.TRACKED, blobs.NOPROBE
B0, B1 = dense_slot(0), dense_slot(1)
G0, G1 = [0b1110, 0b110001], [0b1110001, 0b11000]  # tracked geometries: 3 x 3 and 4 x 2 entries; G1[0] holds G0[1]


def _base():
    dense = [
        dense_row(blobs.ZERO, B0),                                                   # 0
        dense_row(blobs.ZERO, B1, r_mask=1, shape=[0b111100, 0b1111]),               # 1
        dense_row(blobs.FILL, B1, src=3, shape=[0b1100, 0b0110]),                    # 2
        dense_row(blobs.STEP, B0, src=B1, r_mask=0b1010000, shape=[0b1100, 0b0110]),  # 3
        dense_row(blobs.REDUCE, 4, src=B0, shape=[FULL, FULL]),                      # 4
        dense_row(blobs.REDUCE, 2, src=B0, shape=[0b11111111, FULL]),                # 5
        dense_row(blobs.ZERO, B0, src=9, shape=G0, reserved=T),                      # 6
        dense_row(blobs.ZERO, B1, src=11, shape=G1, reserved=T),                     # 7
        dense_row(blobs.FILL, B0, src=3, shape=G0, reserved=T),                      # 8
        dense_row(blobs.STEP, B1, src=B0, r_mask=0b11000, shape=G0, reserved=T),     # 9
        dense_row(blobs.REDUCE, 2, src=B1, shape=G1, reserved=T),                    # 10
    ]
    D = lambda i: (DENSE_OP, i, 0, 0)
    programs = [
        [6, 2, False, [[D(0), (0, 3, 1, 0), (NO_KMER, 4, 0, 0)], [(1, dense_slot(0, 5), 3, 0), D(1)], [D(2)], [D(3)], [D(4), D(5)], [(NO_KMER, 2, 4, 2)]]],
        [5, 2, True, [[D(6), D(7), (2, 3, 1, 0)], [D(8)], [D(9)], [D(10), (NO_KMER, 4, dense_slot(1, 3), 0)]]],
        [5, 0, False, [[(3, 3, 1, 0), (4, 4, 1, 0)], [(NO_KMER, 2, 3, 4)]]],
    ]
    return dict(kmers=np.array([3, 1400, 777, 20000, 31000, 8], dtype=np.uint64), programs=programs, dense=dense, params=dict(P3), n_aux=0)


def _blob(s):
    return write_blob(s["kmers"], [tuple(p) for p in s["programs"]], dense=s["dense"], params=s["params"], n_aux_kmers=s["n_aux"])


def _mut(f):
    """a blob from the base structure after f changed it"""
    s = _base()
    f(s)
    return _blob(s)


def _set_row(i, **kw):
    names = dict(kind=0, dst=1, src=2, r_mask=3, reserved=15)
    def f(s):
        for k, v in kw.items():
            if k.startswith("shape"):
                s["dense"][i][4 + int(k[5:])] = v
            else:
                s["dense"][i][names[k]] = v
    return f


def _set_op(p, level, i, op):
    def f(s):
        s["programs"][p][3][level][i] = op
    return f


def _header(field, value, wide=False):
    blob = _blob(_base())
    return (blobs.patch_u64 if wide else blobs.patch_u32)(blob, blobs.FIELD[field], value)


def _table_word(table, index, value):
    """word `index` of the programs or levels table := value"""
    blob = _blob(_base())
    off = int.from_bytes(blob[blobs.FIELD[table + "_offset"]:blobs.FIELD[table + "_offset"] + 8], "little")
    return blobs.patch_u32(blob, off + 4 * index, value)


def _without_levels(p, ops):
    def f(s):
        s["programs"][p][3:] = [None, ops]
    return f


def _params(**kw):
    return lambda s: s["params"].update(kw)


N_OPS = 10 + 7 + 3  # ops of the three programs; their level tables hold 6 + 4 + 2 entries
MALFORMED = {
    "more auxiliary k-mers than k-mers": lambda: _mut(lambda s: s.update(n_aux=7)),
    "descending level table": lambda: _table_word("levels", 1, 1),
    "levels do not cover the ops": lambda: _table_word("levels", 5, 9),
    "levels run past the ops": lambda: _table_word("levels", 5, 11),
    "program's ops outside the table": lambda: _table_word("programs", 6 * 2 + 0, N_OPS + 1),
    "program's op count outside the table": lambda: _table_word("programs", 6 * 2 + 1, N_OPS),
    "program's levels outside the table": lambda: _table_word("programs", 6 * 2 + 3, 13),
    "program's level count outside the table": lambda: _table_word("programs", 6 * 2 + 4, 3),
    "ops table outside the blob": lambda: _header("ops_offset", len(_blob(_base())) + 8, wide=True),
    "k-mer table not 8-byte aligned": lambda: _header("kmers_offset", 100, wide=True),
    "dense table outside the blob": lambda: _header("dense_offset", len(_blob(_base())) - 56, wide=True),
    "n_dense past the blob": lambda: _header("n_dense", 12),
    "dense op in a program without levels": lambda: _mut(_without_levels(2, [(3, 3, 1, 0), (DENSE_OP, 0, 0, 0)])),
    "dense index >= n_dense": lambda: _mut(_set_op(0, 2, 0, (DENSE_OP, 11, 0, 0))),
    "kind 4": lambda: _mut(_set_row(2, kind=4)),
    "tracked op in an untracked program": lambda: _mut(_set_row(0, reserved=T)),
    "untracked op in a tracked program": lambda: _mut(_set_row(8, reserved=0)),
    "reserved bit above 1": lambda: _mut(_set_row(9, reserved=T | 4)),
    "NOPROBE on a REDUCE": lambda: _mut(_set_row(10, reserved=T | NP)),
    "NOPROBE on an untracked STEP": lambda: _mut(_set_row(3, reserved=NP)),
    "dst inside a block": lambda: _mut(_set_row(3, dst=B0 | 1)),
    "src inside a block": lambda: _mut(_set_row(3, src=B1 | 1)),
    "ZERO of an ordinary slot": lambda: _mut(_set_row(0, dst=3)),
    "block id >= n_blocks": lambda: _mut(_set_row(0, dst=dense_slot(2))),
    "src block id >= n_blocks": lambda: _mut(_set_row(4, src=dense_slot(2))),
    "untracked entry >= A^(k-1)": lambda: _mut(_set_op(0, 1, 0, (1, dense_slot(0, 400), 3, 0))),
    "entry of a block id >= n_blocks": lambda: _mut(_set_op(0, 1, 0, (1, dense_slot(2, 0), 3, 0))),
    "STEP onto its source": lambda: _mut(_set_row(3, src=B0)),
    "r_mask with a code >= A": lambda: _mut(_set_row(3, r_mask=0b1010000 | 1 << 20)),
    "shape with a code >= A": lambda: _mut(_set_row(3, shape1=0b0110 | 1 << 25)),
    "REDUCE shape with a code >= A": lambda: _mut(_set_row(4, shape0=FULL | 1 << 20)),
    "REDUCE into ZERO": lambda: _mut(_set_row(4, dst=0)),
    "REDUCE into ONES": lambda: _mut(_set_row(4, dst=1)),
    "REDUCE into a slot >= n_slots": lambda: _mut(_set_row(4, dst=6)),
    "tracked REDUCE into a block entry": lambda: _mut(_set_row(10, dst=dense_slot(0, 0))),
    "tracked ZERO with an empty position": lambda: _mut(_set_row(6, shape1=0)),
    "tracked ZERO, capacity below its geometry": lambda: _mut(_set_row(6, src=8)),
    "tracked ZERO, capacity above 2^22": lambda: _mut(_set_row(6, src=(1 << 22) + 1)),
    "FILL from a dense slot": lambda: _mut(_set_row(2, src=dense_slot(0, 5))),
    "FILL from a slot >= n_slots": lambda: _mut(_set_row(2, src=6)),
    "block entry in a program without levels": lambda: _mut(_without_levels(0, [(0, 3, 1, 0), (1, dense_slot(0, 5), 3, 0)])),
    "slot with bit 31": lambda: _mut(_set_op(2, 0, 0, (3, 3, 0x80000001, 0))),
    "dst with bit 31": lambda: _mut(_set_op(2, 0, 0, (3, 0x80000003, 1, 0))),
    "dst >= n_slots": lambda: _mut(_set_op(2, 0, 0, (3, 5, 1, 0))),
    "writes ONES": lambda: _mut(_set_op(2, 0, 0, (3, 1, 1, 0))),
    "k-mer index >= n_kmers": lambda: _mut(_set_op(2, 0, 0, (6, 3, 1, 0))),
    "n_slots below 3": lambda: _table_word("programs", 6 * 2 + 2, 2),
    "n_slots with the dense bit": lambda: _table_word("programs", 6 * 2 + 2, 0x40000000),
    "k - 1 > 11": lambda: _mut(_params(k=13, bits=2, alphabet=4)),
    "k = 1": lambda: _mut(_params(k=1)),
    "bits * k > 64": lambda: _mut(_params(k=9, bits=8)),
    "A > 2^bits": lambda: _mut(_params(bits=4)),
    "canonical with bits != 2": lambda: _mut(_params(canonical=1)),
    "A^(k-1) > 2^22": lambda: _mut(_params(k=7)),
    "more than 256 blocks": lambda: _mut(lambda s: s["programs"][0].__setitem__(1, 257)),
    "version 3": lambda: _header("version", 3),
    "program count differs from the session's": lambda: _header("n_programs", 2),
}


def _other_k():
    """a valid blob whose blocks have another size (k = 2: 20 entries), no ops"""
    return write_blob(np.zeros(0, dtype=np.uint64), [(6, 2, False, []), (5, 2, True, []), (5, 0, False, [])], dense=[], params=blobs.PEPTIDE2)


# (first stage or None, the refused stage as (blob, query programs, query slots), expected code)
SESSION_LEVEL = {
    "block size changes between stages": lambda: (_blob(_base()), (_other_k(), [], []), -6),
    "program turns tracked": lambda: (_blob(_base()), (_mut(lambda s: s.update(programs=[[6, 2, True, []], [5, 2, True, []], [5, 0, False, []]], dense=[])), [], []), -6),
    "program turns untracked": lambda: (_blob(_base()), (_mut(lambda s: s.update(programs=[[6, 2, False, []], [5, 2, False, []], [5, 0, False, []]], dense=[])), [], []), -6),
    "tracked block id changes its capacity": lambda: (_blob(_base()), (_mut(_set_row(7, src=12)), [], []), -6),
    "op on a tracked block that no ZERO created": lambda: (None, (_mut(lambda s: s["programs"][1][3].__setitem__(0, [(DENSE_OP, 6, 0, 0), (2, 3, 1, 0)])), [], []), -6),
    "ordinary op on a tracked block that no ZERO created": lambda: (None, (_mut(lambda s: s["programs"][1].__setitem__(3, [[(2, 3, 1, 0)], [(NO_KMER, 4, dense_slot(1, 3), 0)]])), [], []), -6),
    "tracked entry beyond the capacity": lambda: (None, (_mut(_set_op(1, 3, 1, (NO_KMER, 4, dense_slot(1, 11), 0))), [], []), -6),
    "feedback program out of range": lambda: (None, (_blob(_base()), [3], [0]), -1),
    "feedback slot out of range": lambda: (None, (_blob(_base()), [2], [5]), -1),
    "feedback on a dense slot": lambda: (None, (_blob(_base()), [0], [dense_slot(0, 5)]), -1),
    "feedback on a program that has not run": lambda: (None, (_mut(lambda s: s["programs"][2].__setitem__(3, [])), [2], [0]), -1),
    "auxiliary k-mers without an auxiliary index": lambda: (None, (_mut(lambda s: s.update(n_aux=2)), [], []), -4),
}


@pytest.fixture(scope="module")
def small_index(capi, oracle):
    import helpers
    bins, m, h = 130, 509, 2
    words = helpers.random_words(bins, m, 0.8, 77)
    ox = helpers.oracle_ibf_from_words(oracle, bins, m, h, words, k=3)
    ix = capi.Index.upload_ibf(bins, m, h, words)
    yield ox, ix
    ix.free()


def _close(capi, sess):
    capi.lib().txq_session_end(sess._h, None)
    sess._h = None


def _base_is_still_right(capi, ox, ix):
    """the unmutated blob on a fresh session of the same index: the simulator's masks and alive bytes"""
    blob = _blob(_base())
    qp, qs = [0, 0, 1, 1, 2, 2], [4, 0, 3, 4, 3, 2]
    sim = SessionSimulator(ox, 3)
    want_alive = sim.stage(blob, qp, qs)
    sess = ix.session(3)
    assert sess.stage(blob, qp, qs, raw=True).tolist() == want_alive
    got = sess.end()
    for p in range(3):
        assert np.array_equal(got[p], sim.result(p)), p
        assert got[p].any()
    assert sim.dense_kinds == [4, 2, 3, 2] and sim.tracked_ops == 5


def test_the_base_blob_is_valid(capi, small_index, monkeypatch):
    _set(monkeypatch, ROWS)
    _base_is_still_right(capi, *small_index)


@pytest.mark.parametrize("what", sorted(MALFORMED))
def test_malformed_blobs_are_refused(capi, small_index, monkeypatch, what):
    _set(monkeypatch, ROWS)
    ox, ix = small_index
    base, bad = _blob(_base()), MALFORMED[what]()
    assert bad != base and len(bad) == len(base) or what in ("dense op in a program without levels", "block entry in a program without levels")
    sess = ix.session(3)
    with pytest.raises(capi.TxqError) as e:
        sess.stage(bad)
    assert e.value.code == -6, str(e.value)
    _close(capi, sess)
    with pytest.raises(capi.TxqError) as e:  # the one-stage entry point validates the same way
        ix.run_programs(bad, 3)
    assert e.value.code == -6
    _base_is_still_right(capi, ox, ix)


@pytest.mark.parametrize("what", sorted(SESSION_LEVEL))
def test_stages_a_session_cannot_take_are_refused(capi, small_index, monkeypatch, what):
    _set(monkeypatch, ROWS)
    ox, ix = small_index
    first, (bad, qp, qs), code = SESSION_LEVEL[what]()
    sess = ix.session(3)
    if first is not None:
        sess.stage(first)
    with pytest.raises(capi.TxqError) as e:
        sess.stage(bad, qp, qs)
    assert e.value.code == code, str(e.value)
    _close(capi, sess)
    if first is not None or qp:  # what was refused is a valid first stage of a session that asks nothing
        sim = SessionSimulator(ox, 3)
        sim.stage(bad, [], [])
        sess = ix.session(3)
        sess.stage(bad)
        got = sess.end()
        assert all(np.array_equal(got[p], sim.result(p)) for p in range(3))
    _base_is_still_right(capi, ox, ix)
