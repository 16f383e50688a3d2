"""The executor (tetrex_amd/csrc/txq_exec.hip) beside helpers.SessionSimulator on hand-built version-4 sessions
(tests/blobs.py): inputs the frontier compiler never emits although include/txq_program.h allows them, internal state made
visible by observation twins (copy t of a program ends with RESULT = one of its slots or block entries), the raw alive answers
of every stage, and the refusals of validate_blob, plan_units and txq_session_stage.

tests/test_blobs.py shows on the CPU that every session used here is well-formed by the simulator's own checks and holds
every kind of op its cell is there for: a mismatch here is the device's."""
import numpy as np
import pytest

import blobs
from blobs import NO_KMER, DENSE_OP
from blob_cases import MALFORMED, SESSION_LEVEL, _base, _blob
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
# The malformed blobs and the stages a session cannot take: tests/blob_cases.py (tests/test_exec_plan.py runs them without a GPU).
# These cases stop on the host — no kernel is launched — but need an index handle.


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
