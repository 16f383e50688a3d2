"""The blob writer of tests/blobs.py against the host's parsers, and its session generator against the simulator's own
well-formedness checks: every session the GPU tests run (tests/test_gpu_exec_blobs.py) is well-formed and contains every kind
of op they claim to cover.  No GPU."""
import numpy as np
import pytest

import blobs
from blobs import NO_KMER, DENSE_OP, dense_slot, dense_row, write_blob
from helpers import SessionSimulator


def test_writer_round_trips_through_the_host_parsers():
    from tetrex_amd import host
    rng = np.random.default_rng(1)
    kmers = rng.integers(0, 1 << 40, size=7, dtype=np.uint64)  # (an odd number of tables' worth of padding is exercised below)
    par = dict(k=3, bits=5, alphabet=20, canonical=0)
    dense = [dense_row(blobs.ZERO, dense_slot(0)), dense_row(blobs.STEP, dense_slot(1), src=dense_slot(0), r_mask=0x5, shape=[0xFFFFF, 0x3]),
             dense_row(blobs.ZERO, dense_slot(2), src=17, shape=[0x7, 0x30], reserved=blobs.TRACKED)]
    programs = [(9, 2, False, [[(0, 3, 1, 0), (DENSE_OP, 0, 0, 0)], [(DENSE_OP, 1, 0, 0)], [(NO_KMER, 2, dense_slot(1, 45), 2)]]),
                (3, 0, False, []),
                (5, 3, True, [[(DENSE_OP, 2, 0, 0)], [], [(6, 4, 1, 0), (NO_KMER, 2, 4, 2), (NO_KMER, 2, 2, 4)]]),
                (4, 0, False, None, [(1, 3, 1, 0), (NO_KMER, 2, 3, 0)])]
    for params, n_aux in ((par, 2), (None, 0), (None, 3)):
        progs = programs if params else [(p[0], 0, False) + tuple(p[3:]) for p in (programs[1], programs[3], (6, 0, False, [[(2, 5, 1, 0)], [(NO_KMER, 2, 5, 2)]]))]
        blob = write_blob(kmers, progs, dense=dense if params else None, params=params, n_aux_kmers=n_aux)
        got_kmers, got = host.parse_blob(blob)
        assert np.array_equal(got_kmers, kmers) and len(got) == len(progs)
        levels = host.blob_levels(blob)
        for p, g, lv in zip(progs, got, levels):
            want_ops = [op for l in p[3] for op in l] if p[3] is not None else list(p[4])
            assert g[0] == p[0]
            assert [tuple(int(x) for x in op) for op in g[1]] == [tuple(op) for op in want_ops]
            assert lv == ([] if p[3] is None else list(np.cumsum([len(l) for l in p[3]], dtype=np.int64)))
        assert host.blob_aux_kmers(blob) == n_aux
        d = host.blob_dense(blob)
        if params is None:
            assert d is None
        else:
            assert d[0] == par
            assert d[1].tolist() == dense
            assert d[2] == [2, 0, 3 | blobs.TRACKED_BIT, 0]
        for field in ("kmers_offset", "programs_offset", "ops_offset", "levels_offset") + (("dense_offset",) if params else ()):
            assert int.from_bytes(blob[blobs.FIELD[field]:blobs.FIELD[field] + 8], "little") % 8 == 0


def test_slot_and_entry_helpers():
    assert dense_slot(3, 77) == 0x40000000 | (3 << 22) | 77
    full = [(1 << 20) - 1] * 2
    assert blobs.entry_index(full, [7, 13]) == 7 * 20 + 13
    assert blobs.entry_index([0b10110, 0b1001], [4, 3]) == 2 * 2 + 1  # ranks (2, 1) in sets of sizes (3, 2)


def test_session_of_many_tracked_programs(oracle):
    """more tracked dense ops in one level than one launch of the sparse kernels takes (kMaxSparseGroups = 1024)"""
    cell = blobs.build_cell(oracle, "many-tracked")
    stages = blobs.cell_session(cell)
    n = len(blobs.host_programs(stages[0][0]))
    sim = SessionSimulator(cell["ox"], n)
    for blob, qp, qs in stages:
        sim.stage(blob, qp, qs)
    from tetrex_amd import host
    table = host.blob_dense(stages[0][0])[1]
    per_level = {}
    for (n_slots, ops), ends in zip(blobs.host_programs(stages[0][0]), blobs.host_levels(stages[0][0])):
        begin = 0
        for l, end in enumerate(ends):
            for o in ops[begin:end]:
                if int(o[0]) == DENSE_OP:
                    kind = int(table[int(o[1])][0])
                    per_level[(l, kind == blobs.STEP)] = per_level.get((l, kind == blobs.STEP), 0) + 1
            begin = end
    assert per_level[(0, False)] > 2048 and per_level[(2, True)] > 1024
    assert sum(1 for p in range(n) if sim.result(p).any()) > n // 2


@pytest.mark.parametrize("name", sorted(set(blobs.CELLS) - {"many-tracked"}))
def test_generated_sessions_are_well_formed_and_complete(oracle, name):
    """The session of every GPU cell runs through the simulator without one of its assertions firing (operands defined, dense
    ops inside their blocks' shapes and geometries, the level race rules), and holds every kind of op the cell is there for."""
    cell = blobs.build_cell(oracle, name)
    stages = blobs.cell_session(cell)
    spec = cell["spec"]
    n = len(blobs.host_programs(stages[0][0]))
    sim = SessionSimulator(cell["ox"], n, dgram_index=cell.get("dg"))
    sizes = set()
    for blob, qp, qs in stages:
        alive = sim.stage(blob, qp, qs)
        assert len(alive) == len(qp) > 0 and 0 in alive and max(alive) > 0  # feedback in every stage, some of it all-zero
        levels = blobs.host_levels(blob)
        for (n_slots, ops), lv in zip(blobs.host_programs(blob), levels):
            dense = any(int(o[0]) == DENSE_OP or ((int(o[1]) | int(o[2]) | int(o[3])) & blobs.DENSE_BIT and int(o[0]) != DENSE_OP) for o in ops) if len(ops) < 4000 else False
            sizes.add("none" if not len(ops) else "dense" if dense else "big" if len(ops) * spec["W"] >= 32768 else "small")
    assert sizes == {"none", "small", "big", "dense"}
    blobs.check_kinds(sim, spec)
    assert blobs.kinds_wanted(spec) <= blobs.inventory(stages), blobs.kinds_wanted(spec) - blobs.inventory(stages)
    results = [sim.result(p) for p in range(n)]
    assert sum(1 for r in results if r.any()) > n // 2 and any(not r.any() for r in results)
    last = stages[-1][0]
    assert len({lv[-1] if lv else 0 for lv in blobs.host_levels(last)}) > 3
