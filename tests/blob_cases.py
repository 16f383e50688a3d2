"""One valid version-4 blob of three programs and everything that can be wrong with it: the malformed blobs validate_blob
refuses (MALFORMED) and the stages a session cannot take (SESSION_LEVEL).  tests/test_gpu_exec_blobs.py hands them to a device
session; tests/test_exec_plan.py to the host-side planner (csrc/txq_exec_plan.hpp) alone, without a GPU."""
import numpy as np

import blobs
from blobs import NO_KMER, DENSE_OP, dense_slot, dense_row, write_blob

# One valid version-4 blob of three programs (untracked blocks, tracked blocks, ordinary ops only); every malformed blob is
# this one with exactly one thing changed.
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


# ---- the index these cases, and the sessions of golden/exec_plan_sessions.json, run on ------------------------------------
SMALL_INDEX = (130, 509, 2)  # bins, rows, hash functions


def small_index_words():
    import helpers
    bins, m, _ = SMALL_INDEX
    return helpers.random_words(bins, m, 0.8, 77)


def small_oracle_index(oracle):
    import helpers
    bins, m, h = SMALL_INDEX
    return helpers.oracle_ibf_from_words(oracle, bins, m, h, small_index_words(), k=3)


def simulate(ox, stages):
    """a session on the simulator: (alive bytes per stage, final masks [programs][W])"""
    import struct
    from helpers import SessionSimulator
    n = struct.unpack_from("<I", stages[0][0], blobs.FIELD["n_programs"])[0]
    sim = SessionSimulator(ox, n)
    alive = [np.array(sim.stage(blob, qp, qs), dtype=np.uint8) for blob, qp, qs in stages]
    return alive, np.stack([sim.result(p) if sim.result(p) is not None else np.zeros(sim.W, dtype=np.uint64) for p in range(n)])
