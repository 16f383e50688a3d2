#!/usr/bin/env python3
"""Writes exec_plan_sessions.json: the sessions that tests/test_exec_plan.py plans on the CPU (tests/native/exec_plan_dump.cpp)
and tests/test_gpu_exec_plan.py runs on a device beside the simulator.

  python tests/golden/make_exec_plan_sessions.py

"sessions": name -> stages [blob as hex, question programs, question slots]; "cases": name -> the runs of one script of the
dump program, each a session by name with the W, G_dense, dense_tile_rounds and hibf it is planned with (the runs of a case
follow each other on one index: a run adopts what the one before it handed back).  The blobs come from tests/blobs.py and
tests/blob_cases.py with fixed seeds.

exec_plan_expected.json (what the plans must be) is NOT made here: its values were taken from the executor as it was before
the planner was split from it (tests/golden/README.md)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import blobs  # noqa: E402
from blobs import NO_KMER, DENSE_OP, ZERO, REDUCE, TRACKED, dense_slot, dense_row, write_blob  # noqa: E402
from blob_cases import _base, _blob, _mut, _set_row  # noqa: E402
from helpers import make_blob  # noqa: E402

P3 = blobs.PEPTIDE3
FULL = (1 << 20) - 1
BASE_QUESTIONS = ([0, 0, 1, 1, 2, 2], [4, 0, 3, 4, 3, 2])


def generated(seed, mode):
    """a session of tests/blobs.py random_session, cut down: sized for masks of 1024 words (a program of 32 ops is a big one),
    no observation twins, short fan-ins"""
    spec = dict(W=1024, n_kmers=16, kmer_pool=blobs.valid_kmers(P3), dense=dict(P3), dense_mode=mode, twins=1, fan_in=(40,), big=((8, 4),))
    return blobs.random_session(np.random.default_rng(seed), spec)


def versions():
    """three programs through blobs of version 1 (op order), 2 (levels) and 4 (levels and dense ops)"""
    kmers = np.array([3, 1400, 777, 20000, 31000, 8], dtype=np.uint64)
    v1 = make_blob(kmers, [(6, [(0, 3, 1, 0), (1, 4, 3, 0), (NO_KMER, 2, 4, 0)]), (5, [(2, 3, 1, 0), (NO_KMER, 2, 3, 0)]), (5, [(4, 3, 1, 0), (NO_KMER, 4, 0, 0)])])
    v2 = write_blob(kmers, [(6, 0, False, [[(1, 5, 3, 0)], [(NO_KMER, 2, 2, 5)]]), (5, 0, False, None, [(3, 4, 3, 0), (NO_KMER, 2, 2, 4)]), (5, 0, False, [])])
    return [(v1, [0, 1], [4, 3]), (v2, [0, 1, 2], [5, 4, 3]), (_blob(_base()),) + BASE_QUESTIONS]


def region_growth():
    """program 0's region: 8 slots with its first ops, doubled to 16, then moved to the 40 it needs; program 1 begins in stage 1"""
    kmers = np.array([5, 900, 4242], dtype=np.uint64)
    stages = []
    for n0, n1, ops1 in ((7, 3, []), (11, 5, [[(1, 3, 1, 0)], [(NO_KMER, 2, 3, 0)]]), (40, 5, [[(2, 4, 3, 0)]])):
        top = n0 - 1
        ops0 = [[(0, top, 1, 0)], [(NO_KMER, 2, 2, top)]] if n0 == 7 else [[(1, top, 3, 0)], [(NO_KMER, 2, 2, top)]]
        if n0 == 7:
            ops0[0].append((2, 3, 1, 0))
        stages.append((write_blob(kmers, [(n0, 0, False, ops0), (n1, 0, False, ops1)]), [0], [top]))
    return stages


def blocks_recycled():
    """program 0 gives its two blocks back in stage 1; programs 1, 2 and 3 take two blocks each in stages 1, 2 and 3"""
    kmers = np.array([17, 2500, 7000], dtype=np.uint64)
    B0, B1 = dense_slot(0), dense_slot(1)
    stages = []
    for st in range(4):
        dense, table = [], []
        for p in range(4):
            if p != st:
                table.append((4, 2 if p == 0 and st == 0 or 0 < p < st else 0, False, []))
                continue
            dense += [dense_row(ZERO, B0), dense_row(ZERO, B1), dense_row(REDUCE, 2, src=B1, shape=[FULL, FULL])]
            n = len(dense)
            table.append((4, 2, False, [[(DENSE_OP, n - 3, 0, 0), (DENSE_OP, n - 2, 0, 0), (p % 3, 3, 1, 0)], [(1, dense_slot(1, 7 + p), 3, 0)],
                                        [(DENSE_OP, n - 1, 0, 0)]]))
        stages.append((write_blob(kmers, table, dense=dense, params=P3), [st], [3]))
    return stages


def main():
    base = _blob(_base())
    three_blocks = _mut(lambda s: s["programs"][0].__setitem__(1, 3))  # program 0 holds a third untracked block it never touches
    takes_garbage = _mut(_set_row(7, src=400))                         # the tracked block 1 gets the capacity of an untracked block

    def zero_beside_step(s):  # the tracked program creates a third block in the level of its STEP: [ZERO | STEP] in one level's sparse groups
        s["dense"].append(dense_row(ZERO, dense_slot(2), src=9, shape=[0b1110, 0b110001], reserved=TRACKED))
        s["programs"][1][1] = 3
        s["programs"][1][3][2].append((DENSE_OP, 11, 0, 0))
    sessions = {
        "both": generated(11, "both"),
        "untracked": generated(12, "untracked"),
        "versions": versions(),
        "region_growth": region_growth(),
        "blocks_recycled": blocks_recycled(),
        "base": [(base,) + BASE_QUESTIONS],
        "base_three_blocks": [(three_blocks,) + BASE_QUESTIONS],
        "base_takes_garbage": [(takes_garbage,) + BASE_QUESTIONS],
        "base_zero_beside_step": [(_mut(zero_beside_step),) + BASE_QUESTIONS],
    }
    run = lambda name, W=3, G=8, rounds=4, hibf=0: dict(session=name, W=W, G_dense=G, rounds=rounds, hibf=hibf)
    cases = {
        "both_w1024": [run("both", W=1024, G=64, rounds=2)],
        "untracked_w3": [run("untracked")],
        "untracked_hibf_w262144": [run("untracked", W=1 << 18, G=64, hibf=1)],
        "versions": [run("versions")],
        "region_growth": [run("region_growth")],
        "blocks_recycled_two_stages_later": [run("blocks_recycled")],
        "base": [run("base")],
        "tracked_zero_beside_step": [run("base_zero_beside_step")],
        # the second session finds the first one's blocks: a tracked program's as it left them, an untracked program's to be
        # cleared; the third has masks of another width and starts the blocks' chunks over
        "pool_adopted": [run("base_three_blocks"), run("base_takes_garbage"), run("base", W=5)],
    }
    out = dict(sessions={k: [[b.hex(), [int(x) for x in qp], [int(x) for x in qs]] for b, qp, qs in v] for k, v in sessions.items()}, cases=cases)
    path = os.path.join(HERE, "exec_plan_sessions.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(path, os.path.getsize(path), {k: sum(len(b) for b, _, _ in v) for k, v in sessions.items()})


if __name__ == "__main__":
    main()
