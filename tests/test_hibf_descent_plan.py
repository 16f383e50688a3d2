"""The path choice and launch arithmetic of the HIBF descent (csrc/txq_hibf_descent_plan.hpp) without a GPU:
tests/native/hibf_descent_plan_dump.cpp, built with the address and undefined-behaviour sanitizers, answers one command per line.
A table of plans worked out by hand — one for each boundary between two paths and one for each cap of a grid — and the Python
restatement of tests/hibf_descent_ref.py against the header: on every tree, batch and switch setting tests/test_gpu_hibf_scale.py
uses (that file asks the restatement whether a case reaches the loop it is written for) and on a few hundred random shapes."""
import os
import subprocess

import numpy as np
import pytest

import hibf_descent_ref as ref
from conftest import ROOT


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hibf_descent_plan") / "hibf_descent_plan_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(ROOT, "tests", "native", "hibf_descent_plan_dump.cpp")], check=True, timeout=600)

    def run(lines):
        r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


# A general tree of 300 user bins: 5 mask words, 10 IBFs of at most 128 bins (rows of 2 words), 4 IBFs on its widest level.
GENERAL = dict(shard_words=5, n_ibf=10, total_tbs=400, max_stride=2, max_level_width=4, depth=3, has_nodes=1, n_children=0, child_row_words=0,
               children_bytes=0, children_uniform=0, root_stride=2, probes_interleaved=0)
# Regular trees: 9 children of 128 bins (18 mask words, rows of 1000 x 2 words), 130 children of 512 bins, 256 of 256
REG9 = dict(shard_words=18, n_ibf=10, total_tbs=9 + 9 * 128, max_stride=2, max_level_width=9, depth=2, has_nodes=1, n_children=9, child_row_words=2,
            children_bytes=9 * 1000 * 2 * 8, children_uniform=1, root_stride=1, probes_interleaved=0)
REG130 = dict(shard_words=1040, n_ibf=131, total_tbs=130 + 130 * 512, max_stride=8, max_level_width=130, depth=2, has_nodes=1, n_children=130, child_row_words=8,
              children_bytes=130 * 1000 * 8 * 8, children_uniform=1, root_stride=4, probes_interleaved=0)
REG256 = dict(REG130, shard_words=1024, n_ibf=257, total_tbs=256 + 65536, max_stride=4, max_level_width=256, n_children=256, child_row_words=4,
              children_bytes=256 * 1000 * 4 * 8)
# One IBF of 16 448 bins: rows of 257 words, stride 258
LEAF = dict(GENERAL, shard_words=257, n_ibf=1, total_tbs=16448, max_stride=258, max_level_width=1, depth=1, root_stride=258)

# (shape, changes to the shape, switches, n) -> the numbers named (hibf_descent_ref.DESCENT_FIELDS)
HAND = [
    # ---- path boundaries
    (GENERAL, dict(probes_interleaved=1), {}, 1000, {"path": ref.INTERLEAVED}),
    (GENERAL, {}, {}, 1000, {"path": ref.SMALL, "small.applies": 1, "small.blocks": 4}),
    (GENERAL, dict(n_ibf=32), {}, 1000, {"path": ref.SMALL}),
    (GENERAL, dict(n_ibf=33), {}, 1000, {"path": ref.FUSED}),                 # more IBFs than the small kernel's stack
    (GENERAL, dict(shard_words=16), {}, 1000, {"path": ref.SMALL}),
    (GENERAL, dict(shard_words=17), {}, 1000, {"path": ref.FUSED}),
    (GENERAL, dict(max_stride=4), {}, 1000, {"path": ref.SMALL}),
    (GENERAL, dict(max_stride=6), {}, 1000, {"path": ref.FUSED}),                 # an IBF of more than 256 bins
    (GENERAL, dict(total_tbs=0xFFFE), {}, 1000, {"path": ref.SMALL}),
    (GENERAL, dict(total_tbs=0xFFFF), {}, 1000, {"path": ref.FUSED}),             # a technical-bin index does not fit 16 bits
    (GENERAL, {}, dict(small=0), 1000, {"path": ref.FUSED, "small.applies": 0}),
    (GENERAL, {}, dict(levels=1), 1000, {"path": ref.LEVELS, "fused.ok": 0}),
    (GENERAL, dict(has_nodes=0), {}, 1000, {"path": ref.LEVELS}),
    (GENERAL, dict(shard_words=0), {}, 1000, {"path": ref.LEVELS}),
    # 10 IBFs: the whole stack (10 entries, 5 words) is in LDS; 8187 + 5 words are 64 KiB exactly, one word more is too much
    (GENERAL, dict(shard_words=8187), {}, 1000, {"path": ref.FUSED, "fused.stack_lds": 10, "fused.wave_bytes": 65536, "fused.waves_per_block": 1}),
    (GENERAL, dict(shard_words=8188), {}, 1000, {"path": ref.LEVELS, "fused.wave_bytes": 65544}),
    (REG9, {}, {}, 1000, {"path": ref.STATIONARY, "stat.lanes_per_child": 1, "stat.n_steps": 1, "stat.n_groups": 1, "stat.groups_per_phase": 1, "stat.phases": 1,
                          "stat.grid": 1, "stat.root_blocks": 4, "stat.uniform": 1, "stat.unroll": 1}),
    (REG9, dict(shard_words=16, n_children=8), {}, 1000, {"path": ref.SMALL, "stat.ok": 0}),  # 16 mask words: the small kernel
    (REG9, dict(child_row_words=1), {}, 1000, {"path": ref.FUSED, "stat.ok": 0}),             # (18 words: not small) children of one word
    (REG9, {}, dict(stationary=0), 1000, {"path": ref.FUSED, "stat.ok": 0}),
    (REG9, {}, dict(levels=1), 1000, {"path": ref.LEVELS}),                                    # the gate in front of all three kernels
    # ---- 1. fused kernel: 16 384 waves, or TXQ_HIBF_WAVES; (5 + 5) words = 80 bytes per wave, blocks of four waves
    (GENERAL, {}, dict(small=0), 2 * 16384 + 77, {"fused.ok": 1, "fused.wave_bytes": 80, "fused.waves_per_block": 4, "fused.grid": 4096, "fused.G": 1, "fused.w_iters": 1}),
    (GENERAL, {}, dict(small=0), 16385, {"fused.grid": 4096}),
    (GENERAL, {}, dict(small=0), 16383, {"fused.grid": 4096}),
    (GENERAL, {}, dict(small=0), 1000, {"fused.grid": 250}),
    (GENERAL, {}, dict(small=0, waves=1), 1000, {"fused.grid": 1}),
    (GENERAL, {}, dict(small=0, waves=3), 1000, {"fused.grid": 1}),                # (a block of four waves: four run)
    (GENERAL, {}, dict(small=0, waves=64), 1000, {"fused.grid": 16}),
    (GENERAL, {}, dict(small=0, waves=512), 100, {"fused.grid": 25}),              # fewer k-mers than waves
    # the stack: TXQ_HIBF_STACK_LDS entries in LDS when the output row (2 entries per word) takes the rest, else all of it
    (GENERAL, dict(n_ibf=150, shard_words=94), dict(stack_lds=2), 564, {"fused.stack_lds": 2, "fused.wave_bytes": (94 + 1) * 8}),
    (GENERAL, dict(n_ibf=190, shard_words=94), dict(stack_lds=2), 564, {"fused.stack_lds": 2}),
    (GENERAL, dict(n_ibf=191, shard_words=94), dict(stack_lds=2), 564, {"fused.stack_lds": 192}),
    (GENERAL, dict(n_ibf=150, shard_words=94), dict(stack_lds=3), 564, {"fused.stack_lds": 2}),
    (GENERAL, dict(n_ibf=150, shard_words=94), {}, 564, {"fused.stack_lds": 128}),
    (GENERAL, dict(n_ibf=128, shard_words=94), {}, 564, {"fused.stack_lds": 128}),
    # an 11 KB row: 12 resident waves in blocks of four (3 x 44 800 bytes) against 14 in blocks of two (7 x 23 040); single waves: 14 as well
    (GENERAL, dict(shard_words=1375, n_ibf=2), {}, 1000, {"fused.wave_bytes": 11008, "fused.waves_per_block": 2, "fused.grid": 500}),
    # ---- 2. G and w_iters: a lane of the fused kernel owns four row words, a lane of the level kernel one
    (GENERAL, dict(max_stride=32, shard_words=40), {}, 1000, {"fused.G": 8, "fused.w_iters": 1, "lev.G": 32, "lev.w_iters": 1}),   # 2048 bins
    (GENERAL, dict(max_stride=64, shard_words=64), {}, 1000, {"fused.G": 16, "fused.w_iters": 1, "lev.G": 64, "lev.w_iters": 1}),  # 4096 bins
    (GENERAL, dict(max_stride=128, shard_words=128), {}, 1000, {"fused.G": 32, "fused.w_iters": 1, "lev.G": 64, "lev.w_iters": 2}),
    (GENERAL, dict(max_stride=256, shard_words=256), {}, 1000, {"fused.G": 64, "fused.w_iters": 1, "lev.G": 64, "lev.w_iters": 4}),
    (LEAF, {}, {}, 9000, {"path": ref.FUSED, "fused.G": 64, "fused.w_iters": 2, "lev.G": 64, "lev.w_iters": 5}),
    # ---- 3. level kernel: level 0 on at most 2048 blocks of 256 / G k-mers, chunks of 2^24 / max_level_width k-mers, mask_alive on 2048 blocks
    (LEAF, {}, dict(levels=1), 8192, {"path": ref.LEVELS, "lev.chunk": 8192, "lev.cap": 8192, "lev.blocks0": 2048, "lev.blocks_deeper": 2048}),
    (LEAF, {}, dict(levels=1), 8191, {"lev.blocks0": 2048}),   # 8191 * 64 lanes = 2047.75 blocks
    (LEAF, {}, dict(levels=1), 8188, {"lev.blocks0": 2047}),
    (LEAF, {}, dict(levels=1), 9000, {"lev.blocks0": 2048, "lev.alive_blocks": 36}),  # 2250 blocks' worth: a second round
    (GENERAL, dict(max_level_width=40, max_stride=1), dict(levels=1), 525525,
     {"lev.G": 1, "lev.chunk": 419430, "lev.cap": 419430 * 40, "lev.blocks0": 1639, "lev.blocks0_last": 415, "lev.blocks_deeper": 2048, "lev.alive_blocks": 2048}),
    (GENERAL, dict(max_level_width=40, max_stride=1), dict(levels=1), 419430, {"lev.chunk": 419430, "lev.blocks0_last": 1639}),   # one chunk exactly
    (GENERAL, dict(max_level_width=40, max_stride=1), dict(levels=1), 419431, {"lev.chunk": 419430, "lev.blocks0_last": 1}),
    (GENERAL, dict(max_level_width=1 << 25), dict(levels=1), 10, {"lev.chunk": 1, "lev.cap": 1 << 25}),
    (GENERAL, {}, dict(levels=1), 524288, {"lev.alive_blocks": 2048, "lev.blocks0": 2048, "lev.G": 2}),
    (GENERAL, {}, dict(levels=1), 524033, {"lev.alive_blocks": 2048}),  # (rounded up to whole alive words first: 524 096 k-mers)
    (GENERAL, {}, dict(levels=1), 524032, {"lev.alive_blocks": 2047}),
    # ---- 4. children kernel: 64 lanes / lanes_per_child children per wave step; groups of steps of ~2 MB, at least 8 groups when there are 8 steps
    (REG256, {}, {}, 1531, {"path": ref.STATIONARY, "stat.lanes_per_child": 2, "stat.n_steps": 8, "stat.steps_per_group": 1, "stat.n_groups": 8,
                            "stat.groups_per_phase": 8, "stat.phases": 1, "stat.tile": 2048, "stat.n_tiles": 1, "stat.grid": 8}),
    (REG130, {}, {}, 1531, {"path": ref.STATIONARY, "stat.lanes_per_child": 4, "stat.n_steps": 9, "stat.steps_per_group": 1, "stat.n_groups": 9,
                            "stat.groups_per_phase": 8, "stat.phases": 2, "stat.n_tiles": 1, "stat.grid": 16}),
    (REG130, dict(n_children=128), {}, 1531, {"stat.n_steps": 8, "stat.phases": 1, "stat.grid": 8}),
    (REG130, dict(n_children=129), {}, 1531, {"stat.n_steps": 9, "stat.phases": 2}),
    (REG130, dict(n_children=65), {}, 1531, {"stat.n_steps": 5, "stat.steps_per_group": 1, "stat.n_groups": 5, "stat.groups_per_phase": 5, "stat.phases": 1}),  # 13 MB per step
    (REG130, dict(n_children=65, children_bytes=4 << 20), {}, 1531, {"stat.n_steps": 5, "stat.steps_per_group": 2, "stat.n_groups": 3, "stat.groups_per_phase": 3, "stat.phases": 1}),
    (REG130, dict(children_bytes=130 * 100 * 64), {}, 1531, {"stat.steps_per_group": 1, "stat.n_groups": 9}),   # small children: 9 / 8 = 1 step all the same
    (REG130, dict(n_children=17 * 16, children_bytes=17 * 16 * 100 * 64), {}, 1531, {"stat.n_steps": 17, "stat.steps_per_group": 2, "stat.n_groups": 9, "stat.phases": 2}),  # 17 / 8 = 2
    (REG130, {}, dict(steps_per_group=3), 1531, {"stat.steps_per_group": 3, "stat.n_groups": 3, "stat.groups_per_phase": 3, "stat.phases": 1}),
    (REG130, {}, dict(tile=64), 1531, {"stat.tile": 64, "stat.n_tiles": 24, "stat.grid": 2 * 24 * 8}),
    (REG130, {}, dict(tile=10), 193, {"stat.tile": 64, "stat.n_tiles": 4}),           # a tile is at least 64 k-mers
    (REG130, {}, dict(tile=64), 1 << 33, {"path": ref.FUSED, "stat.ok": 0, "stat.n_tiles": 1 << 27}),  # 2 * 2^27 * 8 = 2^31 workgroups: not one grid
    (REG130, {}, dict(unroll=1), 1531, {"stat.unroll": 1, "stat.uniform": 1}),
    (REG130, {}, dict(unroll=2), 1531, {"stat.unroll": 2}),
    (REG130, {}, dict(unroll=3), 1531, {"stat.unroll": 3}),
    (REG130, {}, dict(unroll=4), 1531, {"stat.unroll": 4}),
    (REG130, {}, dict(unroll=5), 1531, {"stat.unroll": 4}),
    (REG130, {}, dict(unroll=8), 1531, {"stat.unroll": 8}),
    (REG130, dict(children_uniform=0), dict(unroll=3), 1531, {"stat.unroll": 4, "stat.uniform": 0}),   # per-lane hashing has no U = 3
    (REG130, {}, dict(unroll=3, lane_hash=1), 1531, {"stat.unroll": 4, "stat.uniform": 0}),
    (REG130, dict(children_uniform=0), dict(unroll=8), 1531, {"stat.unroll": 8}),
    # ---- 5. root pass: at most 8192 blocks
    (REG9, {}, {}, 1 << 21, {"stat.root_blocks": 8192, "stat.n_tiles": 1024}),
    (REG9, {}, {}, (1 << 21) - 256, {"stat.root_blocks": 8191}),
    (REG9, {}, {}, (1 << 21) + 5003, {"path": ref.STATIONARY, "stat.root_blocks": 8192, "stat.n_tiles": 1027, "stat.grid": 1027}),
    # ---- 6. small kernel: at most 2048 blocks
    (GENERAL, {}, {}, 2048 * 256, {"small.blocks": 2048}),
    (GENERAL, {}, {}, 2048 * 256 - 256, {"small.blocks": 2047}),
    (GENERAL, {}, {}, 2048 * 256 + 300, {"path": ref.SMALL, "small.blocks": 2048}),
]

# A layout-order row of 200 words over 100 IBFs of at most 128 bins; v_inner_words = 10, at most 3 groups on a level
LAYOUT = dict(v_words=200, n_ibf=100, max_stride=2, has_vnodes=1, has_split=1, v_inner_words=10, n_groups=3)
HAND_LAYOUT = [
    # direct rows: the LDS holds the whole stack (100 entries = 400 bytes) and nothing else
    (LAYOUT, {}, {}, 5003, {"fused.ok": 1, "fused.stack_lds": 100, "fused.row_lds_words": 0, "fused.wave_bytes": 400, "fused.waves_per_block": 4, "fused.grid": 1251,
                            "fused.G": 1, "fused.w_iters": 1}),
    (LAYOUT, {}, dict(waves=7), 5003, {"fused.grid": 2}),
    (LAYOUT, dict(n_ibf=99), {}, 5003, {"fused.stack_lds": 100}),   # (an even number of entries)
    (LAYOUT, {}, dict(layout_direct=0), 5003, {"fused.ok": 1, "fused.stack_lds": 100, "fused.row_lds_words": 200, "fused.wave_bytes": 2000, "fused.waves_per_block": 4}),
    (LAYOUT, dict(n_ibf=500), dict(layout_direct=0), 5003, {"fused.stack_lds": 128, "fused.wave_bytes": (200 + 64) * 8}),   # 372 entries in the row of 200 words
    (LAYOUT, dict(n_ibf=500), dict(layout_direct=0, stack_lds=2), 5003, {"fused.stack_lds": 500}),                          # 498 do not fit it
    (LAYOUT, {}, dict(layout_fused=0), 5003, {"fused.ok": 0, "level.n_tiles": 3, "level.phases": 1, "level.grid": 24, "level.piece": 4 << 20}),
    (LAYOUT, dict(has_vnodes=0), {}, 5003, {"fused.ok": 0}),
    (LAYOUT, dict(n_ibf=16386), {}, 5003, {"fused.ok": 0, "fused.wave_bytes": 65544}),
    (LAYOUT, dict(n_ibf=16384), {}, 5003, {"fused.ok": 1, "fused.wave_bytes": 65536, "fused.waves_per_block": 1}),
    (LAYOUT, dict(max_stride=258), {}, 5003, {"fused.ok": 0, "fused.G": 64, "fused.w_iters": 2}),   # split bins are unified for one sweep only
    (LAYOUT, dict(max_stride=258, has_split=0), {}, 5003, {"fused.ok": 1, "fused.G": 64, "fused.w_iters": 2}),
    (LAYOUT, dict(max_stride=256), {}, 5003, {"fused.ok": 1, "fused.G": 64, "fused.w_iters": 1}),
    # level kernel: tiles of 2048 k-mers, 8 groups per phase; pieces of 96 MiB of gates, at least 4 M k-mers
    (LAYOUT, {}, {}, 2048, {"level.n_tiles": 1}),
    (LAYOUT, {}, {}, 2049, {"level.n_tiles": 2, "level.grid": 16}),
    (LAYOUT, dict(n_groups=9), {}, 5003, {"level.phases": 2, "level.grid": 48}),
    (LAYOUT, dict(v_inner_words=1), {}, 5003, {"level.piece": 12582912}),
    (LAYOUT, dict(v_inner_words=0), {}, 5003, {"level.piece": 12582912}),
    (LAYOUT, dict(n_groups=8 * 1024), {}, 1 << 31, {"level.n_tiles": 1 << 20, "level.phases": 1024, "level.grid": 0}),   # 2^33 workgroups: refused
]


def test_hand_worked_descent_plans(dump):
    cases = [(dict(sh, **change), ref.knobs(**kn), n, want) for sh, change, kn, n, want in HAND]
    out = dump([ref.descent_command(sh, kn, n) for sh, kn, n, _ in cases])
    for i, ((sh, kn, n, want), got) in enumerate(zip(cases, out)):
        named = dict(zip(ref.DESCENT_FIELDS, got))
        assert len(got) == len(ref.DESCENT_FIELDS)
        assert {k: named[k] for k in want} == want, (i, HAND[i][1:4])
        assert got == ref.descent_numbers(sh, kn, n), (i, HAND[i][1:4])


def test_hand_worked_layout_order_plans(dump):
    cases = [(dict(ls, **change), ref.knobs(**kn), n, want) for ls, change, kn, n, want in HAND_LAYOUT]
    out = dump([ref.layout_command(ls, kn, n) for ls, kn, n, _ in cases])
    for i, ((ls, kn, n, want), got) in enumerate(zip(cases, out)):
        named = dict(zip(ref.LAYOUT_FIELDS, got))
        assert len(got) == len(ref.LAYOUT_FIELDS)
        assert {k: named[k] for k in want} == want, (i, HAND_LAYOUT[i][1:4])
        assert got == ref.layout_numbers(ls, kn, n), (i, HAND_LAYOUT[i][1:4])


def test_hand_worked_plans_name_every_path_and_cap():
    """the table holds every path, and a plan at each cap of "HIBF descent: plan and grids"  with one just below it"""
    want = [w for *_, w in HAND]
    assert {w["path"] for w in want if "path" in w} == {ref.INTERLEAVED, ref.STATIONARY, ref.SMALL, ref.FUSED, ref.LEVELS}
    for field, cap in (("fused.grid", ref.FUSED_WAVES // 4), ("lev.blocks0", ref.LEVEL_BLOCKS), ("lev.alive_blocks", ref.LEVEL_BLOCKS),
                       ("stat.root_blocks", ref.ROOT_BLOCKS), ("small.blocks", ref.SMALL_BLOCKS)):
        seen = {w[field] for w in want if field in w}
        assert cap in seen and any(v < cap for v in seen), field
    assert {w["stat.phases"] for w in want if "stat.phases" in w} >= {1, 2}
    assert {w["stat.unroll"] for w in want if "stat.unroll" in w} == {1, 2, 3, 4, 8}
    assert {w["fused.G"] for w in want if "fused.G" in w} >= {1, 8, 16, 32, 64}
    assert {w["lev.w_iters"] for w in want if "lev.w_iters" in w} >= {1, 2, 4, 5}


def test_restatement_equals_header_on_the_gpu_cases(dump, oracle):
    """every (tree, shard, switches, n) of tests/test_gpu_hibf_scale.py: the tree facts from its upload descriptors"""
    import test_gpu_hibf_scale as gpu
    trees = {}

    def tree(name):
        if name not in trees:
            ub, _, descs, _ = gpu.build_tree(oracle, name)
            trees[name] = (ub, descs)
        return trees[name]
    lines, want = [], []
    for name, R, r, env, n in gpu.CASES:
        ub, descs = tree(name)
        sh = ref.shape_of(ub, descs, r, R, interleave_probe=env.get("TXQ_HIBF_INTERLEAVE_PROBE") != "0")
        kn, n = ref.knobs(env), gpu.batch_size(n, sh)
        lines.append(ref.descent_command(sh, kn, n))
        want.append(ref.descent_numbers(sh, kn, n))
    for name, env, n in gpu.LAYOUT_CASES:
        ub, descs = tree(name)
        ls = ref.layout_shape_of(ub, descs)
        assert ls is not None, name
        lines.append(ref.layout_command(ls, ref.knobs(env), n))
        want.append(ref.layout_numbers(ls, ref.knobs(env), n))
    assert len(lines) == len(gpu.CASES) + len(gpu.LAYOUT_CASES) > 70
    for line, w, got in zip(lines, want, dump(lines)):
        assert got == w, line


def test_tree_facts_of_known_trees(oracle):
    """hibf_descent_ref.shape_of on trees whose facts are plain: a regular tree and its shards, a single IBF, a small uniform tree"""
    import test_gpu_hibf_scale as gpu
    ub, _, descs, _ = gpu.build_tree(oracle, "reg33x256")
    sh = ref.shape_of(ub, descs)
    assert (sh["shard_words"], sh["n_ibf"], sh["total_tbs"], sh["max_stride"], sh["max_level_width"], sh["depth"]) == (132, 34, 33 + 33 * 256, 4, 33, 2)
    assert (sh["n_children"], sh["child_row_words"], sh["children_uniform"], sh["root_stride"], sh["probes_interleaved"]) == (33, 4, 1, 1, 0)
    assert sh["children_bytes"] == 33 * descs[1]["bin_size"] * 4 * 8
    assert ref.shape_of(ub, descs, 1, 3)["n_children"] == 11 and ref.shape_of(ub, descs, 1, 2)["n_children"] == 0  # 66 words: no child boundary
    assert ref.layout_shape_of(ub, descs) is None
    ub, _, descs, _ = gpu.build_tree(oracle, "reg33x256mixed")
    assert ref.shape_of(ub, descs)["children_uniform"] == 0
    ub, _, descs, _ = gpu.build_tree(oracle, "reg9x128")
    assert ref.shape_of(ub, descs)["probes_interleaved"] == 1 and ref.shape_of(ub, descs, interleave_probe=False)["probes_interleaved"] == 0
    ub, _, descs, _ = gpu.build_tree(oracle, "leaf16448")
    sh, ls = ref.shape_of(ub, descs), ref.layout_shape_of(ub, descs)
    assert (sh["shard_words"], sh["n_ibf"], sh["max_stride"], sh["depth"], sh["max_level_width"], sh["n_children"]) == (257, 1, 258, 1, 1, 0)
    assert (ls["v_words"], ls["v_inner_words"], ls["groups"], ls["has_split"], ls["chunk_words"]) == (258, 0, [1], 0, 2)
    ub, _, descs, _ = gpu.build_tree(oracle, "deep16")
    sh = ref.shape_of(ub, descs)
    widths = [len(l) for l in ref.levels_of(descs)]
    assert sum(widths) == len(descs) == sh["n_ibf"] and sh["max_level_width"] == max(widths) and sh["depth"] == len(widths) >= 3 and sh["max_stride"] == 1


def test_restatement_equals_header_on_random_shapes(dump):
    rng = np.random.default_rng(2024)
    pick = lambda *v: v[int(rng.integers(0, len(v)))]
    lines, want = [], []
    for _ in range(400):
        regular = rng.random() < 0.5
        crw = pick(1, 2, 4, 8, 16, 64, 128)
        n_children = int(rng.integers(1, 300)) if regular else 0
        words = n_children * crw if regular else pick(0, 1, 5, 16, 17, 94, 1040, 8187, 8190, 20000)
        sh = dict(shard_words=words, n_ibf=n_children + 1 if regular else pick(1, 2, 31, 32, 33, 127, 128, 129, 300, 5000),
                  total_tbs=pick(64, 0xFFFE, 0xFFFF, 1 << 20), max_stride=max(row for row in (pick(1, 2, 4, 6, 32, 64, 128, 256, 258, 1000), ref.row_stride(crw) if regular else 1)),
                  max_level_width=pick(1, 3, 32, 40, 1000, 1 << 24, (1 << 24) + 1), depth=pick(1, 2, 3, 4), has_nodes=int(rng.random() < 0.9), n_children=n_children,
                  child_row_words=crw if regular else 0, children_bytes=n_children * int(rng.integers(1, 1 << 22)) * 8, children_uniform=int(rng.random() < 0.5),
                  root_stride=pick(1, 2, 4, 6), probes_interleaved=int(rng.random() < 0.05))
        kn = ref.knobs(levels=int(rng.random() < 0.15), stationary=int(rng.random() < 0.85), small=int(rng.random() < 0.8), lane_hash=int(rng.random() < 0.2),
                       steps_per_group=pick(0, 0, 1, 2, 5), tile=pick(0, 0, 1, 64, 100, 256, 4096), unroll=pick(0, 1, 2, 3, 4, 5, 8), waves=pick(0, 0, 1, 3, 5, 64, 512, 100000),
                       stack_lds=pick(128, 128, 2, 3, 32, 96, 1000))
        n = pick(1, 63, 257, 1000, 9000, 16384, 16385, 32845, 524288, 524588, 2102155, int(rng.integers(1, 1 << 23)))
        lines.append(ref.descent_command(sh, kn, n))
        want.append(ref.descent_numbers(sh, kn, n))
        ls = dict(v_words=pick(2, 200, 2800, 8192, 20000), n_ibf=pick(1, 2, 99, 100, 600, 16384, 16386), max_stride=pick(1, 2, 4, 64, 256, 258, 1000), has_vnodes=int(rng.random() < 0.9),
                  has_split=int(rng.random() < 0.5), v_inner_words=pick(0, 1, 10, 500, 5000), n_groups=pick(1, 3, 8, 9, 100))
        kl = ref.knobs(layout_fused=int(rng.random() < 0.8), layout_direct=int(rng.random() < 0.5), waves=kn["waves"], stack_lds=kn["stack_lds"])
        lines.append(ref.layout_command(ls, kl, n))
        want.append(ref.layout_numbers(ls, kl, n))
    assert len({w[0] for w in want[0::2]}) == 5  # every path is drawn
    for line, w, got in zip(lines, want, dump(lines)):
        assert got == w, line
