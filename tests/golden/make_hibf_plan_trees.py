#!/usr/bin/env python3
"""Writes hibf_plan_trees.json: the tree SHAPES (no IBF words) that tests/test_hibf_plan.py plans on the CPU and
tests/test_gpu_hibf_plan.py uploads — per case the entry point (mode 0 txq_index_upload, 1 txq_index_upload_subtrees), rank and
shard count, the user bins, and per IBF bins, bin_size, hash_funs, next, tbu (null: the IBF's maps are null pointers).

  python tests/golden/make_hibf_plan_trees.py

hibf_plan_expected.json (what the plans of these trees must be) is NOT made here: its digests were taken from the upload code as
it was before the planner existed (tests/golden/README.md)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from helpers import MERGED, split_heavy_hibf  # noqa: E402


class _NoOracle:
    """split_heavy_hibf fills an oracle index as it goes; only the tree's shape is wanted here."""
    class Index:
        @staticmethod
        def hibf(*a, **k):
            return _NoOracle.Index()

        def add_ibf(self, *a):
            self.n = getattr(self, "n", -1) + 1
            return self.n

        def hibf_emplace(self, *a):
            pass

        def hibf_words(self, i):
            return None


def ibf(bins, bin_size, hash_funs, next_, tbu):
    return dict(bins=bins, bin_size=bin_size, hash_funs=hash_funs, next=[int(x) for x in next_] if next_ is not None else None,
                tbu=[int(x) for x in tbu] if tbu is not None else None)


def case(name, user_bins, ibfs, mode=0, rank=0, n_shards=1):
    return dict(name=name, mode=mode, rank=rank, n_shards=n_shards, user_bins=user_bins, ibfs=ibfs)


def from_descs(descs, bin_size=None):
    return [ibf(d["bins"], bin_size or d["bin_size"], d["hash_funs"], d["next_ibf_id"], d["tb_to_user"]) for d in descs]


def general_tree(rng, shape, bin_size, hash_funs=2):
    """shape: per IBF (technical bins, [children]); IBF 0 is the root.  Children sit behind randomly placed merged bins, every
    other technical bin is a user bin; the user-bin ids are a random permutation."""
    slots = []
    for bins, children in shape:
        at = rng.choice(bins, size=len(children), replace=False)
        s = [None] * bins
        for c, b in zip(children, at):
            s[int(b)] = c
        slots.append(s)
    n_user = sum(1 for s in slots for x in s if x is None)
    ids = iter(rng.permutation(n_user))
    out = []
    for i, ((bins, _), s) in enumerate(zip(shape, slots)):
        bs = bin_size[i] if isinstance(bin_size, list) else bin_size
        out.append(ibf(bins, bs, hash_funs if i % 3 else hash_funs + 1, [x or 0 for x in s], [MERGED if x is not None else next(ids) for x in s]))
    return n_user, out


def regular_tree(children, bins, bin_sizes, hash_funs=2, root_rows=64):
    """A root of merged bins only over `children` leaves that each map an aligned run of `bins` user bins; the root's bins lead to
    the children in reverse order, so that a child's root bin is not its column."""
    ibfs = [ibf(children, root_rows, hash_funs, [children - c for c in range(children)], [MERGED] * children)]
    for c in range(children):
        ibfs.append(ibf(bins, bin_sizes[c % len(bin_sizes)], hash_funs, [0] * bins, range(c * bins, (c + 1) * bins)))
    return children * bins, ibfs


def main():
    rng = np.random.default_rng(2026)
    cases = []
    # 1. many parts per chunk, two split bins in a chunk, a chunk that starts mid-word: 16-byte and 8-byte chunks
    for narrow in (False, True):
        _, descs, _, _ = split_heavy_hibf(_NoOracle, 3, narrow=narrow, rows=96)
        user_bins = 1 + max(int(u) for d in descs for u in d["tb_to_user"] if int(u) != MERGED)
        cases.append(case("split_heavy_narrow" if narrow else "split_heavy_wide", user_bins, from_descs(descs)))
    # 2. three one-word IBFs: 8-byte chunks, a row of three words and the padding word
    n_user, ibfs = general_tree(rng, [(50, [1, 2]), (64, []), (33, [])], 80)
    cases.append(case("odd_row_padding_word", n_user, ibfs))
    # 3. three levels, user bins beside merged bins, shuffled ids, IBFs of several widths; big enough rows that a level is cut into groups
    shape3 = [(130, [1, 2, 3]), (200, [4, 5]), (64, []), (300, [6]), (70, []), (128, []), (257, [])]
    n_user3, tree3 = general_tree(rng, shape3, [300, 70000, 200, 70000, 64, 64, 100])
    cases.append(case("three_levels", n_user3, tree3))
    # 4. the deepest tree sessions follow in layout order (four levels), and one level more
    for levels in (4, 5):
        shape = [(70 + 10 * i, [i + 1] if i + 1 < levels else []) for i in range(levels)]
        n_user, ibfs = general_tree(rng, shape, 128)
        cases.append(case("%d_levels" % levels, n_user, ibfs))
    # 5. sub-tree shards: three sub-trees over three shards, and two sub-trees over three shards (the last shard keeps the root alone, all bins cleared)
    for r in range(3):
        cases.append(case("three_levels_subtrees_%d_of_3" % r, n_user3, tree3, mode=1, rank=r, n_shards=3))
    n_user, ibfs = general_tree(rng, [(40, [1, 2]), (100, [3]), (64, []), (65, [])], 100)
    for r in range(3):
        cases.append(case("two_subtrees_%d_of_3" % r, n_user, ibfs, mode=1, rank=r, n_shards=3))
    # 6. regular two-level trees
    ub, uniform = regular_tree(4, 128, [512])
    cases.append(case("regular_uniform", ub, uniform))
    ub2, mixed = regular_tree(6, 256, [512, 300, 1000])
    cases.append(case("regular_mixed", ub2, mixed))
    for r in range(2):
        cases.append(case("regular_mixed_columns_%d_of_2" % r, ub2, mixed, rank=r, n_shards=2))
        cases.append(case("regular_uniform_subtrees_entry_%d_of_2" % r, ub, uniform, mode=1, rank=r, n_shards=2))
    almost = json.loads(json.dumps(uniform))
    almost[2]["tbu"] = list(range(192, 320))
    almost[3]["tbu"] = list(range(320, 448))
    almost[4]["tbu"] = list(range(128, 192)) + list(range(448, 512))
    cases.append(case("almost_regular_misaligned_child", ub, almost))
    cases.append(case("almost_regular_subtrees_1_of_2", ub, almost, mode=1, rank=1, n_shards=2))
    # 7. invalid trees (those of tests/test_gpu_errors.py, a self-child that is not the root's, null maps)
    def two(nxt, tbu, child=([0] * 4, [3, 4, 5, 6])):
        return [ibf(4, 16, 2, nxt, tbu), ibf(4, 16, 2, *child)]
    bad = {"child_out_of_range": two([5, 0, 0, 0], [MERGED, 0, 1, 2]),
           "root_its_own_child": two([0, 0, 0, 0], [MERGED, 0, 1, 2]),
           "two_parents": two([1, 1, 0, 0], [MERGED, MERGED, 1, 2]),
           "unreachable": two([0, 0, 0, 0], [0, 1, 2, 3]),
           "user_bin_out_of_range": two([1, 0, 0, 0], [MERGED, 0, 1, 99]),
           "self_child": two([1, 0, 0, 0], [MERGED, 0, 1, 2], child=([0, 1, 0, 0], [3, MERGED, 5, 6])),
           "null_map": two([1, 0, 0, 0], [MERGED, 0, 1, 2], child=(None, None)),
           "several_faults": two([1, 7, 0, 0], [MERGED, MERGED, 1, 99])}
    for name, tree in bad.items():
        cases.append(case("invalid_" + name, 7, tree))
        cases.append(case("invalid_%s_subtrees_entry" % name, 7, tree, mode=1, rank=1, n_shards=2))
    with open(os.path.join(HERE, "hibf_plan_trees.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases) + "\n]\n")
    print("%d cases" % len(cases))


if __name__ == "__main__":
    main()
