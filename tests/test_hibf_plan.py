"""The HIBF upload's host-side planner (csrc/txq_hibf_plan.hpp) without a GPU: tests/native/hibf_plan_dump.cpp, built with the
address and undefined-behaviour sanitizers, plans every tree of golden/hibf_plan_trees.json with made-up device addresses and
prints every array and scalar; they must be, byte for byte, what the upload code sent to the device before the planner was
split from it (golden/hibf_plan_expected.json: scalars as they are, arrays as sha256 of their bytes — golden/README.md says how
those were taken).  The plan's own invariants are asserted too, so that a later change has more than digests to go by."""
import hashlib
import json
import os
import struct
import subprocess

import pytest

from conftest import ROOT, GOLDEN

MERGED = (1 << 64) - 1
CLEARED = (1 << 64) - 2
NONE32 = 0xFFFFFFFF


def load_cases():
    with open(os.path.join(GOLDEN, "hibf_plan_trees.json")) as f:
        return json.load(f)


def case_input(case):
    """One case as the number stream hibf_plan_dump reads."""
    out = [case["mode"], case["rank"], case["n_shards"], case["user_bins"], len(case["ibfs"])]
    for f in case["ibfs"]:
        out += [f["bins"], f["bin_size"], f["hash_funs"], 0 if f["next"] is None else 1]
        if f["next"] is not None:
            out += f["next"] + f["tbu"]
    return " ".join(str(x) for x in out) + "\n"


def run_dump(exe, case):
    """{name: int | str (error text) | bytes} of one case."""
    r = subprocess.run([exe], input=case_input(case), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (case["name"], r.stderr[-3000:])
    out = {}
    for line in r.stdout.splitlines():
        name, _, rest = line.partition(" ")
        assert name not in out, name
        if name == "error":
            out[name] = rest
        elif " " in rest:
            n, _, hexed = rest.partition(" ")
            out[name] = bytes.fromhex(hexed)
            assert len(out[name]) == int(n)
        else:
            out[name] = int(rest)
    return out


def digest(dump):
    return {k: hashlib.sha256(v).hexdigest() if isinstance(v, bytes) else v for k, v in dump.items()}


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hibf_plan") / "hibf_plan_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(ROOT, "tests", "native", "hibf_plan_dump.cpp")], check=True, timeout=600)
    return {c["name"]: run_dump(exe, c) for c in load_cases()}


@pytest.fixture(scope="module")
def expected():
    with open(os.path.join(GOLDEN, "hibf_plan_expected.json")) as f:
        return json.load(f)


def test_the_fixture_has_the_cases_the_planner_is_judged_on():
    cases = {c["name"]: c for c in load_cases()}
    assert len(cases) == len(load_cases())
    for name in ("split_heavy_wide", "split_heavy_narrow", "odd_row_padding_word", "three_levels", "4_levels", "5_levels", "regular_uniform",
                 "regular_mixed", "regular_mixed_columns_0_of_2", "regular_mixed_columns_1_of_2", "almost_regular_misaligned_child",
                 "three_levels_subtrees_0_of_3", "two_subtrees_2_of_3", "invalid_child_out_of_range", "invalid_two_parents", "invalid_unreachable",
                 "invalid_user_bin_out_of_range", "invalid_self_child", "invalid_null_map"):
        assert name in cases, name


def test_every_planned_array_is_what_the_upload_sent_before(dumps, expected):
    assert set(dumps) == set(expected)
    for name, dump in dumps.items():
        got = digest(dump)
        assert set(got) == set(expected[name]), name
        for key in got:
            assert got[key] == expected[name][key], (name, key)


def test_the_cases_take_the_paths_they_are_there_for(dumps):
    d = dumps
    assert d["split_heavy_wide"]["v_chunk_words"] == 2 and d["split_heavy_narrow"]["v_chunk_words"] == 1
    for name in ("split_heavy_wide", "split_heavy_narrow"):
        ranges = _records(d[name]["vsplit_range"], "<II4IQII")
        assert d[name]["split_bins"] == 1 and max(r[1] for r in ranges) > 128            # a chunk with over 128 parts
        assert any(r[1] and r[8] == 2 for r in ranges)                                   # a chunk that starts mid-word at bit0 = 2
        assert any(r[1] and bin(r[2] | r[3] << 32 | r[4] << 64 | r[5] << 96).count("1") == 2 for r in ranges)  # two split bins share a chunk
    odd = d["odd_row_padding_word"]
    assert odd["v_chunk_words"] == 1 and odd["v_words"] == 4 and odd["n_vchunks"] == 4   # three one-word IBFs and the padding word
    assert d["three_levels"]["depth"] == 3 and d["three_levels"]["layout_order"] == 1
    assert len(d["three_levels"]["vgroups"]) // 4 > 2 * 3                                 # a level cut into several groups
    assert d["4_levels"]["depth"] == 4 and d["4_levels"]["layout_order"] == 1
    assert d["5_levels"]["depth"] == 5 and d["5_levels"]["layout_order"] == 0 and d["5_levels"]["regular"] == 0
    assert d["two_subtrees_2_of_3"]["n_ibf"] == 1                                         # the root alone, every bin cleared
    assert set(struct.unpack("<%dQ" % (len(d["two_subtrees_2_of_3"]["tb_user"]) // 8), d["two_subtrees_2_of_3"]["tb_user"])) == {CLEARED}
    assert sum(d["three_levels_subtrees_%d_of_3" % r]["n_ibf"] - 1 for r in range(3)) == d["three_levels"]["n_ibf"] - 1
    assert d["regular_uniform"]["regular"] == 1 and d["regular_uniform"]["interleave"] == 1 and d["regular_uniform"]["children_uniform"] == 1
    assert d["regular_mixed"]["regular"] == 1 and d["regular_mixed"]["children_uniform"] == 0 and d["regular_mixed"]["interleave"] == 0
    for r in range(2):
        assert d["regular_mixed_columns_%d_of_2" % r]["regular"] == 1 and d["regular_mixed_columns_%d_of_2" % r]["shard_words"] == 12
        assert d["regular_uniform_subtrees_entry_%d_of_2" % r]["regular"] == 1 and d["regular_uniform_subtrees_entry_%d_of_2" % r]["shard_words"] == 4
    assert d["almost_regular_misaligned_child"]["regular"] == 0 and d["almost_regular_misaligned_child"]["layout_order"] == 1
    for name, dump in d.items():
        assert (dump["rc"] != 0) == name.startswith("invalid_") or name in ("invalid_user_bin_out_of_range_subtrees_entry",), name
    # with several faults the first one met in breadth-first order is reported, as ever
    assert d["invalid_several_faults"]["error"] == "IBF 0 bin 1: bad child 7"
    assert d["invalid_several_faults_subtrees_entry"]["error"] == "HIBF: bad child 7 (out of range or reached twice)"


def _records(raw, fmt):
    size = struct.calcsize(fmt)
    assert len(raw) % size == 0
    return [struct.unpack_from(fmt, raw, i) for i in range(0, len(raw), size)]


def _u(raw, width):
    return list(struct.unpack("<%d%s" % (len(raw) // width, "Q" if width == 8 else "I"), raw))


def test_layout_plans_keep_their_invariants(dumps):
    cases = {c["name"]: c for c in load_cases()}
    checked = 0
    for name, d in dumps.items():
        if not d.get("layout_order"):
            continue
        checked += 1
        n, cw, words = d["n_ibf"], d["v_chunk_words"], d["v_words"]
        tbu, off, nxt = _u(d["tb_user"], 8), _u(d["map_off"], 8), _u(d["next"], 8)
        ibfs = _records(d["ibf"], "<QQ8I")  # words, bin_size, hash_shift, hash_funs, stride, shard_words, word0, bins, ident_word, reserved
        bins = [f[7] for f in ibfs]
        off.append(off[-1] + bins[-1])
        seg, chunk0 = _u(d["seg"], 8), _u(d["chunk0"], 4)
        chunks = _records(d["vchunks"], "<QII4I")  # words, bin_size, packed, col, gate_word, gate_bit, ibf
        padded = [((b + 63) // 64 + cw - 1) // cw * cw for b in bins]
        # segments are disjoint and tile the row up to the padding word
        spans = sorted((seg[i], seg[i] + padded[i]) for i in range(n))
        assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), name
        assert words - spans[-1][1] in (0, 1) and words % 2 == 0, name
        assert len(chunks) == words // cw if cw == 2 else len(chunks) == words, name
        # a chunk writes its own words of the row: chunk c is row words [c * cw, (c + 1) * cw)
        for i in range(n):
            for j in range(padded[i] // cw):
                c = chunks[chunk0[i] + j]
                assert chunk0[i] + j == seg[i] // cw + j and c[6] == i and c[3] == j * cw and c[0] == ibfs[i][0], (name, i, j)
        # every gate is seg[parent] + bit
        parent = {}
        for i in range(n):
            for b in range(bins[i]):
                if tbu[off[i] + b] == MERGED:
                    parent[nxt[off[i] + b]] = (i, b)
        paths = _records(d["vpaths"], "<II" + "QIIII" * 3)
        for i in range(n):
            for j in range(padded[i] // cw):
                c = chunks[chunk0[i] + j]
                if i not in parent:
                    assert i == 0 and c[4] == NONE32, (name, i)
                else:
                    p, b = parent[i]
                    assert c[4] * 64 + c[5] == seg[p] * 64 + b, (name, i)
            chain, a = [], i
            while a in parent:
                chain.append(parent[a])
                a = parent[a][0]
            chain.reverse()
            assert paths[i][0] == len(chain) <= 3, (name, i)
            for k, (p, b) in enumerate(chain):
                words_p, rows_p, _, word, bit = paths[i][2 + 5 * k: 7 + 5 * k]
                assert (words_p, rows_p, word * 64 + bit) == (ibfs[p][0], ibfs[p][1], b), (name, i, k)
        # leaf and vuser: exactly the technical bins that are user bins (split bins: one of their parts), each with its user bin
        leaf, vuser = _u(d["vleaf"], 8), _u(d["vuser"], 4)
        nonrep = _u(d["vnonrep"], 8) if d["split_bins"] else [0] * words
        rep = _u(d["vrep"], 4) if d["split_bins"] else []
        assert all(l & m == 0 for l, m in zip(leaf, nonrep)), name  # leaf and nonrep are disjoint
        for i in range(n):
            users = {}
            for b in range(bins[i]):
                ub, pos = tbu[off[i] + b], seg[i] * 64 + b
                is_leaf, is_nonrep = leaf[pos >> 6] >> (pos & 63) & 1, nonrep[pos >> 6] >> (pos & 63) & 1
                if ub in (MERGED, CLEARED):
                    assert not is_leaf and not is_nonrep and vuser[pos] == NONE32, (name, i, b)
                    continue
                assert vuser[pos] == ub and is_leaf + is_nonrep == 1, (name, i, b)
                users.setdefault(ub, []).append((pos, is_leaf))
                if is_nonrep:  # every rep_pos target is a leaf bit of the same IBF, and of the same user bin
                    to = rep[pos]
                    assert seg[i] * 64 <= to < seg[i] * 64 + bins[i] and leaf[to >> 6] >> (to & 63) & 1 and vuser[to] == ub, (name, i, b)
            for ub, parts in users.items():  # one representative per user bin and IBF: its lowest technical bin
                assert [l for _, l in parts] == [1] + [0] * (len(parts) - 1), (name, i, ub)
        if d["split_bins"]:
            ranges = _records(d["vsplit_range"], "<II4IQII")  # first, count, reps[4], side, side_stride, bit0
            splits = _records(d["vsplits"], "<IHH")           # part_word, rep_bit, part_bit
            side_pos, side_off, side_stride = _u(d["side_pos"], 4), _u(d["side_off"], 8), _u(d["side_stride"], 4)
            assert len(side_pos) == len(splits) and len(ranges) == len(chunks), name
            for i in range(n):
                seen = set()
                for j in range(padded[i] // cw):
                    c = chunk0[i] + j
                    first, count, r0, r1, r2, r3, side, stride, bit0 = ranges[c]
                    assert bool(count) == bool(chunks[c][2] >> 30 & 1) and stride == side_stride[i], (name, c)
                    if not count:
                        continue
                    # a chunk's entries are consecutive from bit0 of its side word
                    base = (side - side_off[i]) * 64 + bit0
                    assert side_pos[first:first + count] == list(range(base, base + count)) and bit0 < 64, (name, c)
                    assert base + count <= stride * 64 and side_off[i] + stride * ibfs[i][1] == side_off[i + 1], (name, c)
                    reps = r0 | r1 << 32 | r2 << 64 | r3 << 96
                    for e in range(first, first + count):
                        part_word, rep_bit, part_bit = splits[e]
                        part = seg[i] * 64 + part_word * 64 + part_bit
                        assert reps >> rep_bit & 1 and rep[part] == (seg[i] + j * cw) * 64 + rep_bit, (name, c, e)
                        assert side_pos[e] not in seen, (name, c, e)  # the side bits of one IBF are distinct
                        seen.add(side_pos[e])
                assert len(seen) == sum(bin(w).count("1") for w in nonrep[seg[i]:seg[i] + padded[i]]), (name, i)
        assert name in cases
    assert checked >= 8


def test_sub_tree_shards_deal_every_sub_tree_to_exactly_one_shard(dumps):
    """Largest sub-tree first, ties to the lower shard: the three ranks' kept IBFs partition the tree below the root, and a rank's
    root keeps exactly the technical bins that lead into its sub-trees (rank 0: the root's own user bins too)."""
    cases = {c["name"]: c for c in load_cases()}
    for stem in ("three_levels_subtrees_%d_of_3", "two_subtrees_%d_of_3"):
        tree = cases[stem % 0]["ibfs"]
        kept = [_u(dumps[stem % r]["shard.kept"], 8) for r in range(3)]
        assert all(k[0] == 0 for k in kept)
        below = sorted(i for k in kept for i in k[1:])
        assert below == list(range(1, len(tree)))
        weight = {}
        for r in range(3):
            mask = _u(dumps[stem % r]["shard.keep_mask"], 8)
            mine = [b for b in range(tree[0]["bins"]) if mask[b >> 6] >> (b & 63) & 1]
            assert {tree[0]["next"][b] for b in mine if tree[0]["tbu"][b] == MERGED} <= set(kept[r])
            assert all(r == 0 for b in mine if tree[0]["tbu"][b] != MERGED)
            weight[r] = sum((tree[i]["bins"] + 63) // 64 for i in kept[r][1:])
        assert weight[0] >= weight[1] >= weight[2]
