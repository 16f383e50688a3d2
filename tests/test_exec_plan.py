"""The executor's host-side stage planner (csrc/txq_exec_plan.hpp) without a GPU: tests/native/exec_plan_dump.cpp, built with the
address and undefined-behaviour sanitizers, runs the sessions of golden/exec_plan_sessions.json — validate, grow, plan, chunk,
block table, as the phases of session_stage do — with made-up device addresses and prints everything a stage would upload; all
of it must be, byte for byte, what the executor planned before the planner was split from it (golden/exec_plan_expected.json:
scalars as they are, arrays as sha256 of their bytes — golden/README.md says how those were taken).  The malformed blobs and
refused stages of tests/blob_cases.py are refused here with the same code and text, and the one case that validates on several
threads runs under the thread sanitizer."""
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import blobs
import blob_cases
from blobs import DENSE_OP
from conftest import ROOT, GOLDEN

BASE_QUESTIONS = ([0, 0, 1, 1, 2, 2], [4, 0, 3, 4, 3, 2])
GXX = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
SOURCE = os.path.join(ROOT, "tests", "native", "exec_plan_dump.cpp")


def load_fixture():
    with open(os.path.join(GOLDEN, "exec_plan_sessions.json")) as f:
        fx = json.load(f)
    fx["sessions"] = {k: [(bytes.fromhex(b), qp, qs) for b, qp, qs in v] for k, v in fx["sessions"].items()}
    return fx


def run_text(stages, W=3, G_dense=8, rounds=4, hibf=0, files=None, n_programs=None):
    """one session as exec_plan_dump reads it; stages: [(blob, question programs, question slots)]; files: {stage: path} for
    blobs that are handed over in a file; n_programs: the session's (None: what its first blob says)"""
    if n_programs is None:
        n_programs = struct.unpack_from("<I", stages[0][0], blobs.FIELD["n_programs"])[0]
    out = ["%d %d %d %d %d %d" % (W, G_dense, rounds, hibf, n_programs, len(stages))]
    for i, (blob, qp, qs) in enumerate(stages):
        body = "@" + files[i] if files and i in files else blob.hex() if blob else "-"
        out.append("%d %s %d %s" % (len(blob), body, len(qp), " ".join("%d %d" % (p, s) for p, s in zip(qp, qs))))
    return "\n".join(out) + "\n"


def case_text(fx, runs):
    return "%d\n" % len(runs) + "".join(run_text(fx["sessions"][r["session"]], r["W"], r["G_dense"], r["rounds"], r["hibf"]) for r in runs)


def refusal_text(first, refused):
    """the refused stage (after `first`, where there is one) in a session of its own, then the base session on the same index"""
    stages = ([(first, [], [])] if first is not None else []) + [refused]
    return "2\n" + run_text(stages, n_programs=3) + run_text([(blob_cases._blob(blob_cases._base()),) + BASE_QUESTIONS])


def run_dump(exe, text):
    """{name: int | str (error text) | bytes}"""
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {}
    for line in r.stdout.splitlines():
        name, _, rest = line.partition(" ")
        assert name not in out, name
        if name.endswith(".error"):
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


def session_digest(dump, prefix):
    """one sha256 over everything a session printed"""
    h = hashlib.sha256()
    for k, v in sorted(digest(dump).items()):
        if k.startswith(prefix):
            h.update(("%s=%s\n" % (k[len(prefix):], v)).encode())
    return h.hexdigest()


def refusal_cases():
    """name -> (first stage or None, (blob, question programs, question slots), code); every case that needs no index"""
    cases = {"malformed: " + what: (None, (make(), [], []), -6) for what, make in blob_cases.MALFORMED.items()}
    for what, make in blob_cases.SESSION_LEVEL.items():
        if what != "auxiliary k-mers without an auxiliary index":
            cases["session: " + what] = make()
    return cases


def build(tmp, sanitizers, name):
    exe = str(tmp / name)
    subprocess.run(GXX + [sanitizers, "-fno-sanitize-recover=undefined", "-o", exe, SOURCE], check=True, timeout=600)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("exec_plan"), "-fsanitize=address,undefined", "exec_plan_dump")


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


@pytest.fixture(scope="module")
def dumps(exe, fixture):
    return {name: run_dump(exe, case_text(fixture, runs)) for name, runs in fixture["cases"].items()}


@pytest.fixture(scope="module")
def expected():
    with open(os.path.join(GOLDEN, "exec_plan_expected.json")) as f:
        return json.load(f)


def test_every_planned_list_is_what_the_executor_planned_before(dumps, expected):
    assert set(dumps) == set(expected["cases"])
    for name, dump in dumps.items():
        got = digest(dump)
        assert set(got) == set(expected["cases"][name]), name
        for key in got:
            assert got[key] == expected["cases"][name][key], (name, key)


def _rec(raw, fmt):
    size = struct.calcsize(fmt)
    assert len(raw) % size == 0
    return [struct.unpack_from(fmt, raw, i) for i in range(0, len(raw), size)]


def _u64(raw):
    return [r[0] for r in _rec(raw, "<Q")]


def _stages(d, s=0):
    t = 0
    while "s%d.t%d.rc" % (s, t) in d:
        yield "s%d.t%d." % (s, t)
        t += 1


def _dense_rows(blob):
    """[(kind, reserved)] of the blob's dense table, and per program whether an ordinary op touches a block entry"""
    from tetrex_amd import host
    d = host.blob_dense(blob)
    rows = [(int(r[0]), int(r[15])) for r in d[1]] if d else []
    on_entries = [any(int(o[0]) != DENSE_OP and (int(o[1]) | int(o[2]) | int(o[3])) & blobs.DENSE_BIT for o in ops) for _, ops in host.parse_blob(blob)[1]]
    return rows, on_entries, ([bool(x & blobs.TRACKED_BIT) for x in d[2]] if d else [])


def test_the_cases_take_the_paths_they_are_there_for(dumps, fixture):
    ses = fixture["sessions"]
    for name, d in dumps.items():
        assert all(v == 0 for k, v in d.items() if k.endswith(".rc")), name
    # blob versions 1, 2 and 4 in one session
    assert [struct.unpack_from("<I", b, 4)[0] for b, _, _ in ses["versions"]] == [1, 2, 4]
    assert len(list(_stages(dumps["versions"]))) == 3
    # small and big programs, the four kinds of untracked and of tracked dense ops, ordinary ops on entries of tracked blocks
    d = dumps["both_w1024"]
    kinds, tracked_entry_ops = set(), False
    for blob, _, _ in ses["both"]:
        rows, on_entries, tracked = _dense_rows(blob)
        kinds |= set(rows)
        tracked_entry_ops |= any(a and b for a, b in zip(on_entries, tracked))
    T, NP = blobs.TRACKED, blobs.NOPROBE
    assert {(k, 0) for k in range(4)} | {(blobs.ZERO, T), (blobs.FILL, T), (blobs.STEP, T), (blobs.STEP, T | NP), (blobs.REDUCE, T)} <= kinds
    assert tracked_entry_ops
    t0 = "s0.t0."
    assert d[t0 + "n_small"] > 0 and len(d[t0 + "units"]) > 0 and d["s0.t1.n_small"] > 0
    levels = _rec(d[t0 + "levels"], "<7Q")  # units, tiles, hsteps, sparse, sparse_chunks, sparse_misc, step_chunks
    assert any(lv[5] < lv[3] and lv[6] > 0 for lv in levels) and any(lv[5] and lv[4] > 0 for lv in levels)
    mixed = _rec(dumps["tracked_zero_beside_step"][t0 + "levels"], "<7Q")[2]  # a level's groups are ordered [others | STEPs]
    assert mixed[3:] == (2, 1, 1, 1) and _rec(dumps["tracked_zero_beside_step"][t0 + "sparse_groups"], "<2I")[3:5] == [(11, 0xFFFFFFFF), (9, 0xFFFFFFFF)]
    groups = _rec(d[t0 + "tile_groups"], "<4IQ")
    assert sum(1 for lv in levels if lv[1]) >= 3 and d[t0 + "n_tiles"] == sum(lv[1] for lv in levels)
    first = [g[4] for g in groups]
    assert first == sorted(first) and first[0] == 0 and first[-1] > levels[0][1] and len(d[t0 + "hsteps"]) == 0
    assert len(d[t0 + "sparse_groups"]) // 8 == sum(lv[3] for lv in levels) and len(d[t0 + "optr"]) // 24 == d[t0 + "n_dense"]
    # the same untracked session with its steps descending an HIBF: a level in two chunks on the 8192-pair floor
    h, u = dumps["untracked_hibf_w262144"], dumps["untracked_w3"]
    assert len(u[t0 + "hsteps"]) == 0 and len(h[t0 + "hsteps"]) > 0
    lv_h = _rec(h[t0 + "levels"], "<7Q")
    n_chunks = len(h[t0 + "chunk_first"]) // 8 - 1
    assert n_chunks > sum(1 for lv in lv_h if lv[2]) and 0 < h[t0 + "most_pairs"] <= 8192
    assert max(_rec(h[t0 + "chunk_pairs"], "<I"))[0] == h[t0 + "most_pairs"]
    # a region of 8 slots, doubled, then moved to what is needed
    g, W = dumps["region_growth"], 3
    assert _rec(g["s0.t0.fresh"], "<I") == [(0,)] and g["s0.t0.moves"] == b""
    assert _rec(g["s0.t1.fresh"], "<I") == [(1,)] and [m[2] for m in _rec(g["s0.t1.moves"], "<3Q")] == [8 * W]
    assert g["s0.t2.fresh"] == b"" and [m[2] for m in _rec(g["s0.t2.moves"], "<3Q")] == [16 * W]
    assert _u64(g["s0.t2.arenas"])[2] == (8 + 16 + 8 + 40) * W
    # blocks given back in stage 1 reach another program in stage 3, not in stage 2
    r = dumps["blocks_recycled_two_stages_later"]
    made = [_u64(r["s0.t%d.counters" % t])[1] for t in range(4)]
    assert made == [2, 4, 6, 6]
    def own(t):  # the two blocks of the program that begins in stage t, from its row [flags | block | cap | block | cap]
        row = _u64(r["s0.t%d.row_of" % t])[t]
        return {_u64(r["s0.t%d.block_table" % t])[row + i] for i in (1, 3)}
    assert own(3) == own(0) and not own(2) & own(0) and not own(1) & own(0) and len(own(0) | own(1) | own(2)) == 6
    # a second session adopts the pool: a listed block is taken as it is, a garbage block is cleared; another width starts over
    p = dumps["pool_adopted"]
    assert p["s0.begin.pool"] == 0 and len(p["s0.end.pool"]) // 24 == 5
    assert p["s1.begin.pool"] == 5 and p["s1.begin.cached_W"] == 3
    c0, c1 = _u64(p["s0.t0.counters"]), _u64(p["s1.t0.counters"])
    assert c0[1] == 5 and c0[3] == 0 and len(p["s0.t0.clears"]) // 24 == 2
    assert c1[1] == 0 and c1[3] == 1 and len(p["s1.t0.clears"]) // 24 == 1
    pooled = {b[0]: b for b in _rec(p["s0.end.pool"], "<3Q")}
    cleared = _rec(p["s1.t0.clears"], "<3Q")[0][0]
    assert pooled[cleared][1:] == (400, 0) and sorted(b[2] for b in pooled.values()) == [0, 0, 0, 1, 1]
    assert p["s2.begin.cached_blocks"] == 5 and p["s2.begin.cached_W"] == 3 and p["s2.begin.pool"] == 0
    assert _u64(p["s2.begin.arenas"])[4:7] == [1, 0, 0] and _u64(p["s2.t0.counters"])[1] == 4


def test_fixture_sessions_are_well_formed(oracle, fixture):
    """by the simulator's own assertions, on the index the GPU test runs them on"""
    ox = blob_cases.small_oracle_index(oracle)
    for name, stages in fixture["sessions"].items():
        want_alive, want = blob_cases.simulate(ox, stages)
        assert all(len(a) == len(st[1]) for a, st in zip(want_alive, stages)), name
        assert any(m.any() for m in want), name


@pytest.fixture(scope="module")
def refusals(exe):
    return {name: run_dump(exe, refusal_text(first, refused)) for name, (first, refused, _) in refusal_cases().items()}


def test_refusals_have_the_code_and_text_they_had(refusals, expected):
    assert len(refusals) == len(blob_cases.MALFORMED) + len(blob_cases.SESSION_LEVEL) - 1 == len(expected["refusals"])
    for name, (first, _, code) in refusal_cases().items():
        d, want = refusals[name], expected["refusals"][name]
        at = "s0.t%d." % (0 if first is None else 1)
        if first is not None:
            assert d["s0.t0.rc"] == 0, name
        assert d[at + "rc"] == code == want["rc"], (name, d[at + "error"])
        assert d[at + "error"] == want["error"], name
        assert at + "units" not in d, name


def test_the_base_session_plans_as_ever_after_a_refusal(refusals, dumps, expected):
    base = {k[len("s0."):]: v for k, v in digest(dumps["base"]).items()}
    for name, d in refusals.items():
        assert session_digest(d, "s1.") == expected["refusals"][name]["base_after"], name
        if name.startswith("malformed: "):  # nothing was grown: the index is as a fresh one, but for the width the refused session named
            assert d["s1.begin.cached_W"] == 3 and d["s1.begin.cached_blocks"] == 0
            assert {k[len("s1."):]: v for k, v in digest(d).items() if k.startswith("s1.") and k != "s1.begin.cached_W"} == \
                   {k: v for k, v in base.items() if k != "begin.cached_W"}, name


# ---- validation on several threads ------------------------------------------------------------------------------------------
def _huge_blob(bad=()):
    """just over 2^20 trivial ops in 300 programs of one level; bad: programs whose last op reads a slot they do not have"""
    n_prog, per = 300, 3500
    assert n_prog * per > 1 << 20
    kmers = np.arange(4, dtype=np.uint64)
    ops = np.empty((n_prog, per, 4), dtype=np.uint32)
    ops[:, :, 0] = np.arange(per, dtype=np.uint32)[None, :] % 4
    ops[:, :, 1] = 3 + np.arange(per, dtype=np.uint32)[None, :] % 5
    ops[:, :, 2] = 1
    ops[:, :, 3] = 0
    for p in bad:
        ops[p, per - 1, 2] = 8
    out = bytearray(blobs.HEADER_V2)
    k_off = len(out)
    out += kmers.tobytes()
    p_off = len(out)
    rows = np.zeros((n_prog, 6), dtype="<u4")
    rows[:, 0] = np.arange(n_prog) * per
    rows[:, 1] = per
    rows[:, 2] = 8
    rows[:, 3] = np.arange(n_prog)
    rows[:, 4] = 1
    out += rows.tobytes()
    o_off = len(out)
    out += ops.astype("<u4").tobytes()
    l_off = len(out)
    out += np.full(n_prog, per, dtype="<u4").tobytes()
    struct.pack_into("<6I5Q", out, 0, blobs.MAGIC, 2, n_prog, kmers.size, n_prog * per, n_prog, k_off, p_off, o_off, l_off, 0)
    return bytes(out)


@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_large_stages_are_validated_by_several_threads(tmp_path, exe, sanitizer):
    """from 2^20 ops on validate_blob shares the programs out to threads: the stage is accepted, and of two bad programs
    the lower one is named, as a single thread would"""
    if sanitizer == "thread":
        exe = build(tmp_path, "-fsanitize=thread", "exec_plan_dump_tsan")
    for bad, want in (((), None), ((211, 97), "program 97 op 3499: slot out of range")):
        path = str(tmp_path / "huge.blob")
        blob = _huge_blob(bad)
        with open(path, "wb") as f:
            f.write(blob)
        d = run_dump(exe, "1\n" + run_text([(blob, [], [])], files={0: path}))
        if want is None:
            assert d["s0.t0.rc"] == 0 and d["s0.t0.n_ops"] == 300 * 3500 and d["s0.t0.n_small"] == 300
        else:
            assert d["s0.t0.rc"] == -6 and d["s0.t0.error"] == want
