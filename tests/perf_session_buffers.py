"""Host overhead of libtxq's sessions and buffers, this build's libtxq.so against a build of another commit, for changes to
who owns device memory that must not cost time — not collected by pytest.  Timed per build, the builds alternating round by
round so that drift hits both alike, each round in a process of its own (a process loads one libtxq.so):

  sessions      200 single-program sessions (begin, one stage, end) on a small flat index
  cycle         the cycle of tests/test_gpu_torch_interop.py test_no_device_memory_is_left_behind, 20 times
  cycle_owners  the cycle of its sibling (other_owners_cycle), 20 times
  bench         bench.py's end-to-end leg: the single-motif latency and the 1000-motif batch as it prints them

The bar: every median of this build lies within the other build's own spread over its rounds, that is at or below its slowest
round (a median below the other build's fastest round is no regression either; both bounds are written out).

    python tests/perf_session_buffers.py --parent DIR [--rounds 7] [--out profiles/libtxq_buffers.json]

DIR holds the other build's libraries as DIR/tetrex_amd/libtxq.so, libtetrex_query.so and libtetrex_host.so (the query library
finds libtxq.so beside itself, so each build's query library comes with it)."""
import argparse
import json
import os
import runpy
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

# (--full: a plain run times the probe steps alone; the legs this leaves on run too, the figures are the end-to-end leg's)
BENCH_ARGS = ["--gpus", "1", "--steps", "5", "--warmup", "2", "--full", "--no-cpu", "--no-dna-batch"]


def note(*what):
    print("[perf_session_buffers]", *what, file=sys.stderr, flush=True)


def use_library(directory):
    """tetrex_amd.capi on the libraries of `directory` (set before its first call loads them)"""
    from tetrex_amd import capi
    capi._HERE = directory
    capi.LIB_PATH = os.path.join(directory, "libtxq.so")
    return capi


def worker_host(path):
    """sessions, cycle and cycle_owners in this process, on the libraries in `path`: one JSON line of seconds"""
    capi = use_library(path)
    import oracle as O
    from helpers import NO_KMER, make_blob, random_hibf, random_words, splitmix64
    from test_gpu_torch_interop import other_owners_cycle
    capi.init(0)
    out = {}
    words = random_words(300, 4099, 0.3, 1)
    kmers = splitmix64(5, 5000) >> np.uint64(44)
    blob = make_blob(kmers[:8], [(4, [(0, 3, 1, 0), (1, 3, 3, 0), (7, 3, 3, 0), (NO_KMER, 2, 3, 2)])])
    ix = capi.Index.upload_ibf(300, 4099, 3, words)

    def sessions(n):
        for _ in range(n):
            s = ix.session(1)
            s.stage(blob)
            s.end()
    sessions(20)
    t = time.perf_counter()
    sessions(200)
    out["sessions"] = time.perf_counter() - t
    ix.free()
    _, descs, _ = random_hibf(O, 2, user_bins=120, levels=3)

    def cycle():
        ix = capi.Index.upload_ibf(300, 4099, 3, words)
        ix.probe(kmers)
        ix.query_masks(["LMAEG", "A.CD[EK]"], False, 4)
        ix.free()
        hx = capi.Index.upload_hibf(120, descs)
        hx.probe(kmers)
        hx.query_masks(["LMAEG"], False, 4)
        hx.free()
        hb = capi.HostBuffer((1000, 5))
        hb.free()
        db = capi.DeviceBuffer(1 << 20)
        db.free()

    def delenv(name):
        del os.environ[name]
    for name, fn in (("cycle", cycle), ("cycle_owners", other_owners_cycle(os.environ.__setitem__, delenv))):
        for _ in range(3):
            fn()
        capi.synchronize()
        t = time.perf_counter()
        for _ in range(20):
            fn()
        capi.synchronize()
        out[name] = time.perf_counter() - t
    print(json.dumps(out))


def worker_bench(path):
    use_library(path)
    sys.argv = [os.path.join(ROOT, "bench.py")] + BENCH_ARGS
    runpy.run_path(sys.argv[0], run_name="__main__")


def run_worker(kind, path):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", kind, "--library", path], capture_output=True, text=True, timeout=1800)
    if r.returncode != 0:
        raise RuntimeError(r.stdout[-2000:] + r.stderr[-4000:])
    line = [x for x in r.stdout.splitlines() if x.startswith("{")][-1]
    d = json.loads(line)
    if kind == "host":
        return d
    e = d["end_to_end"]
    return {"bench_single_query_ms": e["single_query"]["median_latency_ms"], "bench_batch_1000_s": e["batch"]["seconds"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a build of the commit to compare with (its libraries in DIR/tetrex_amd/)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "libtxq_buffers.json"))
    ap.add_argument("--worker", choices=["host", "bench"])
    ap.add_argument("--library", help="(with --worker) the directory of the build's libraries")
    a = ap.parse_args()
    if a.worker:
        return (worker_host if a.worker == "host" else worker_bench)(a.library)
    if not a.parent:
        ap.error("--parent is required")
    builds = (("parent", os.path.join(os.path.abspath(a.parent), "tetrex_amd")), ("new", os.path.join(ROOT, "tetrex_amd")))
    raw = {tag: {} for tag, _ in builds}
    for r in range(a.rounds):
        for tag, path in builds:
            got = dict(run_worker("host", path), **run_worker("bench", path))
            for k, v in got.items():
                raw[tag].setdefault(k, []).append(v)
            note("round %d %s: %s" % (r, tag, " ".join("%s %.4g" % kv for kv in sorted(got.items()))))
    res = dict(timing="seconds (bench_single_query_ms: milliseconds); %d rounds per build, parent and new alternating, every round in fresh processes; "
                      "sessions: 200 sessions, cycle / cycle_owners: 20 cycles, bench: python bench.py %s" % (a.rounds, " ".join(BENCH_ARGS)),
               bar="the new build's median lies at or below the parent build's slowest round", legs={})
    for k in sorted(raw["new"]):
        p, n = sorted(raw["parent"][k]), sorted(raw["new"][k])
        res["legs"][k] = dict(parent=raw["parent"][k], new=raw["new"][k], parent_median=float(np.median(p)), parent_min=p[0], parent_max=p[-1],
                              new_median=float(np.median(n)), new_median_within_parent_min_max=bool(p[0] <= np.median(n) <= p[-1]),
                              new_median_not_above_parent_max=bool(np.median(n) <= p[-1]))
        note("%s: parent median %.4g [%.4g .. %.4g], new median %.4g" % (k, np.median(p), p[0], p[-1], np.median(n)))
    res["all_not_above_parent_max"] = all(e["new_median_not_above_parent_max"] for e in res["legs"].values())
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
