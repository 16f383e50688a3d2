"""Measurement of `tetrex index --layout sized --rearrange` — not collected by pytest.  Two 1024-bin peptide libraries, k = 6:
the Swissprot-shaped one of tests/perf_sized_hibf.py (log-normal sizes, no families: nothing to gain, shows the cost) and
a library of 128 families of 8 (tests/family_fasta.py).  For each: index bytes with and without --rearrange, the build phases
(TETREX_TRACE lines of the CLI), the kernels' times from one `rocprofv3 --kernel-trace --stats` run of a rearranging build,
and the 200-motif k = 6 batch (mask stage) on both trees.  --baseline-tetrex names another build of the CLI (the parent
commit's) whose plain sized build of the same files is the yardstick for the added build time.

    python tests/perf_rearrange.py [--bins 1024] [--out profiles/sized_hibf_rearrange.json] [--baseline-tetrex PATH] [--no-rocprof]
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
TETREX = os.path.join(ROOT, "bin", "tetrex")

import perf_sized_hibf as P  # noqa: E402
from family_fasta import family_library  # noqa: E402


def build(d, name, files, flags, tetrex=TETREX, prefix=()):
    lst = os.path.join(d, "bins.lst")
    with open(lst, "w") as f:
        f.write("\n".join(files) + "\n")
    t = time.perf_counter()
    r = subprocess.run([*prefix, tetrex, "index", "-k", "6", "--layout", "sized", *flags, os.path.join(d, name), lst],
                       capture_output=True, text=True, env=dict(os.environ, TETREX_TRACE="1"), timeout=300)
    wall = time.perf_counter() - t
    if r.returncode != 0 or not os.path.exists(os.path.join(d, name + ".ibf")):
        raise RuntimeError(r.stderr[-4000:])
    stages = {}
    for m in re.finditer(r"build ms: (.*)", r.stderr):
        for key, val in re.findall(r"([a-z+]+) ([0-9.]+)", m.group(1)):
            stages[key] = float(val)
    notes = re.findall(r"sized layout: (.*)", r.stderr)
    return dict(wall_s=wall, stages_ms=stages, bytes=os.path.getsize(os.path.join(d, name + ".ibf")), layout=notes)


def kernel_stats(d, files):
    """One profiled build with --rearrange: per kernel calls and total / average ns (rocprofv3's kernel stats)."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = os.path.join(d, "prof")
    build(d, "profiled", files, ["--rearrange"],
          prefix=(rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "build", "--"))
    rows = {}
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "").replace("(anonymous namespace)::", "")
            short = re.sub(r"\(.*", "", name).split("::")[-1].split(" ")[-1]
            rows[short] = dict(calls=int(row.get("Calls", 0)), total_ns=int(float(row.get("TotalDurationNs", 0))),
                               average_ns=float(row.get("AverageNs", 0)), max_ns=int(float(row.get("MaxNs", 0))))
    return rows


def motif_batch(capi, host, path, bins, motifs):
    ix = host.IndexFile.load(path)
    _, descs = P.to_descs(ix)
    dx = capi.Index.upload_hibf(bins, descs)
    dx.query_masks(motifs, False, 6)  # warm-up
    best = None
    for _ in range(3):
        t = time.perf_counter()
        dx.query_masks(motifs, False, 6)
        dt = (time.perf_counter() - t) * 1e3
        best = dt if best is None else min(best, dt)
    dx.free()
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline-tetrex", default=None)
    ap.add_argument("--no-rocprof", action="store_true")
    a = ap.parse_args()
    res = dict(bins=a.bins, k=6, libraries={})
    with tempfile.TemporaryDirectory() as tmp:
        libs = {}
        for name in ("lognormal", "families"):
            d = os.path.join(tmp, name)
            os.makedirs(d)
            if name == "lognormal":
                files, _ = P.library(d, a.bins, 1)
            else:
                names, _, _ = family_library(d, families=a.bins // 8, members=8, seed=2, empty=())
                files = [os.path.join(d, n) for n in names]
            libs[name] = (d, files)
            r = res["libraries"][name] = {}
            build(d, "warm", files, [])  # the first build of a process pays for the files' first read
            r["sized"] = build(d, "sized", files, [])
            r["rearranged"] = build(d, "rearranged", files, ["--rearrange"])
            r["bytes_ratio_rearranged_over_sized"] = r["rearranged"]["bytes"] / r["sized"]["bytes"]
            if a.baseline_tetrex:
                build(d, "warm", files, [], tetrex=a.baseline_tetrex)
                r["baseline_sized"] = base = build(d, "baseline", files, [], tetrex=a.baseline_tetrex)
                r["baseline_bytes_equal_sized"] = open(os.path.join(d, "baseline.ibf"), "rb").read() == open(os.path.join(d, "sized.ibf"), "rb").read()
                total = sum(base["stages_ms"].values())
                r["rearrange_ms_over_baseline_build_ms"] = r["rearranged"]["stages_ms"].get("rearrange", 0.0) / total
            if not a.no_rocprof:
                r["kernels_of_a_rearranging_build"] = kernel_stats(d, files)
        from tetrex_amd import capi, host
        from motifs import random_prosite_motifs
        capi.init(0)
        motifs = random_prosite_motifs(200, 7)
        for name, (d, files) in libs.items():
            for tree in ("sized", "rearranged"):
                res["libraries"][name][tree]["motifs200_mask_ms_best_of_3"] = motif_batch(capi, host, os.path.join(d, tree + ".ibf"), a.bins, motifs)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
