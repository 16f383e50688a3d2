"""Measurement of `tetrex search --verify --align` (txq_edit_align_device) — not collected by pytest.  Two
workloads, each at the -e its own script uses:
  * proteins: the library, the flat index and the 10 000 query proteins of tests/perf_search_verify.py (1024 peptide bins of
    200 000 residues, k = 6; proteins of 300 residues with 3 % substitutions), `search -e 9`;
  * reads: the nucleotide workload of tests/perf_search_verify_long.py (bins of 200 000 letters in records of 4000, k = 16;
    reads of 3000 letters with 3 % substitutions), `search -e 90`.  Their 90 edits are above TXQ_EDIT_ALIGN_MAX_DISTANCE: the
    device declines every pair and the host twin aligns it, so here the two --align commands differ only in the launches.
For each: three runs of the whole command with --verify, with --verify --align, and with --verify --align under
TETREX_VERIFY_ALIGN=host (interleaved, so drift hits all alike; best and spread are reported), the rows of the two --align
commands required identical and their prefix equal to the --verify rows; then one run of the --align command under
`rocprofv3 --kernel-trace --stats` for the align kernel's own time next to the search kernels'.

    python tests/perf_search_align.py [--bins 1024] [--residues 200000] [--queries 10000] [--reads 500] [--runs 3]
                                      [--workloads proteins,reads] [--no-rocprof] [--out profiles/search_align.json]
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
import perf_search as P  # noqa: E402
import perf_search_verify_long as L  # noqa: E402

COMMANDS = (("verify", [], {}), ("align", ["--align"], {}), ("align_host", ["--align"], {"TETREX_VERIFY_ALIGN": "host"}))


def note(*what):
    print("[perf_search_align]", *what, file=sys.stderr, flush=True)


def cli(args, env=None, prefix=()):
    t = time.perf_counter()
    r = subprocess.run([*prefix, P.TETREX, *args], capture_output=True, text=True, timeout=3600, env=dict(os.environ, **(env or {})))
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-4000:])
    return time.perf_counter() - t, r.stdout, r.stderr


def kernel_stats(d, args):
    """one profiled run of the command: per kernel calls and total / average ns (rocprofv3's kernel stats)"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = os.path.join(d, "prof")
    cli(args, prefix=(rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "search", "--"))
    rows = {}
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "").replace("(anonymous namespace)::", "")
            short = re.sub(r"\(.*", "", name).replace("void ", "").split("::")[-1]
            if "edit" in short:
                rows[short] = dict(calls=int(row.get("Calls", 0)), total_ns=int(float(row.get("TotalDurationNs", 0))),
                                   average_ns=float(row.get("AverageNs", 0)), max_ns=int(float(row.get("MaxNs", 0))))
    return rows


def measure(d, path, qpath, errors, runs, rocprof):
    base = ["search", "-e", str(errors), "--verify", "-v"]
    times = {name: [] for name, _, _ in COMMANDS}
    outs, notes = {}, {}
    for _ in range(runs):
        for name, flags, env in COMMANDS:
            s, so, se = cli(base + flags + [path, qpath], dict(env, TETREX_TRACE="1"))
            times[name].append(s)
            outs[name] = so
            notes[name] = [l for l in se.splitlines() if l.startswith("Verified:") or "routes" in l]
    if outs["align"] != outs["align_host"]:
        raise SystemExit("the device route and the host twin print different rows")
    if outs["verify"].splitlines() != ["\t".join(l.split("\t")[:-2]) for l in outs["align"].splitlines()]:
        raise SystemExit("--align changes the columns in front of its own")
    res = dict(confirmed_rows=len(outs["align"].splitlines()),
               **{"%s_%s" % (name, key): val for name, ts in times.items()
                  for key, val in (("best_s", min(ts)), ("spread_s", max(ts) - min(ts)), ("runs_s", ts), ("stderr", notes[name]))})
    res["align_cost_device_s"] = res["align_best_s"] - res["verify_best_s"]
    res["align_cost_host_s"] = res["align_host_best_s"] - res["verify_best_s"]
    if rocprof:
        res["kernels_of_one_align_run"] = kernel_stats(d, base + ["--align", path, qpath])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--residues", type=int, default=200_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--reads", type=int, default=500)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--workloads", default="proteins,reads")
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_align.json"))
    a = ap.parse_args()
    res = dict(device=L.device_name(), bins=a.bins, letters_per_bin=a.residues, runs=a.runs,
               timing="wall time of the whole command, best of %d interleaved runs; kernels: one rocprofv3 --kernel-trace --stats run of its own" % a.runs)
    for name in a.workloads.split(","):
        with tempfile.TemporaryDirectory() as d:
            if name == "proteins":
                files, seqs = P.library(d, a.bins, a.residues, 1)
                qpath, _ = P.queries(d, seqs, a.queries, 300, 0.03, 2)
                P.build(d, "flat", files, ["-i"])
                errors, shape = 9, dict(queries=a.queries, query_length=300, k=6)
            else:
                letters, k, flags, record, length, errors = L.WORKLOADS["nucleotide"]
                files, seqs = L.library(d, letters, a.bins, a.residues, record, 1)
                qpath, _ = L.queries(d, letters, seqs, a.reads, record, length, 0.03, 2)
                lst = os.path.join(d, "bins.lst")
                with open(lst, "w") as f:
                    f.write("\n".join(files) + "\n")
                cli(["index", "-k", str(k), *flags, "-i", os.path.join(d, "flat"), lst])
                shape = dict(queries=a.reads, query_length=length, k=k, record_length=record)
            note(name, "library, queries and index ready")
            res[name] = dict(shape, errors=errors, substitutions=0.03, **measure(d, os.path.join(d, "flat.ibf"), qpath, errors, a.runs, not a.no_rocprof))
            note(name, "verify %.2f s, align %.2f s, align on the host %.2f s" % tuple(res[name][k + "_best_s"] for k in ("verify", "align", "align_host")))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
