"""Measurement of the sliding window count on an HIBF (txq_count_windows with TXQ_COUNT_WINDOWS_TREE) — not
collected by pytest.  One MI355X.

  (a) kernels: txq_count_windows_device on the sized HIBF of tests/perf_sized_hibf.py (Swissprot-shaped, 1024 bins, k = 6) and
      on the uniform tree of the same library, over `--windows` windows that slide by `--step` values, of step x 2, 4, 8 and
      16 values each.  The value array alternates runs of a library record's own k-mers with runs of random values of the
      same length, so half of the values are bins' own and the windows over them descend.  Variants: the knob at 0 (the
      windows as independent queries: the parent commit's route) and sliding in units of 16, 8 and 32 windows.  All variants
      run in one process in interleaved rounds with device events around each call; the figure of a variant is its best of
      `--reps` rounds, and the independent route's spread is the range of its own rounds.  Every variant's hits are compared
      with the independent route's.  gather_ratio is txq_count_windows_trace's (added + subtracted) over the independent
      route's added.  With `--parent DIR` (a tree of the parent commit with its build) the independent leg is timed on that
      build too, by this script run from a child process with --root DIR on the same index files and windows.
  (b) the command: `--records` chimeric records of `--letters` letters (a third from one bin, a third random, a third from
      another) against the sized index with `--window 120 --step 30 -e 4`, plain and with --verify-windows: this build at its
      default, this build with TXQ_COUNT_WINDOWS_TREE=0 and the parent's build, best wall time of `--reps` interleaved runs.

    python tests/perf_count_windows_tree.py [--windows 200000] [--step 16] [--reps 5] [--parent DIR] [--resource-usage FILE]
                                            [--out profiles/count_windows_tree.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
VARIANTS = {"independent": {"TXQ_COUNT_WINDOWS_TREE": "0"}, "U16": {"TXQ_COUNT_WINDOWS_TREE": "1", "TXQ_COUNT_WINDOWS_UNIT": "16"},
            "U8": {"TXQ_COUNT_WINDOWS_TREE": "1", "TXQ_COUNT_WINDOWS_UNIT": "8"}, "U32": {"TXQ_COUNT_WINDOWS_TREE": "1", "TXQ_COUNT_WINDOWS_UNIT": "32"}}
KNOBS = ("TXQ_COUNT_WINDOWS_TREE", "TXQ_COUNT_WINDOWS_UNIT")


def set_env(env):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)


def records_of(path):
    return [line.strip() for line in open(path) if not line.startswith(">")]


def value_stream(host, files, n_values, seed):
    """runs of a record's own k-mer values alternating with runs of random values of the same length"""
    rng = np.random.default_rng(seed)
    parts, total = [], 0
    while total < n_values:
        recs = records_of(files[int(rng.integers(0, len(files)))])
        own = host.record_values_array(recs[int(rng.integers(0, len(recs)))], 6, False, 0, False)
        if own.size == 0:
            continue
        parts += [own, rng.integers(0, 1 << 30, size=own.size, dtype=np.uint64)]
        total += 2 * own.size
    return np.concatenate(parts)[:n_values]


def kernels(a, res, d, files, only_independent):
    import torch
    from perf_sized_hibf import to_descs
    from tetrex_amd import capi, host
    stream = torch.cuda.current_stream().cuda_stream
    n, S = a.windows, a.step
    dev = lambda x: torch.from_numpy(x).cuda()
    variants = {"independent": VARIANTS["independent"]} if only_independent else VARIANTS
    out = res["kernels"] = dict(windows=n, step_values=S, timing="device events around each call, best of %d interleaved rounds in one process" % a.reps, trees={})
    for name in ("sized", "uniform"):
        f = host.IndexFile.load(os.path.join(d, name + ".ibf"))
        desc, descs = to_descs(f)
        ix = capi.Index.upload_hibf(a.bins, descs)
        W = ix.shard_words
        tree = out["trees"][name] = dict(ibfs=len(descs), widest_ibf=max(x["bins"] for x in descs), by_ratio={})
        for ratio in (2, 4, 8, 16):
            w = S * ratio
            values = value_stream(host, files, n * S + w, 7 + ratio)
            begins = np.arange(n, dtype=np.uint64) * np.uint64(S)
            lens = np.full(n, w, dtype=np.uint32)
            thr = np.full(n, max(1, w // 2), dtype=np.uint32)
            d_val, d_beg, d_len, d_thr = dev(values.view(np.int64)), dev(begins.view(np.int64)), dev(lens.view(np.int32)), dev(thr.view(np.int32))
            hit = {v: torch.zeros(n * W, dtype=torch.int64, device="cuda") for v in variants}

            def run(v):
                set_env(variants[v])
                ix.count_windows_device(d_val.data_ptr(), d_beg.data_ptr(), d_len.data_ptr(), n, d_thr.data_ptr(), hit[v].data_ptr(), None, stream)
            r = tree["by_ratio"][str(ratio)] = dict(window_values=w, variants={})
            for v in variants:  # warm-up; the routes must agree; what each did
                run(v)
                torch.cuda.synchronize()
                if not torch.equal(hit[v], hit["independent"]):
                    raise RuntimeError("%s: hits differ from the independent route's on the %s tree at w = %d" % (v, name, w))
                r["variants"][v] = dict(times_ms=[])
                if hasattr(ix, "count_windows_trace"):
                    r["variants"][v]["trace"] = dict(zip(("visits", "added", "subtracted", "items"), ix.count_windows_trace()))
            r["hit_fraction"] = float((hit["independent"] != 0).float().mean())
            for _ in range(a.reps):
                for v in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run(v)
                    e1.record()
                    torch.cuda.synchronize()
                    r["variants"][v]["times_ms"].append(e0.elapsed_time(e1))
            base = r["variants"]["independent"]
            for v, e in r["variants"].items():
                e["ms"] = min(e["times_ms"])
                e["time_ratio"] = e["ms"] / min(base["times_ms"])
                if "trace" in e and base["trace"]["added"]:
                    e["gather_ratio"] = (e["trace"]["added"] + e["trace"]["subtracted"]) / base["trace"]["added"]
            r["independent_spread_ms"] = max(base["times_ms"]) - min(base["times_ms"])
            print("%s w = %d: %s" % (name, w, ", ".join("%s %.3f ms" % (v, e["ms"]) for v, e in r["variants"].items())), file=sys.stderr, flush=True)
            del hit
            torch.cuda.empty_cache()
        ix.free()
    set_env({})


def chimeras(a, d, files):
    rng = np.random.default_rng(5)
    third = a.letters // 3
    recs = []
    for q in range(a.records):
        x, y = (int(v) for v in rng.choice(len(files), size=2, replace=False))
        part = lambda b: ("".join(records_of(files[b])) * (third // 30 + 1))[:third]
        mid = AA[rng.integers(0, 20, size=a.letters - 2 * third)].tobytes().decode()
        recs.append(">c%d_b%d_b%d\n%s\n" % (q, x, y, part(x) + mid + part(y)))
    path = os.path.join(d, "chimeras.fa")
    with open(path, "w") as f:
        f.write("".join(recs))
    return path


def command(a, res, d, files, root):
    tetrex = os.path.join(root, "bin", "tetrex")
    qpath = chimeras(a, d, files)
    index = os.path.join(d, "sized.ibf")
    out = res["command"] = dict(index="sized", records=a.records, letters=a.letters, window=120, step=30, errors=4,
                                timing="wall time of the process, best of %d interleaved runs after one warm-up run each" % a.reps, commands={})
    for cname, extra in (("window", []), ("verify_windows", ["--verify-windows"])):
        args = ["search", "--window", "120", "--step", "30", "-e", "4", *extra, index, qpath]
        legs = {"default": ([tetrex, *args], {}), "independent": ([tetrex, *args], {"TXQ_COUNT_WINDOWS_TREE": "0"})}
        if a.parent:
            legs["parent_build"] = ([os.path.join(a.parent, "bin", "tetrex"), *args], {})
        base_env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        c = out["commands"][cname] = {}
        outputs = {}
        for rep in range(a.reps + 1):
            for name, (cmd, env) in legs.items():
                t = time.perf_counter()
                cp = subprocess.run(cmd, capture_output=True, text=True, timeout=1800, env=dict(base_env, **env))
                wall = time.perf_counter() - t
                if cp.returncode != 0:
                    raise RuntimeError(cp.stderr)
                outputs[name] = cp.stdout
                if rep == 0:
                    c[name] = dict(rows=len(cp.stdout.splitlines()), walls_s=[])
                else:
                    c[name]["walls_s"].append(wall)
        for name in legs:
            c[name]["wall_s"] = min(c[name]["walls_s"])
            print("%s %s: %.3f s" % (cname, name, c[name]["wall_s"]), file=sys.stderr, flush=True)
            c[name]["same_bytes_as_default"] = outputs[name] == outputs["default"]


def resource_usage(path):
    """the compiler's figures of count_windows_tree_kernel (-Rpass-analysis=kernel-resource-usage), per hash count"""
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            h = re.search(r"count_windows_tree_kernelILi(\d)E", m.group(1))
            cur = out.setdefault("H%s" % h.group(1), {}) if h else None
        m = re.search(r"remark:\s+(VGPRs|AGPRs|SGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--windows", type=int, default=200_000)
    ap.add_argument("--step", type=int, default=16, help="values a window slides by (a)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--letters", type=int, default=3000)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--parent", default=None, help="a tree of the parent commit with its build (DIR/tetrex_amd, DIR/bin/tetrex)")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the tree whose build is measured (a child process: the parent's)")
    ap.add_argument("--library", default=None, help="a directory that already holds the library and both indexes (a child process)")
    ap.add_argument("--resource-usage", default=None, help="the compiler's remarks for txq_count.hip, to go with the figures")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    sys.path.insert(0, a.root)
    from tetrex_amd import capi, host  # (before perf_sized_hibf, which puts its own tree first on the path)
    import perf_sized_hibf
    from perf_sized_hibf import library, build
    assert os.path.dirname(os.path.dirname(os.path.abspath(capi.__file__))) == os.path.abspath(a.root)
    capi.init(0)
    res = dict(measured_on="MI355X")
    if a.library:  # the child: the independent route alone, on the files of the process that started it
        files = [line.strip() for line in open(os.path.join(a.library, "bins.lst"))]
        kernels(a, res, a.library, files, True)
        print(json.dumps(res))
        return
    perf_sized_hibf.TETREX = os.path.join(a.root, "bin", "tetrex")
    with tempfile.TemporaryDirectory() as d:
        files, n_recs = library(d, a.bins, 1)
        res["library"] = dict(bins=a.bins, k=6, records=n_recs)
        for name, flags in (("sized", ["--layout", "sized"]), ("uniform", [])):
            res["library"][name + "_bytes"] = build(d, name, files, flags)["bytes"]
        kernels(a, res, d, files, False)
        if a.parent:
            cp = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", a.parent, "--library", d, "--bins", str(a.bins), "--windows", str(a.windows),
                                 "--step", str(a.step), "--reps", str(a.reps)], capture_output=True, text=True, timeout=3000)
            if cp.returncode != 0:
                raise RuntimeError(cp.stderr[-3000:])
            theirs = json.loads(cp.stdout.strip().splitlines()[-1])["kernels"]["trees"]
            for name, tree in res["kernels"]["trees"].items():
                for ratio, r in tree["by_ratio"].items():
                    e = theirs[name]["by_ratio"][ratio]["variants"]["independent"]
                    r["parent_build_independent"] = dict(ms=e["ms"], times_ms=e["times_ms"], over_this_build=e["ms"] / r["variants"]["independent"]["ms"])
        if not a.no_cli:
            command(a, res, d, files, a.root)
    if a.resource_usage:
        res["count_windows_tree_kernel_resource_usage"] = resource_usage(a.resource_usage)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
