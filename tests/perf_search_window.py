"""Measurement of the sliding window count (txq_count_windows, `tetrex search --window`) — not collected by
pytest.  One MI355X.

  (a) kernels: txq_count_windows_device on the flat 1024-bin index of bench.py (S-IBF-1024: h = 3, 1 247 045 rows, 200 000
      values per bin) over `--windows` windows that slide by `--step` values, of step x 2, 4, 8 and 16 values each, for every
      unit size of `--units` and for one and four waves per unit — against the same windows written out as duplicated
      disjoint queries through txq_count_device.  All variants are timed in the same process, in interleaved rounds, with
      device events around each call; the figure of a variant is its best of `--reps` rounds.  The hit matrices of the
      routes are compared.  rows_ratio is what the sliding kernel gathers of the baseline's rows by count,
      (w + (U - 1) 2 S) / (U w).
  (b) the command: `tetrex search -e E` with and without --window on `--records` chimeric records of `--letters` letters
      (a third from one bin, a third random, a third from another bin) against a 1024-bin flat peptide index, wall time
      and rows; with `--parent DIR` (a build of the parent commit: DIR/bin/tetrex) the plain search of that build on the
      same file too, interleaved.

    python tests/perf_search_window.py [--windows 200000] [--step 16] [--units 4,8,16,32,64] [--reps 5] [--no-cli]
                                       [--parent DIR] [--out profiles/search_window.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
TETREX = os.path.join(ROOT, "bin", "tetrex")
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)


def kernels(a, res):
    import torch
    import bench
    from helpers import splitmix64
    from tetrex_amd import capi
    bins, h, rows, per_bin, bits = 1024, 3, 1247045, 200000, 20
    ix = bench.build_index(capi, torch, bins, bins, rows, h, 0, 1, per_bin, bits)
    W = ix.shard_words
    stream = torch.cuda.current_stream().cuda_stream
    n, S = a.windows, a.step
    dev = lambda x: torch.from_numpy(x).cuda()
    out = res["kernels"] = dict(index="S-IBF-1024 of bench.py (1024 bins, h = 3, %d rows, %d values per bin)" % (rows, per_bin), windows=n, step_values=S,
                                timing="device events around each call, best of %d interleaved rounds in one process" % a.reps, by_ratio={})
    for ratio in (2, 4, 8, 16):
        w = S * ratio
        values = splitmix64(7 + ratio, n * S + w) >> np.uint64(64 - bits)
        begins = np.arange(n, dtype=np.uint64) * np.uint64(S)
        lens = np.full(n, w, dtype=np.uint32)
        thr = np.full(n, max(1, w // 8), dtype=np.uint32)
        d_val, d_beg, d_len, d_thr = dev(values.view(np.int64)), dev(begins.view(np.int64)), dev(lens.view(np.int32)), dev(thr.view(np.int32))
        idx = d_beg[:, None] + torch.arange(w, device="cuda", dtype=torch.int64)[None, :]
        d_dup = d_val[idx.reshape(-1)].contiguous()  # the windows written out
        del idx
        d_off = torch.arange(n + 1, device="cuda", dtype=torch.int64) * w
        hit_w = torch.zeros(n * W, dtype=torch.int64, device="cuda")
        hit_b = torch.zeros(n * W, dtype=torch.int64, device="cuda")
        variants = {"baseline": lambda: ix.count_device(d_dup.data_ptr(), d_off.data_ptr(), n, d_thr.data_ptr(), hit_b.data_ptr(), None, stream)}
        for U in a.units:
            for waves in (1, 4):
                def run(U=U, waves=waves):
                    os.environ["TXQ_COUNT_WINDOWS_UNIT"] = str(U)
                    os.environ["TXQ_COUNT_WINDOWS_WAVES"] = str(waves)
                    ix.count_windows_device(d_val.data_ptr(), d_beg.data_ptr(), d_len.data_ptr(), n, d_thr.data_ptr(), hit_w.data_ptr(), None, stream)
                variants["U%d_waves%d" % (U, waves)] = run
        best = {}
        for name, fn in variants.items():  # warm-up, and the routes must agree
            fn()
            torch.cuda.synchronize()
            if name != "baseline" and not torch.equal(hit_w, hit_b):
                raise RuntimeError("%s: hits differ from txq_count_device's at w = %d" % (name, w))
            hit_w.zero_()
        for _ in range(a.reps):
            for name, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1)
                best[name] = min(best.get(name, ms), ms)
        r = out["by_ratio"][str(ratio)] = dict(window_values=w, baseline_ms=best["baseline"], hit_fraction=float((hit_b != 0).float().mean()), variants={})
        for name, ms in best.items():
            if name == "baseline":
                continue
            U = int(name[1:].split("_")[0])
            r["variants"][name] = dict(ms=ms, time_ratio=ms / best["baseline"], rows_ratio=(w + (U - 1) * 2 * S) / (U * w))
        fastest = min(r["variants"], key=lambda k: r["variants"][k]["ms"])
        r["fastest"] = fastest
        r["fastest_time_ratio"] = r["variants"][fastest]["time_ratio"]
        del d_dup, d_off, hit_w, hit_b
        torch.cuda.empty_cache()
    os.environ.pop("TXQ_COUNT_WINDOWS_UNIT", None)
    os.environ.pop("TXQ_COUNT_WINDOWS_WAVES", None)
    ix.free()


def command(a, res):
    rng = np.random.default_rng(5)
    bins, residues, k = 1024, 20000, 6
    with tempfile.TemporaryDirectory() as d:
        files, seqs = [], []
        for b in range(bins):
            seq = AA[rng.integers(0, 20, size=residues)].tobytes()
            p = os.path.join(d, "bin%04d.fa" % b)
            with open(p, "wb") as f:
                f.write(b"".join(b">b%d_%d\n%s\n" % (b, i, seq[i:i + 2000]) for i in range(0, residues, 2000)))
            files.append(p)
            seqs.append(seq)
        third = a.letters // 3
        recs = []
        for q in range(a.records):
            x, y = (int(v) for v in rng.choice(bins, size=2, replace=False))
            ax, ay = int(rng.integers(0, 10)) * 2000, int(rng.integers(0, 10)) * 2000
            mid = AA[rng.integers(0, 20, size=a.letters - 2 * third)].tobytes()
            recs.append(b">c%d_b%d_b%d\n%s\n" % (q, x, y, seqs[x][ax:ax + third] + mid + seqs[y][ay:ay + third]))
        qpath = os.path.join(d, "chimeras.fa")
        with open(qpath, "wb") as f:
            f.write(b"".join(recs))
        lst = os.path.join(d, "bins.lst")
        with open(lst, "w") as f:
            f.write("\n".join(files) + "\n")
        r = subprocess.run([TETREX, "index", "-k", str(k), "-i", os.path.join(d, "flat"), lst], capture_output=True, text=True, timeout=1800)
        if r.returncode != 0:
            raise RuntimeError(r.stderr)
        index = os.path.join(d, "flat.ibf")
        legs = {"window": [TETREX, "search", "--window", str(a.window), "--step", str(a.window_step), "-e", str(a.errors), "-v", index, qpath],
                "plain": [TETREX, "search", "-e", str(a.errors), "-v", index, qpath]}
        if a.parent:
            legs["plain_parent_build"] = [os.path.join(a.parent, "bin", "tetrex"), "search", "-e", str(a.errors), "-v", index, qpath]
        out = res["command"] = dict(bins=bins, residues_per_bin=residues, k=k, records=a.records, letters=a.letters, window=a.window, step=a.window_step,
                                    errors=a.errors, timing="wall time of the process, best of %d interleaved runs after one warm-up run each" % a.reps, legs={})
        outputs = {}
        for rep in range(a.reps + 1):
            for name, cmd in legs.items():
                t = time.perf_counter()
                cp = subprocess.run(cmd, capture_output=True, text=True, timeout=1800)
                wall = time.perf_counter() - t
                if cp.returncode != 0:
                    raise RuntimeError(cp.stderr)
                outputs[name] = cp.stdout
                if rep == 0:
                    out["legs"][name] = dict(rows=len(cp.stdout.splitlines()), stderr_tail=cp.stderr.strip().splitlines()[-2:])
                    continue
                e = out["legs"][name]
                e["wall_s"] = min(e.get("wall_s", wall), wall)
                e["search_time_s"] = min(e.get("search_time_s", 1e9), float(cp.stderr.split("Search time:")[1].split()[0]))
        if a.parent:
            out["plain_rows_equal_parent_build"] = outputs["plain"] == outputs["plain_parent_build"]
        # how many chimeras are found in both of their bins
        found = set()
        for line in outputs["window"].splitlines():
            f = line.split("\t")
            found.add((f[0], f[1]))
        both = 0
        for q in range(a.records):
            name = recs[q].split(b"\n")[0][1:].decode()
            x, y = (int(s[1:]) for s in name.split("_")[1:])
            both += (name, os.path.abspath(files[x])) in found and (name, os.path.abspath(files[y])) in found
        out["window_both_bins_reported"] = both / a.records
        out["plain_records_with_a_row"] = len({line.split("\t")[0] for line in outputs["plain"].splitlines()}) / a.records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=200_000)
    ap.add_argument("--step", type=int, default=16, help="values a window slides by (a)")
    ap.add_argument("--units", default="4,8,16,32,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--letters", type=int, default=3000)
    ap.add_argument("--window", type=int, default=120, help="letters of a window (b)")
    ap.add_argument("--window-step", type=int, default=30)
    ap.add_argument("--errors", type=int, default=4)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--parent", default=None, help="a build of the parent commit (DIR/bin/tetrex) for the plain search")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.units = [int(u) for u in a.units.split(",")]
    from tetrex_amd import capi
    capi.init(0)
    res = dict(measured_on="MI355X")
    if not a.no_kernels:
        kernels(a, res)
    if not a.no_cli:
        command(a, res)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
