"""Measurement of `tetrex search ... --align-windows` (txq_edit_align_windows_device) — not collected by pytest.
One MI355X.  The yardstick is what the verifier would have done without the new call, never the new kernel against itself.

  (a) the call: the nearest windows of §19(b)'s workload — `--records` chimeric records of `--letters` letters (a third from
      one bin, a third random, a third from another bin), W = 120, S = 30, E = 4, `--bins` peptide bins of 20 000 residues in
      ten records; per (record, planted bin) the first window that lies in the planted third, about two pairs a record spread
      over nearly every bin — through ONE txq_edit_align_windows_device call on a table of one view per bin, against
      txq_edit_align_device called once per bin on the same windows written out as patterns, all calls queued on one stream,
      and the host twin (txh_edit_align, 16 threads) beside them.  The triples come from one txq_edit_windows_device call.  The
      device variants are timed in one process, in interleaved rounds, with device events around each; every round is kept and
      the best reported.  All three must give the same words.
  (b) the command: §19(b)'s `tetrex search --window 120 --step 30 -e 4 --verify-windows` on `--records` such records and §20's
      `--translate --frame-window 40 --frame-step 10 -e 2 --verify-frame-windows` on `--records` contigs, each against a
      1024-bin flat peptide index: without the flag, with --align-windows, and with --align-windows under
      TETREX_VERIFY_ALIGN=host; with `--parent DIR` (a build of the parent commit: DIR/bin/tetrex) the parent's command without
      the flag as well.  Wall time of the process, `--reps` interleaved runs after one warm-up run each, every run kept, best
      and spread reported; the rows with the flag must be the rows without it plus four columns, and equal on both routes.
Not measured: an HIBF, nucleotide libraries, hardware counters.

    python tests/perf_search_align_windows.py [--records 2000] [--bins 1024] [--reps 5] [--no-call] [--no-cli] [--parent DIR]
                                              [--out profiles/search_align_windows.json]
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
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from perf_search_verify_windows import AA, RESIDUES, RECORD, chimeras  # noqa: E402
from perf_search_frame_window import NT, CODON_OF, COMPLEMENT  # noqa: E402

TETREX = os.path.join(ROOT, "bin", "tetrex")


def note(*what):
    print("[perf_search_align_windows]", *what, file=sys.stderr, flush=True)


def call(a, res):
    import torch
    from tetrex_amd import capi, host
    import edit_ref as E
    rng = np.random.default_rng(19)
    W, S, cap = a.window, a.window_step, a.errors
    n_rec = RESIDUES // RECORD
    seqs = [AA[rng.integers(0, 20, size=RESIDUES)].tobytes() for _ in range(a.bins)]
    recs = chimeras(rng, seqs, a.records, a.letters)
    third = a.letters // 3
    let = np.frombuffer(b"".join(r for _, _, r in recs), dtype=np.uint8)
    win_begin, pairs = [], []  # the nearest window of a run of exact windows is its first one
    for q, (x, y, _) in enumerate(recs):
        for lo, b in ((0, x), (a.letters - third, y)):
            at = (lo + S - 1) // S * S
            pairs.append((len(win_begin), b, cap))
            win_begin.append(q * a.letters + at)
    order = sorted(range(len(pairs)), key=lambda i: pairs[i][1])  # by bin, as the verifier sends them
    pairs, win_begin = [pairs[i] for i in order], [win_begin[i] for i in order]
    pairs = [(i, b, cap) for i, (_, b, cap) in enumerate(pairs)]
    n = len(pairs)
    wb, wl = np.array(win_begin, dtype=np.uint64), np.full(n, W, dtype=np.uint32)
    text = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    rec_off = np.arange(0, a.bins * RESIDUES + 1, RECORD, dtype=np.uint64)
    grp_off = np.arange(0, a.bins * n_rec + 1, n_rec, dtype=np.uint64)
    pr = np.array(pairs, dtype=np.uint32)
    codes = E.letter_codes("ABCDEFGHIJKLMNOPQRSTUVWXYZ")
    max_errors = min(cap, capi.EDIT_ALIGN_MAX_DISTANCE)
    stride = capi.edit_align_stride(max_errors)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()
    d_let, d_wb, d_wl, d_text, d_rec, d_grp, d_pr, d_codes = (dev(x) for x in (np.concatenate([let, np.zeros(16, np.uint8)]), wb, wl,
                                                                                 np.concatenate([text, np.zeros(16, np.uint8)]), rec_off, grp_off, pr, codes))
    L = capi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    # the triples: one windowed search over all pairs; r comes back counted over all records and goes down counted in its bin
    d_res = torch.zeros(n * 12, dtype=torch.uint8, device="cuda")
    work = torch.empty(capi.edit_windows_workspace_bytes(n) // 8 + 1, dtype=torch.int64, device="cuda")
    capi.check(L.txq_edit_windows_device(d_let.data_ptr(), let.size, d_wb.data_ptr(), d_wl.data_ptr(), n, d_text.data_ptr(), d_rec.data_ptr(), rec_off.size - 1,
                                         text.size, d_grp.data_ptr(), a.bins, d_pr.data_ptr(), n, d_codes.data_ptr(), d_res.data_ptr(), work.data_ptr(), stream))
    torch.cuda.synchronize()
    flat = d_res.cpu().numpy().view(np.uint32).reshape(n, 3).copy()
    if (flat[:, 0] == 0xFFFFFFFF).any():
        raise RuntimeError("a planted window was not found")
    local = flat.copy()
    local[:, 1] -= (pr[:, 1] * n_rec).astype(np.uint32)
    d_local = dev(local)
    # the new route: one view per bin (its text where it lies, offsets of its own), one call
    view_rec = np.tile(np.arange(0, RESIDUES + 1, RECORD, dtype=np.uint64), a.bins)
    d_view_rec = dev(view_rec)
    views = np.zeros((a.bins, 4), dtype=np.uint64)
    for b in range(a.bins):
        views[b] = (d_text.data_ptr() + b * RESIDUES, d_view_rec.data_ptr() + 8 * b * (n_rec + 1), n_rec, RESIDUES)
    d_views = dev(views)
    out_new = torch.zeros(n * stride * 4, dtype=torch.uint8, device="cuda")
    out_old = torch.zeros(n * stride * 4, dtype=torch.uint8, device="cuda")

    def one_call():
        capi.check(L.txq_edit_align_windows_device(d_let.data_ptr(), let.size, d_wb.data_ptr(), d_wl.data_ptr(), n, d_views.data_ptr(), a.bins, d_pr.data_ptr(), n,
                                                   d_local.data_ptr(), d_codes.data_ptr(), max_errors, out_new.data_ptr(), None, stream))
    # the yardstick: the windows written out, txq_edit_align_device once per bin on the bin's own text, its records one group
    written = np.concatenate([let[b:b + W] for b in win_begin])
    d_written, d_po = dev(np.concatenate([written, np.zeros(16, np.uint8)])), dev(np.arange(n + 1, dtype=np.uint64) * np.uint64(W))
    d_bin_pr = dev(np.array([(i, 0, cap) for i in range(n)], dtype=np.uint32))
    d_bin_grp = dev(np.array([0, n_rec], dtype=np.uint64))
    runs_of_bins, i = [], 0
    while i < n:
        e = i
        while e < n and pairs[e][1] == pairs[i][1]:
            e += 1
        runs_of_bins.append((pairs[i][1], i, e))
        i = e

    def per_bin():
        for b, lo, hi in runs_of_bins:
            capi.check(L.txq_edit_align_device(d_written.data_ptr(), d_po.data_ptr(), n, written.size, d_text.data_ptr() + b * RESIDUES,
                                               d_view_rec.data_ptr() + 8 * b * (n_rec + 1), n_rec, RESIDUES, d_bin_grp.data_ptr(), 1, d_bin_pr.data_ptr() + 12 * lo,
                                               hi - lo, d_local.data_ptr() + 12 * lo, d_codes.data_ptr(), max_errors, out_old.data_ptr() + 4 * stride * lo, None, stream))
    variants = {"one_call_all_bins": one_call, "one_call_per_bin": per_bin}
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    records = [s[i:i + RECORD] for s in seqs for i in range(0, RESIDUES, RECORD)]
    patterns = [written[i * W:(i + 1) * W].tobytes() for i in range(n)]
    t = time.perf_counter()
    want = host.edit_align(patterns, records, grp_off, pairs, flat, codes, max_errors, threads=16, raw=True)
    host_s = [time.perf_counter() - t]
    for _ in range(a.reps - 1):
        t = time.perf_counter()
        host.edit_align(patterns, records, grp_off, pairs, flat, codes, max_errors, threads=16, raw=True)
        host_s.append(time.perf_counter() - t)
    new, old = (o.cpu().numpy().view(np.uint32).reshape(n, stride) for o in (out_new, out_old))
    if not (np.array_equal(new, want) and np.array_equal(old, want)):
        raise RuntimeError("the routes give different words")
    every = {name: [] for name in variants}
    for _ in range(a.reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            every[name].append(round(e0.elapsed_time(e1), 4))
    res["call"] = dict(bins=a.bins, residues_per_bin=RESIDUES, records=a.records, letters=a.letters, window=W, step=S, errors=cap, pairs=n,
                       bins_with_a_pair=len(runs_of_bins), distances=sorted(set(int(d) for d in flat[:, 0])),
                       timing="device events around each variant, %d interleaved rounds in one process; host twin: wall time of txh_edit_align, 16 threads" % a.reps,
                       ms={name: dict(best=min(r), runs=r) for name, r in every.items()},
                       host_twin_ms=dict(best=round(1e3 * min(host_s), 4), runs=[round(1e3 * s, 4) for s in host_s]),
                       per_bin_over_one_call=min(every["one_call_per_bin"]) / min(every["one_call_all_bins"]), words_equal=True)
    note("call: one call %.3f ms, a call per bin %.3f ms, host twin %.3f ms" % (min(every["one_call_all_bins"]), min(every["one_call_per_bin"]), 1e3 * min(host_s)))


def library(d, rng, bins):
    files, seqs = [], []
    for b in range(bins):
        seq = AA[rng.integers(0, 20, size=RESIDUES)].tobytes()
        p = os.path.join(d, "bin%04d.fa" % b)
        with open(p, "wb") as f:
            f.write(b"".join(b">b%d_%d\n%s\n" % (b, i, seq[i:i + RECORD]) for i in range(0, RESIDUES, RECORD)))
        files.append(p)
        seqs.append(seq)
    lst = os.path.join(d, "bins.lst")
    with open(lst, "w") as f:
        f.write("\n".join(files) + "\n")
    r = subprocess.run([TETREX, "index", "-k", "6", "-i", os.path.join(d, "flat"), lst], capture_output=True, text=True, timeout=1800)
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    return seqs, os.path.join(d, "flat.ibf")


def command(a, res):
    rng = np.random.default_rng(5)
    bins = 1024
    with tempfile.TemporaryDirectory() as d:
        seqs, index = library(d, rng, bins)
        note("library and index ready")
        qpath = os.path.join(d, "chimeras.fa")
        with open(qpath, "wb") as f:
            f.write(b"".join(b">c%d_b%d_b%d\n%s\n" % (q, x, y, s) for q, (x, y, s) in enumerate(chimeras(rng, seqs, a.records, a.letters))))
        stretch, contig = 300, 9000
        back = lambda pep: "".join(CODON_OF[c] for c in pep.decode()).encode()
        flank = (contig - 6 * stretch) // 3
        cpath = os.path.join(d, "contigs.fa")
        with open(cpath, "wb") as f:
            for q in range(a.records):
                x, y = (int(v) for v in rng.choice(bins, size=2, replace=False))
                ax, ay = int(rng.integers(0, RESIDUES - stretch)), int(rng.integers(0, RESIDUES - stretch))
                parts = [NT[rng.integers(0, 4, size=flank + int(rng.integers(0, 3)))].tobytes(), back(seqs[x][ax:ax + stretch]),
                         NT[rng.integers(0, 4, size=flank)].tobytes(), back(seqs[y][ay:ay + stretch]).translate(COMPLEMENT)[::-1],
                         NT[rng.integers(0, 4, size=flank)].tobytes()]
                f.write(b">c%d_b%d_b%d\n%s\n" % (q, x, y, b"".join(parts)))
        workloads = {
            "windows": (["search", "--window", str(a.window), "--step", str(a.window_step), "-e", str(a.errors), "--verify-windows", "-v"], qpath),
            "frame_windows": (["search", "--translate", "--frame-window", "40", "--frame-step", "10", "-e", "2", "--verify-frame-windows", "-v"], cpath),
        }
        res["command"] = dict(bins=bins, residues_per_bin=RESIDUES, k=6, records=a.records,
                              timing="wall time of the process, %d interleaved runs after one warm-up run each; best, spread (max - min) and all runs" % a.reps)
        for wname, (flags, queries) in workloads.items():
            legs = {"verify": ([TETREX] + flags + [index, queries], {}),
                    "align_windows": ([TETREX] + flags + ["--align-windows", index, queries], {}),
                    "align_windows_host": ([TETREX] + flags + ["--align-windows", index, queries], {"TETREX_VERIFY_ALIGN": "host"})}
            if a.parent:
                legs["verify_parent_build"] = ([os.path.join(a.parent, "bin", "tetrex")] + flags + [index, queries], {})
            out, outputs = {}, {}
            for rep in range(a.reps + 1):
                for name, (cmd, env) in legs.items():
                    t = time.perf_counter()
                    cp = subprocess.run(cmd, capture_output=True, text=True, timeout=1800, env=dict(os.environ, TETREX_TRACE="1", **env))
                    wall = time.perf_counter() - t
                    if cp.returncode != 0:
                        raise RuntimeError(cp.stderr)
                    if rep == 0:
                        outputs[name] = cp.stdout
                        out[name] = dict(rows=len(cp.stdout.splitlines()), wall_s=[], search_time_s=[],
                                         notes=[l for l in cp.stderr.splitlines() if l.startswith(("Windows:", "Verified:")) or "verify routes" in l or "align windows" in l])
                        continue
                    out[name]["wall_s"].append(round(wall, 4))
                    out[name]["search_time_s"].append(float(cp.stderr.split("Search time:")[1].split()[0]))
            for e in out.values():
                e["best_wall_s"], e["spread_wall_s"] = min(e["wall_s"]), round(max(e["wall_s"]) - min(e["wall_s"]), 4)
                e["best_search_time_s"] = min(e["search_time_s"])
            if outputs["align_windows"] != outputs["align_windows_host"]:
                raise RuntimeError("%s: the device route and the host twin print different rows" % wname)
            if outputs["verify"].splitlines() != ["\t".join(l.split("\t")[:-4]) for l in outputs["align_windows"].splitlines()]:
                raise RuntimeError("%s: --align-windows changes the columns in front of its own" % wname)
            if a.parent and outputs["verify_parent_build"] != outputs["verify"]:
                raise RuntimeError("%s: the rows without the flag differ from the parent build's" % wname)
            m = re.search(r"align windows: device (\d+), host (\d+), calls (\d+)", "\n".join(out["align_windows"]["notes"]))
            res["command"][wname] = dict(legs=out, rows_equal_on_both_routes=True, prefix_equals_rows_without_the_flag=True,
                                         rows_equal_parent_build=bool(a.parent), aligned_on_device=int(m.group(1)), aligned_on_host=int(m.group(2)),
                                         align_calls=int(m.group(3)),
                                         align_cost_device_s=out["align_windows"]["best_wall_s"] - out["verify"]["best_wall_s"],
                                         align_cost_host_s=out["align_windows_host"]["best_wall_s"] - out["verify"]["best_wall_s"])
            note(wname, "verify %.2f s, --align-windows %.2f s, on the host %.2f s" % tuple(out[x]["best_wall_s"] for x in ("verify", "align_windows", "align_windows_host")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--bins", type=int, default=1024, help="bins of the call measurement (a)")
    ap.add_argument("--letters", type=int, default=3000)
    ap.add_argument("--window", type=int, default=120)
    ap.add_argument("--window-step", type=int, default=30)
    ap.add_argument("--errors", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-call", action="store_true")
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--parent", default=None, help="a build of the parent commit (DIR/bin/tetrex) for the commands without the flag")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from tetrex_amd import capi
    capi.init(0)
    res = dict(measured_on="MI355X")
    if not a.no_call:
        call(a, res)
    if not a.no_cli:
        command(a, res)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
