"""Measurement of `tetrex search ... --window-targets` (txq_edit_window_targets_device) — not collected by pytest.
One MI355X.  The yardstick is what the parent commit's code would have forced, never the new kernel against itself.

  (a) the call: §19(b)'s candidates — `--records` chimeric records of `--letters` letters (a third from one bin, a third random,
      a third from another bin), W = 120, S = 30, E = 4, every window that lies in a planted third paired with its bin — on
      `--bins` peptide bins that are FAMILIES: ten records of 2 000 residues, record i the family's base with i per cent of its
      residues substituted, so that a window is within E of the first members only (between one and eight hits a pair).  ONE
      txq_edit_window_targets_device call on a table of one view per bin, against txq_edit_targets_device called once per bin on
      the same windows written out as patterns (all calls queued on one stream), and the host twin (txh_edit_targets, 16 threads)
      beside them.  The device variants are timed in one process, in interleaved rounds, with device events around each; every
      round is kept and the best reported.  All three must give the same hits.
  (b) the command: `tetrex search --window 120 --step 30 -e 4 --verify-windows` on `--records` such records against a 1024-bin
      flat peptide index of such families: without the flag, with --window-targets, and with --window-targets under
      TETREX_VERIFY_TARGETS=host; with `--parent DIR` (a build of the parent commit: DIR/bin/tetrex) the parent's command without
      the flag as well.  Wall time of the process and its `Search time`, `--reps` interleaved runs after one warm-up run each,
      every run kept, best and spread reported; both routes must print the same rows, and the rows without the flag must be the
      parent build's.
Not measured: an HIBF, nucleotide libraries, the frame-window command, hardware counters.

    python tests/perf_search_window_targets.py [--records 2000] [--bins 1024] [--reps 5] [--no-call] [--no-cli] [--parent DIR]
                                               [--out profiles/search_window_targets.json]
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

TETREX = os.path.join(ROOT, "bin", "tetrex")
MEMBERS = RESIDUES // RECORD


def note(*what):
    print("[perf_search_window_targets]", *what, file=sys.stderr, flush=True)


def family(rng):
    """a bin: MEMBERS records of RECORD residues, record i the base with i per cent of its residues substituted"""
    base = AA[rng.integers(0, 20, size=RECORD)]
    out = []
    for i in range(MEMBERS):
        mine = base.copy()
        at = rng.random(RECORD) < 0.01 * i
        mine[at] = AA[rng.integers(0, 20, size=int(at.sum()))]
        out.append(mine.tobytes())
    return b"".join(out)


def call(a, res):
    import torch
    from tetrex_amd import capi, host
    import edit_ref as E
    rng = np.random.default_rng(19)
    W, S, cap = a.window, a.window_step, a.errors
    seqs = [family(rng) for _ in range(a.bins)]
    recs = chimeras(rng, seqs, a.records, a.letters)
    third = a.letters // 3
    let = np.frombuffer(b"".join(r for _, _, r in recs), dtype=np.uint8)
    win_begin, pairs = [], []
    for q, (x, y, _) in enumerate(recs):
        for at in range(0, a.letters - W + 1, S):
            for lo, hi, b in ((0, third, x), (a.letters - third, a.letters, y)):
                if at >= lo and at + W <= hi:
                    pairs.append((len(win_begin), b, cap))
                    win_begin.append(q * a.letters + at)
    order = sorted(range(len(pairs)), key=lambda i: (pairs[i][1], i))  # by bin and by window within the bin, as the verifier sends them
    pairs, win_begin = [pairs[i] for i in order], [win_begin[i] for i in order]
    pairs = [(i, b, cap) for i, (_, b, cap) in enumerate(pairs)]
    n = len(pairs)
    n_slots = n * MEMBERS
    wb, wl = np.array(win_begin, dtype=np.uint64), np.full(n, W, dtype=np.uint32)
    text = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    pr = np.array(pairs, dtype=np.uint32)
    codes = E.letter_codes("ABCDEFGHIJKLMNOPQRSTUVWXYZ")
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()
    d_let, d_wb, d_wl, d_text, d_pr, d_codes = (dev(x) for x in (np.concatenate([let, np.zeros(16, np.uint8)]), wb, wl, np.concatenate([text, np.zeros(16, np.uint8)]),
                                                                   pr, codes))
    view_rec = np.tile(np.arange(0, RESIDUES + 1, RECORD, dtype=np.uint64), a.bins)
    d_view_rec = dev(view_rec)
    views = np.zeros((a.bins, 4), dtype=np.uint64)
    for b in range(a.bins):
        views[b] = (d_text.data_ptr() + b * RESIDUES, d_view_rec.data_ptr() + 8 * b * (MEMBERS + 1), MEMBERS, RESIDUES)
    d_views = dev(views)
    L = capi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    new = dict(hits=torch.zeros(n_slots * 16, dtype=torch.uint8, device="cuda"), total=torch.zeros(8, dtype=torch.uint8, device="cuda"),
               status=torch.zeros(n * 4 + 4, dtype=torch.uint8, device="cuda"),
               work=torch.empty(capi.edit_window_targets_workspace(n, n_slots) // 8 + 1, dtype=torch.int64, device="cuda"))

    def one_call():
        capi.check(L.txq_edit_window_targets_device(d_let.data_ptr(), let.size, d_wb.data_ptr(), d_wl.data_ptr(), n, d_views.data_ptr(), a.bins, d_pr.data_ptr(), n,
                                                    d_codes.data_ptr(), new["hits"].data_ptr(), n_slots, new["total"].data_ptr(), new["status"].data_ptr(), n_slots,
                                                    new["work"].data_ptr(), stream))
    # the yardstick: the windows written out, txq_edit_targets_device once per bin on the bin's own text, its records one group
    written = np.concatenate([let[b:b + W] for b in win_begin])
    d_written, d_po = dev(np.concatenate([written, np.zeros(16, np.uint8)])), dev(np.arange(n + 1, dtype=np.uint64) * np.uint64(W))
    d_bin_pr = dev(np.array([(i, 0, cap) for i in range(n)], dtype=np.uint32))
    d_bin_grp = dev(np.array([0, MEMBERS], dtype=np.uint64))
    runs_of_bins, i = [], 0
    while i < n:
        e = i
        while e < n and pairs[e][1] == pairs[i][1]:
            e += 1
        runs_of_bins.append((pairs[i][1], i, e))
        i = e
    old = dict(hits=torch.zeros(n_slots * 16, dtype=torch.uint8, device="cuda"), total=torch.zeros(8 * len(runs_of_bins), dtype=torch.uint8, device="cuda"),
               status=torch.zeros(n * 4 + 4, dtype=torch.uint8, device="cuda"),
               work=torch.empty(sum(capi.edit_targets_workspace(hi - lo, (hi - lo) * MEMBERS) + 8 for _, lo, hi in runs_of_bins) // 8 + 1, dtype=torch.int64, device="cuda"))

    def per_bin():
        work = old["work"].data_ptr()
        for c, (b, lo, hi) in enumerate(runs_of_bins):
            slots = (hi - lo) * MEMBERS
            capi.check(L.txq_edit_targets_device(d_written.data_ptr(), d_po.data_ptr(), n, written.size, d_text.data_ptr() + b * RESIDUES,
                                                 d_view_rec.data_ptr() + 8 * b * (MEMBERS + 1), MEMBERS, RESIDUES, d_bin_grp.data_ptr(), 1, d_bin_pr.data_ptr() + 12 * lo,
                                                 hi - lo, d_codes.data_ptr(), old["hits"].data_ptr() + 16 * lo * MEMBERS, slots, old["total"].data_ptr() + 8 * c,
                                                 old["status"].data_ptr() + 4 * lo, slots, work, stream))
            work += (capi.edit_targets_workspace(hi - lo, slots) + 15) // 8 * 8
    variants = {"one_call_all_bins": one_call, "one_call_per_bin": per_bin}
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    total = int(new["total"].cpu().numpy().view(np.uint64)[0])
    got = new["hits"].cpu().numpy().view(np.uint32).reshape(-1, 4)[:total].copy()
    totals = old["total"].cpu().numpy().view(np.uint64)
    area = old["hits"].cpu().numpy().view(np.uint32).reshape(-1, 4)
    parts = []
    for c, (b, lo, hi) in enumerate(runs_of_bins):
        rows = area[lo * MEMBERS:lo * MEMBERS + int(totals[c])].copy()
        rows[:, 0] += lo
        parts.append(rows)
    per_bin_hits = np.concatenate(parts)
    records = [s[i:i + RECORD] for s in seqs for i in range(0, RESIDUES, RECORD)]
    grp_off = np.arange(0, a.bins * MEMBERS + 1, MEMBERS, dtype=np.uint64)
    patterns = [written[i * W:(i + 1) * W].tobytes() for i in range(n)]
    host_s, want = [], None
    for _ in range(a.reps):
        t = time.perf_counter()
        want, _ = host.edit_targets(patterns, records, grp_off, pairs, codes, threads=16)
        host_s.append(time.perf_counter() - t)
    want = want.copy()
    want[:, 2] -= (pr[want[:, 0], 1] * MEMBERS).astype(np.uint32)  # (r counted in its bin)
    if not (np.array_equal(got, want) and np.array_equal(per_bin_hits, want)) or new["status"].any() or old["status"].any():
        raise RuntimeError("the routes give different hits")
    per_pair = np.bincount(want[:, 0], minlength=n)
    every = {name: [] for name in variants}
    for _ in range(a.reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            every[name].append(round(e0.elapsed_time(e1), 4))
    res["call"] = dict(bins=a.bins, residues_per_bin=RESIDUES, records_per_bin=MEMBERS, records=a.records, letters=a.letters, window=W, step=S, errors=cap, pairs=n,
                       slots=n_slots, hits=int(total), hits_per_pair=dict(least=int(per_pair.min()), most=int(per_pair.max()), mean=float(per_pair.mean())),
                       bins_with_a_pair=len(runs_of_bins),
                       timing="device events around each variant, %d interleaved rounds in one process; host twin: wall time of txh_edit_targets, 16 threads" % a.reps,
                       ms={name: dict(best=min(r), runs=r) for name, r in every.items()},
                       host_twin_ms=dict(best=round(1e3 * min(host_s), 4), runs=[round(1e3 * s, 4) for s in host_s]),
                       per_bin_over_one_call=min(every["one_call_per_bin"]) / min(every["one_call_all_bins"]), hits_equal=True)
    note("call: %d pairs, %d hits; one call %.3f ms, a call per bin %.3f ms, host twin %.3f ms" %
         (n, total, min(every["one_call_all_bins"]), min(every["one_call_per_bin"]), 1e3 * min(host_s)))


def command(a, res):
    rng = np.random.default_rng(5)
    bins = 1024
    with tempfile.TemporaryDirectory() as d:
        files, seqs = [], []
        for b in range(bins):
            seq = family(rng)
            p = os.path.join(d, "bin%04d.fa" % b)
            with open(p, "wb") as f:
                f.write(b"".join(b">b%d_%d\n%s\n" % (b, i // RECORD, seq[i:i + RECORD]) for i in range(0, RESIDUES, RECORD)))
            files.append(p)
            seqs.append(seq)
        lst = os.path.join(d, "bins.lst")
        with open(lst, "w") as f:
            f.write("\n".join(files) + "\n")
        r = subprocess.run([TETREX, "index", "-k", "6", "-i", os.path.join(d, "flat"), lst], capture_output=True, text=True, timeout=1800)
        if r.returncode != 0:
            raise RuntimeError(r.stderr)
        index = os.path.join(d, "flat.ibf")
        note("library and index ready")
        qpath = os.path.join(d, "chimeras.fa")
        with open(qpath, "wb") as f:
            f.write(b"".join(b">c%d_b%d_b%d\n%s\n" % (q, x, y, s) for q, (x, y, s) in enumerate(chimeras(rng, seqs, a.records, a.letters))))
        flags = ["search", "--window", str(a.window), "--step", str(a.window_step), "-e", str(a.errors), "--verify-windows", "-v"]
        legs = {"verify": ([TETREX] + flags + [index, qpath], {}),
                "window_targets": ([TETREX] + flags + ["--window-targets", index, qpath], {}),
                "window_targets_host": ([TETREX] + flags + ["--window-targets", index, qpath], {"TETREX_VERIFY_TARGETS": "host"})}
        if a.parent:
            legs["verify_parent_build"] = ([os.path.join(a.parent, "bin", "tetrex")] + flags + [index, qpath], {})
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
                                     notes=[l for l in cp.stderr.splitlines() if l.startswith(("Windows:", "Verified:", "Targets:")) or "verify routes" in l or "window targets" in l])
                    continue
                out[name]["wall_s"].append(round(wall, 4))
                out[name]["search_time_s"].append(float(cp.stderr.split("Search time:")[1].split()[0]))
        for e in out.values():
            e["best_wall_s"], e["spread_wall_s"] = min(e["wall_s"]), round(max(e["wall_s"]) - min(e["wall_s"]), 4)
            e["best_search_time_s"], e["spread_search_time_s"] = min(e["search_time_s"]), round(max(e["search_time_s"]) - min(e["search_time_s"]), 4)
        if outputs["window_targets"] != outputs["window_targets_host"]:
            raise RuntimeError("the device route and the host route print different rows")
        if a.parent and outputs["verify_parent_build"] != outputs["verify"]:
            raise RuntimeError("the rows without the flag differ from the parent build's")
        m = re.search(r"window targets: device (\d+), host (\d+), calls (\d+)", "\n".join(out["window_targets"]["notes"]))
        dev_best, host_best = out["window_targets"]["best_wall_s"], out["window_targets_host"]["best_wall_s"]
        spread = max(out["window_targets"]["spread_wall_s"], out["window_targets_host"]["spread_wall_s"])
        res["command"] = dict(bins=bins, residues_per_bin=RESIDUES, records_per_bin=MEMBERS, k=6, records=a.records,
                              timing="wall time of the process, %d interleaved runs after one warm-up run each; best, spread (max - min) and all runs" % a.reps,
                              legs=out, rows_equal_on_both_routes=True, rows_without_the_flag_equal_parent_build=bool(a.parent),
                              candidates_on_device=int(m.group(1)), candidates_on_host=int(m.group(2)), calls=int(m.group(3)),
                              default_rule=dict(device_best_wall_s=dev_best, host_best_wall_s=host_best, larger_spread_s=spread,
                                                device_stays_default=not (dev_best > host_best + spread)))
        note("verify %.2f s, --window-targets %.2f s, on the host %.2f s" % tuple(out[x]["best_wall_s"] for x in ("verify", "window_targets", "window_targets_host")))


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
    ap.add_argument("--parent", default=None, help="a build of the parent commit (DIR/bin/tetrex) for the command without the flag")
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
