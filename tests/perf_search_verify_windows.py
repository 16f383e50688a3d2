"""Measurement of the windowed edit-distance call (txq_edit_windows, `tetrex search --window --verify-windows`) —
not collected by pytest.  One MI355X.  The yardstick is the written-out route, never the new kernel against itself.

  (a) kernels: windows of the §17(b) shape — `--records` chimeric records of `--letters` letters (a third from one bin, a third
      random, a third from another bin), W = 120, S = 30, E = 4, `--bins` peptide bins of 20 000 residues in ten records; the
      pairs are the windows that lie in a planted third against its bin, a run of about 30 consecutive windows per (record,
      bin) — through txq_edit_windows_device at TXQ_EDIT_WINDOWS_BUNDLE = 1, 2 and 4 and unset, against the same windows written out as
      patterns through txq_edit_search_device.  All variants are timed in one process, in interleaved rounds, with device
      events around each call; the figure of a variant is its best of `--reps` rounds.  The results must be equal.  The bytes
      that go up for the patterns on either route are recorded.
  (b) the command: `tetrex search --window 120 --step 30 -e 4` on `--cli-records` such records against a 1024-bin flat peptide
      index: the filter alone, --verify-windows (as it comes, and with TXQ_EDIT_WINDOWS_BUNDLE=2: a call per bin is too small to
      walk bundled by default), and --verify-windows with TETREX_VERIFY_WINDOWS=written; best wall time of
      `--reps` interleaved runs, and the rows before and after verification.

    python tests/perf_search_verify_windows.py [--records 400] [--bins 64] [--reps 5] [--no-kernels] [--no-cli]
                                               [--out profiles/search_verify_windows.json]
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
RESIDUES, RECORD = 20000, 2000


def chimeras(rng, seqs, n, letters):
    """n records: a third of bin x, random letters, a third of bin y; returns [(x, y, bytes)]"""
    third = letters // 3
    out = []
    for _ in range(n):
        x, y = (int(v) for v in rng.choice(len(seqs), size=2, replace=False))
        ax, ay = int(rng.integers(0, RESIDUES // RECORD)) * RECORD, int(rng.integers(0, RESIDUES // RECORD)) * RECORD
        mid = AA[rng.integers(0, 20, size=letters - 2 * third)].tobytes()
        out.append((x, y, seqs[x][ax:ax + third] + mid + seqs[y][ay:ay + third]))
    return out


def kernels(a, res):
    import torch
    from tetrex_amd import capi
    import edit_ref as E
    rng = np.random.default_rng(19)
    W, S, cap = a.window, a.window_step, a.errors
    seqs = [AA[rng.integers(0, 20, size=RESIDUES)].tobytes() for _ in range(a.bins)]
    recs = chimeras(rng, seqs, a.records, a.letters)
    third = a.letters // 3
    letters = b"".join(r for _, _, r in recs)
    win_begin, win_len, pairs = [], [], []
    for q, (x, y, _) in enumerate(recs):
        for at in range(0, a.letters - W + 1, S):
            for lo, hi, b in ((0, third, x), (a.letters - third, a.letters, y)):
                if at >= lo and at + W <= hi:
                    pairs.append((len(win_begin), b, cap))
                    win_begin.append(q * a.letters + at)
                    win_len.append(W)
    n = len(pairs)
    text = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    rec_off = np.arange(0, a.bins * RESIDUES + 1, RECORD, dtype=np.uint64)
    grp_off = np.arange(0, a.bins * (RESIDUES // RECORD) + 1, RESIDUES // RECORD, dtype=np.uint64)
    let = np.frombuffer(letters, dtype=np.uint8)
    wb, wl = np.array(win_begin, dtype=np.uint64), np.array(win_len, dtype=np.uint32)
    written = np.concatenate([let[b:b + W] for b in win_begin])
    pat_off = np.arange(n + 1, dtype=np.uint64) * np.uint64(W)
    pr = np.array(pairs, dtype=np.uint32)
    codes = E.letter_codes("ABCDEFGHIJKLMNOPQRSTUVWXYZ")
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()
    d_let, d_wb, d_wl, d_written, d_po, d_text, d_rec, d_grp, d_pr, d_codes = (dev(x) for x in (let, wb, wl, written, pat_off, text, rec_off, grp_off, pr, codes))
    out_w = torch.zeros(n * 12, dtype=torch.uint8, device="cuda")
    out_b = torch.zeros(n * 12, dtype=torch.uint8, device="cuda")
    work = torch.empty(max(capi.edit_windows_workspace_bytes(n), capi.edit_workspace_bytes(n)) // 8, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    L = capi.lib()

    def baseline():
        capi.check(L.txq_edit_search_device(d_written.data_ptr(), d_po.data_ptr(), n, written.size, d_text.data_ptr(), d_rec.data_ptr(), rec_off.size - 1, text.size,
                                            d_grp.data_ptr(), a.bins, d_pr.data_ptr(), n, d_codes.data_ptr(), out_b.data_ptr(), work.data_ptr(), stream))

    def windows(bundle):
        os.environ.pop("TXQ_EDIT_WINDOWS_BUNDLE", None)
        if bundle:
            os.environ["TXQ_EDIT_WINDOWS_BUNDLE"] = str(bundle)
        capi.check(L.txq_edit_windows_device(d_let.data_ptr(), let.size, d_wb.data_ptr(), d_wl.data_ptr(), n, d_text.data_ptr(), d_rec.data_ptr(), rec_off.size - 1,
                                             text.size, d_grp.data_ptr(), a.bins, d_pr.data_ptr(), n, d_codes.data_ptr(), out_w.data_ptr(), work.data_ptr(), stream))
    variants = {"written_out": baseline, "bundle1": lambda: windows(1), "bundle2": lambda: windows(2), "bundle4": lambda: windows(4), "default": lambda: windows(None)}
    for name, fn in variants.items():  # warm-up, and the routes must agree
        fn()
        torch.cuda.synchronize()
        if name != "written_out" and not torch.equal(out_w, out_b):
            raise RuntimeError("%s: results differ from txq_edit_search_device's" % name)
        out_w.zero_()
    best, every = {}, {}
    for _ in range(a.reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            best[name] = min(best.get(name, ms), ms)
            every.setdefault(name, []).append(round(ms, 3))
    os.environ.pop("TXQ_EDIT_WINDOWS_BUNDLE", None)
    got = out_b.cpu().numpy().view(np.uint32).reshape(-1, 3)
    res["kernels"] = dict(bins=a.bins, residues_per_bin=RESIDUES, records=a.records, letters=a.letters, window=W, step=S, errors=cap, pairs=n,
                          pairs_per_run=n / (2 * a.records), confirmed_fraction=float((got[:, 0] != 0xFFFFFFFF).mean()),
                          timing="device events around each call, best of %d interleaved rounds in one process" % a.reps,
                          ms=best, all_ms=every, time_ratio_to_written_out={k: v / best["written_out"] for k, v in best.items()},
                          pattern_upload_bytes=dict(written_out=int(written.size + pat_off.size * 8), windows=int(let.size + wb.size * 8 + wl.size * 4)),
                          results_equal=True)


def command(a, res):
    rng = np.random.default_rng(5)
    bins, k = 1024, 6
    with tempfile.TemporaryDirectory() as d:
        files, seqs = [], []
        for b in range(bins):
            seq = AA[rng.integers(0, 20, size=RESIDUES)].tobytes()
            p = os.path.join(d, "bin%04d.fa" % b)
            with open(p, "wb") as f:
                f.write(b"".join(b">b%d_%d\n%s\n" % (b, i, seq[i:i + RECORD]) for i in range(0, RESIDUES, RECORD)))
            files.append(p)
            seqs.append(seq)
        recs = chimeras(rng, seqs, a.cli_records, a.letters)
        qpath = os.path.join(d, "chimeras.fa")
        with open(qpath, "wb") as f:
            f.write(b"".join(b">c%d_b%d_b%d\n%s\n" % (q, x, y, s) for q, (x, y, s) in enumerate(recs)))
        lst = os.path.join(d, "bins.lst")
        with open(lst, "w") as f:
            f.write("\n".join(files) + "\n")
        r = subprocess.run([TETREX, "index", "-k", str(k), "-i", os.path.join(d, "flat"), lst], capture_output=True, text=True, timeout=1800)
        if r.returncode != 0:
            raise RuntimeError(r.stderr)
        index = os.path.join(d, "flat.ibf")
        base = [TETREX, "search", "--window", str(a.window), "--step", str(a.window_step), "-e", str(a.errors), "-v"]
        legs = {"filter_only": (base + [index, qpath], {}),
                "verify_windows": (base + ["--verify-windows", index, qpath], {}),
                "verify_windows_bundle2": (base + ["--verify-windows", index, qpath], {"TXQ_EDIT_WINDOWS_BUNDLE": "2"}),
                "verify_windows_written_out": (base + ["--verify-windows", index, qpath], {"TETREX_VERIFY_WINDOWS": "written"})}
        out = res["command"] = dict(bins=bins, residues_per_bin=RESIDUES, k=k, records=a.cli_records, letters=a.letters, window=a.window, step=a.window_step,
                                    errors=a.errors, timing="wall time of the process, best of %d interleaved runs after one warm-up run each" % a.reps, legs={})
        outputs = {}
        for rep in range(a.reps + 1):
            for name, (cmd, env) in legs.items():
                t = time.perf_counter()
                cp = subprocess.run(cmd, capture_output=True, text=True, timeout=1800, env=dict(os.environ, TETREX_TRACE="1", **env))
                wall = time.perf_counter() - t
                if cp.returncode != 0:
                    raise RuntimeError(cp.stderr)
                outputs[name] = cp.stdout
                if rep == 0:
                    notes = [l for l in cp.stderr.splitlines() if l.startswith(("Windows:", "Verified:")) or "verify routes" in l]
                    out["legs"][name] = dict(rows=len(cp.stdout.splitlines()), notes=notes)
                    continue
                e = out["legs"][name]
                e["wall_s"] = min(e.get("wall_s", wall), wall)
                e.setdefault("all_wall_s", []).append(round(wall, 3))
                e["search_time_s"] = min(e.get("search_time_s", 1e9), float(cp.stderr.split("Search time:")[1].split()[0]))
        out["routes_rows_equal"] = outputs["verify_windows"] == outputs["verify_windows_written_out"]
        found = {tuple(line.split("\t")[:2]) for line in outputs["verify_windows"].splitlines()}
        both = sum((("c%d_b%d_b%d" % (q, x, y)), os.path.abspath(files[x])) in found and (("c%d_b%d_b%d" % (q, x, y)), os.path.abspath(files[y])) in found
                   for q, (x, y, _) in enumerate(recs))
        out["verified_both_bins_reported"] = both / a.cli_records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=400, help="chimeric records of the kernel measurement (a)")
    ap.add_argument("--bins", type=int, default=64, help="bins of the kernel measurement (a)")
    ap.add_argument("--cli-records", type=int, default=2000)
    ap.add_argument("--letters", type=int, default=3000)
    ap.add_argument("--window", type=int, default=120)
    ap.add_argument("--window-step", type=int, default=30)
    ap.add_argument("--errors", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
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
