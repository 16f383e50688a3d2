"""Measurement of `tetrex search --translate --frame-window --verify-frame-windows` (txq_frame_window_letters) —
not collected by pytest.  One MI355X.

  (a) the new call: txq_frame_window_letters_device against txq_translate_windows_device alone on the same bytes (§18(a)'s two
      inputs: `--reads` reads of `--read-length` nt, and one contig of `--contig` nt), and txq_translate_frames_device for
      scale; in one process, interleaved rounds with device events around each call, best of `--reps` with all rounds kept.
  (b) the command on §18(c)'s workload — `--records` contigs of `--letters` nt (random nucleotides around a back-translated
      stretch of one bin and the reverse complement of a stretch of another) against a 1024-bin flat peptide index — with
      the new flag, and with `--parent DIR` (a build of the parent commit: DIR/bin/tetrex) `--frame-window` alone from that
      build, interleaved: rows, windows searched, candidate and confirmed windows, wall time of every run.  On the first
      `--ab-records` contigs alone (the plain threshold makes a candidate of nearly every window of a wrong frame) the new
      flag once more next to TETREX_FRAME_WINDOW_THRESHOLD=plain and TETREX_VERIFY_FRAME_WINDOWS=written.  The profile also
      holds, as "command_ab_all_records", the command part of a second run with --no-kernels --reps 3 --ab-records 2000.

    python tests/perf_search_verify_frame_windows.py [--reps 5] [--no-kernels] [--no-cli] [--parent DIR]
                                                     [--out profiles/search_verify_frame_windows.json]
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
from perf_search_frame_window import AA, NT, CODON_OF, COMPLEMENT  # noqa: E402

TETREX = os.path.join(ROOT, "bin", "tetrex")


def timed(torch, variants, reps):
    runs = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            runs[name].append(e0.elapsed_time(e1))
    return runs


def kernels(a, res):
    import torch
    from tetrex_amd import capi, host
    L = capi.lib()
    k, W, S, E = 6, a.window, a.window_step, a.errors
    rng = np.random.default_rng(11)
    stream = torch.cuda.current_stream().cuda_stream
    dev = lambda x: torch.from_numpy(x).cuda()
    codes = dev(np.ascontiguousarray(host.peptide_codes(0), dtype=np.uint8))
    out = res["letters"] = dict(k=k, window=W, step=S, errors=E, inputs={},
                                timing="device events around each call, %d interleaved rounds in one process, best and all rounds" % a.reps)
    for name, n, length in (("reads", a.reads, a.read_length), ("contig", 1, a.contig)):
        seq = NT[rng.integers(0, 4, size=n * length)]
        rec = (np.arange(n + 1, dtype=np.uint64) * np.uint64(length))
        bound, n_win, fbytes = capi.translate_bound(rec, k), capi.translate_windows_bound(rec, k, W, S), capi.translate_frames_bound(rec)
        d_seq, d_rec = dev(np.concatenate([seq, np.zeros(16, dtype=np.uint8)])), dev(rec.view(np.int64))
        i64 = lambda m: torch.zeros(m, dtype=torch.int64, device="cuda")
        i32 = lambda m: torch.zeros(m, dtype=torch.int32, device="cuda")
        val, off, woff, beg, ln = i64(bound + 1), i64(6 * n + 1), i64(6 * n + 1), i64(n_win + 1), i32(n_win + 2)
        frames, foff = torch.zeros(fbytes + 16, dtype=torch.uint8, device="cuda"), i64(6 * n + 1)
        lbeg, llen, stops, thr = i64(n_win + 1), i32(n_win + 2), i32(n_win + 2), i32(n_win + 2)
        variants = {
            "translate_windows": lambda: capi.check(L.txq_translate_windows_device(d_seq.data_ptr(), d_rec.data_ptr(), n, k, codes.data_ptr(), W, S, val.data_ptr(),
                                                                                   off.data_ptr(), woff.data_ptr(), beg.data_ptr(), ln.data_ptr(), stream)),
            "translate_frames": lambda: capi.check(L.txq_translate_frames_device(d_seq.data_ptr(), d_rec.data_ptr(), n, frames.data_ptr(), fbytes, foff.data_ptr(),
                                                                                 stream)),
            "frame_window_letters": lambda: capi.check(L.txq_frame_window_letters_device(d_rec.data_ptr(), n, k, W, S, frames.data_ptr(), fbytes, foff.data_ptr(),
                                                                                         woff.data_ptr(), ln.data_ptr(), n_win, E, lbeg.data_ptr(), llen.data_ptr(),
                                                                                         stops.data_ptr(), thr.data_ptr(), stream)),
        }
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        # the stops against a prefix count over the frames as the device wrote them
        letters = frames[:fbytes].cpu().numpy()
        pref = np.concatenate([[0], np.cumsum(letters == ord("*"))])
        b, l = lbeg[:n_win].cpu().numpy(), llen[:n_win].cpu().numpy().astype(np.int64)
        if not np.array_equal(pref[b + l] - pref[b], stops[:n_win].cpu().numpy()):
            raise RuntimeError("%s: the stops differ from a prefix count" % name)
        runs = timed(torch, variants, a.reps)
        t = thr[:n_win].cpu().numpy().view(np.uint32)
        plain = np.maximum(ln[:n_win].cpu().numpy().astype(np.int64) - k * E, 0)
        out["inputs"][name] = dict(records=n, length=length, windows=n_win, frames_bytes=fbytes, searched=int((t != 0xFFFFFFFF).sum()),
                                   searched_by_the_plain_threshold=int((plain > 0).sum()),
                                   ms={v: dict(best=min(r), runs=r) for v, r in runs.items()},
                                   letters_over_translate_windows=min(runs["frame_window_letters"]) / min(runs["translate_windows"]))


def command(a, res):
    rng = np.random.default_rng(5)
    bins, residues, k, stretch = 1024, 20000, 6, 300
    with tempfile.TemporaryDirectory() as d:
        files, seqs = [], []
        for b in range(bins):
            seq = AA[rng.integers(0, 20, size=residues)].tobytes()
            p = os.path.join(d, "bin%04d.fa" % b)
            with open(p, "wb") as f:
                f.write(b"".join(b">b%d_%d\n%s\n" % (b, i, seq[i:i + 2000]) for i in range(0, residues, 2000)))
            files.append(p)
            seqs.append(seq)
        back = lambda pep: "".join(CODON_OF[c] for c in pep.decode()).encode()
        flank = (a.letters - 6 * stretch) // 3
        recs = []
        for q in range(a.records):
            x, y = (int(v) for v in rng.choice(bins, size=2, replace=False))
            ax, ay = int(rng.integers(0, residues - stretch)), int(rng.integers(0, residues - stretch))
            parts = [NT[rng.integers(0, 4, size=flank + int(rng.integers(0, 3)))].tobytes(), back(seqs[x][ax:ax + stretch]),
                     NT[rng.integers(0, 4, size=flank)].tobytes(), back(seqs[y][ay:ay + stretch]).translate(COMPLEMENT)[::-1],
                     NT[rng.integers(0, 4, size=flank)].tobytes()]
            recs.append(b">c%d_b%d_b%d\n%s\n" % (q, x, y, b"".join(parts)))
        qpath, abpath = os.path.join(d, "contigs.fa"), os.path.join(d, "contigs_ab.fa")
        with open(qpath, "wb") as f:
            f.write(b"".join(recs))
        with open(abpath, "wb") as f:
            f.write(b"".join(recs[:a.ab_records]))
        lst = os.path.join(d, "bins.lst")
        with open(lst, "w") as f:
            f.write("\n".join(files) + "\n")
        r = subprocess.run([TETREX, "index", "-k", str(k), "-i", os.path.join(d, "flat"), lst], capture_output=True, text=True, timeout=1800)
        if r.returncode != 0:
            raise RuntimeError(r.stderr)
        index = os.path.join(d, "flat.ibf")
        flags = ["search", "--translate", "--frame-window", str(a.window), "--frame-step", str(a.window_step), "-e", str(a.errors)]
        legs = {"verify_frame_windows": ([TETREX] + flags + ["--verify-frame-windows", "-v", index, qpath], {})}
        if a.parent:
            legs["frame_window_parent_build"] = ([os.path.join(a.parent, "bin", "tetrex")] + flags + ["-v", index, qpath], {})
        ab = [TETREX] + flags + ["--verify-frame-windows", "-v", index, abpath]
        legs["ab_verify_frame_windows"] = (ab, {})
        legs["ab_threshold_plain"] = (ab, {"TETREX_FRAME_WINDOW_THRESHOLD": "plain"})
        legs["ab_written"] = (ab, {"TETREX_VERIFY_FRAME_WINDOWS": "written"})
        out = res["command"] = dict(bins=bins, residues_per_bin=residues, k=k, records=a.records, ab_records=a.ab_records, letters=a.letters,
                                    planted_residues=stretch, window=a.window, step=a.window_step, errors=a.errors,
                                    timing="wall time of the process, %d interleaved runs after one warm-up run each, best and all runs" % a.reps, legs={})
        outputs = {}
        for rep in range(a.reps + 1):
            for name, (cmd, env) in legs.items():
                t = time.perf_counter()
                cp = subprocess.run(cmd, capture_output=True, text=True, timeout=1800, env=dict(os.environ, **env))
                wall = time.perf_counter() - t
                if cp.returncode != 0:
                    raise RuntimeError(cp.stderr)
                if rep == 0:
                    outputs[name] = cp.stdout
                    e = out["legs"][name] = dict(rows=len(cp.stdout.splitlines()), wall_s=[], search_time_s=[])
                    m = re.search(r"Windows: (\d+) searched, (\d+) hit, (\d+) rows", cp.stderr)
                    e["windows_searched"], e["windows_hit"] = int(m.group(1)), int(m.group(2))
                    m = re.search(r"Verified: (\d+) of (\d+) candidate windows", cp.stderr)
                    if m:
                        e["confirmed_windows"], e["candidate_windows"] = int(m.group(1)), int(m.group(2))
                    continue
                e = out["legs"][name]
                e["wall_s"].append(wall)
                e["search_time_s"].append(float(cp.stderr.split("Search time:")[1].split()[0]))
        for e in out["legs"].values():
            e["best_wall_s"], e["best_search_time_s"] = min(e["wall_s"]), min(e["search_time_s"])
        out["ab_rows_equal"] = outputs["ab_verify_frame_windows"] == outputs["ab_threshold_plain"] == outputs["ab_written"]
        # the claim about rows: both planted bins of every contig reported in their frames, and nothing else
        rows = [line.split("\t") for line in outputs["verify_frame_windows"].splitlines()]
        found = {(r[0], r[1]) for r in rows}
        both = planted_rows = 0
        for q in range(a.records):
            name = recs[q].split(b"\n")[0][1:].decode()
            x, y = (os.path.abspath(files[int(s[1:])]) for s in name.split("_")[1:])
            both += (name, x) in found and (name, y) in found
            planted_rows += sum(1 for r in rows if r[0] == name and r[1] in (x, y))
        out["both_bins_reported"] = both / a.records
        out["rows_of_planted_bins"] = planted_rows
        out["rows_of_other_bins"] = len(rows) - planted_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reads", type=int, default=10_000)
    ap.add_argument("--read-length", type=int, default=900)
    ap.add_argument("--contig", type=int, default=1_000_000)
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--ab-records", type=int, default=100)
    ap.add_argument("--letters", type=int, default=9000)
    ap.add_argument("--window", type=int, default=40, help="residues of a window")
    ap.add_argument("--window-step", type=int, default=10)
    ap.add_argument("--errors", type=int, default=2)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--parent", default=None, help="a build of the parent commit (DIR/bin/tetrex) for --frame-window alone")
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
