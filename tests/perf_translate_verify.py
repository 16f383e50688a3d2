"""Measurement of `tetrex search --translate --verify-frames` (txq_translate_frames_device) — not collected by
pytest.  The index and the reads are tests/perf_translate.py's: 1024 peptide bins of 200 000 residues at k = 6, flat (-i);
10 000 reads of 900 nt, back-translated from 300-residue pieces of the library's proteins with 3 % residue substitutions,
every other one reverse-complemented; `-e 9`.  Reports:
  (a) txq_translate_frames_device for the whole batch: median of `--reps` calls after a warm-up, waiting for the stream,
      its bytes in and out; against the yardstick, translate_frame (txh_translate_frame) over the same 60 000 frames on one
      host thread plus the upload of the letters and their offsets.  The host loop is driven from Python, so the cost of
      60 000 calls that translate nothing is measured and reported next to it.  Identical bytes are required.
  (b) the wall time of the whole command, best of `--reps` and the spread (max - min), the three variants interleaved:
      by default (the frames translated on the device), with TETREX_VERIFY_FRAMES=host (translate_frame on the host, the
      patterns uploaded as strings), and `--translate -e 9` without verification.  Identical rows are required of the first
      two, and every read's source bin and frame must be among them.
The yardsticks are the host route and the unverified command in the same session, not the code under test.

    python tests/perf_translate_verify.py [--bins 1024] [--residues 200000] [--reads 10000] [--reps 5]
                                          [--out profiles/search_translate_verify.json]
"""
import argparse
import ctypes as C
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

from perf_search import TETREX, build, library, queries, timed  # noqa: E402
from perf_translate import back_translate  # noqa: E402
import translate_ref as T  # noqa: E402


def note(*what):
    print("[perf_translate_verify]", *what, file=sys.stderr, flush=True)


def cli(args, env=None):
    t = time.perf_counter()
    r = subprocess.run([TETREX, *args], capture_output=True, text=True, timeout=3600, env=dict(os.environ, **(env or {})))
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    return time.perf_counter() - t, r.stdout, r.stderr


def host_frames(host, raw, empty=False):
    """txh_translate_frame on every frame of every read, one thread, one output buffer; (letters, offsets, seconds)"""
    L = host.lib()
    L.txh_translate_frame.restype = C.c_int64
    L.txh_translate_frame.argtypes = [C.c_char_p, C.c_size_t, C.c_uint, C.c_void_p, C.c_size_t]
    cap = sum(2 * len(s) for s in raw) + 8
    letters = np.zeros(cap, dtype=np.uint8)
    offsets = np.zeros(6 * len(raw) + 1, dtype=np.uint64)
    t = time.perf_counter()
    at = 0
    for r, s in enumerate(raw):
        for f in range(6):
            n = L.txh_translate_frame(s, 0 if empty else len(s), f, letters.ctypes.data + at, cap - at)
            at += n
            offsets[6 * r + f + 1] = at
    return letters[:at], offsets, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--residues", type=int, default=200_000)
    ap.add_argument("--reads", type=int, default=10_000)
    ap.add_argument("--errors", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_translate_verify.json"))
    a = ap.parse_args()
    from tetrex_amd import capi, host
    capi.init(0)
    Lq = capi.lib()
    res = dict(bins=a.bins, residues_per_bin=a.residues, k=6, reads=a.reads, read_length=900, substitutions=0.03, errors=a.errors, measured_on="MI355X",
               timing="kernel: median of %d calls after one warm-up, host clock around call + synchronize; command: wall time of the "
                      "process, best of %d, the variants interleaved" % (a.reps, a.reps))
    with tempfile.TemporaryDirectory() as d:
        files, seqs = library(d, a.bins, a.residues, 1)
        _, peptides = queries(d, seqs, a.reads, 300, 0.03, 2)
        reads = back_translate(peptides, 3)
        qpath = os.path.join(d, "reads.fa")
        with open(qpath, "w") as f:
            f.write("".join(">%s\n%s\n" % (n, s) for n, _, _, s in reads))
        note("library and reads written")
        # (a) the kernel against translate_frame on the host plus the upload
        raw = [s.encode() for _, _, _, s in reads]
        seq, rec = capi._records(raw)
        nq = 6 * len(reads)
        bound = capi.translate_frames_bound(rec)
        d_seq, d_rec = capi.DeviceBuffer.from_numpy(seq), capi.DeviceBuffer.from_numpy(rec)
        d_frames, d_off = capi.DeviceBuffer(bound + 16), capi.DeviceBuffer(8 * (nq + 1))

        def translate():
            capi.check(Lq.txq_translate_frames_device(d_seq.ptr, d_rec.ptr, len(reads), d_frames.ptr, bound, d_off.ptr, None))
        dev_s = timed(capi, translate, a.reps)
        got, got_o = d_frames.to_numpy(np.uint8, (bound,)), d_off.to_numpy(np.uint64, (nq + 1,))
        host_runs, want, want_o = [], None, None
        for _ in range(a.reps):
            want, want_o, s = host_frames(host, raw)
            t = time.perf_counter()
            capi.check(Lq.txq_memcpy_h2d(d_frames.ptr, want.ctypes.data, want.nbytes))
            capi.check(Lq.txq_memcpy_h2d(d_off.ptr, want_o.ctypes.data, want_o.nbytes))
            capi.synchronize()
            host_runs.append((s, time.perf_counter() - t))
        empty_s = float(np.median([host_frames(host, raw, empty=True)[2] for _ in range(a.reps)]))
        if not (np.array_equal(got_o, want_o) and np.array_equal(got, want)):
            raise SystemExit("device and host frames differ")
        if T.translate_frame(reads[1][3], 4).encode() != want[int(want_o[10]):int(want_o[11])].tobytes():
            raise SystemExit("host frames differ from the restatement")
        hs, us = float(np.median([x for x, _ in host_runs])), float(np.median([y for _, y in host_runs]))
        res["kernel"] = dict(frames=nq, frame_bytes=bound, input_bytes=int(seq.nbytes + rec.nbytes), output_bytes=int(bound + 8 * (nq + 1)),
                             device_seconds=dev_s, device_output_bytes_per_s=(bound + 8 * (nq + 1)) / dev_s,
                             host_translate_one_thread_s=hs, host_calls_that_translate_nothing_s=empty_s, host_upload_s=us,
                             host_total_s=hs + us, identical_bytes=True)
        note("kernel: %.6f s; host %.4f s (+ upload %.4f s; %.4f s of the host time is the cost of the calls)" % (dev_s, hs, us, empty_s))
        for b in (d_seq, d_rec, d_frames, d_off):
            b.free()
        # (b) the command
        res["index"] = build(d, "flat", files, ["-i"])
        note("index built")
        path = os.path.join(d, "flat.ibf")
        base = ["search", "--translate", "-e", str(a.errors)]
        variants = (("device", ["--verify-frames", "-v"], {}), ("host", ["--verify-frames", "-v"], {"TETREX_VERIFY_FRAMES": "host"}), ("unverified", [], {}))
        runs = {v: [] for v, _, _ in variants}
        outs = {}
        for rep in range(a.reps):
            for v, flags, env in variants:  # (interleaved: drift hits all alike)
                s, so, se = cli(base + flags + [path, qpath], dict(env, TETREX_TRACE="1"))
                runs[v].append(s)
                outs[v] = (so, [l for l in se.splitlines() if l.startswith("Verified:") or "verify routes" in l])
        if outs["device"][0] != outs["host"][0]:
            raise SystemExit("the two routes print different rows")
        rows = {tuple(l.split("\t")[:3]) for l in outs["device"][0].splitlines()}
        res["command"] = dict(candidate_rows=len(outs["unverified"][0].splitlines()), confirmed_rows=len(outs["device"][0].splitlines()),
                              source_bin_and_frame_confirmed=float(np.mean([(n, os.path.abspath(files[b]), T.FRAMES[f]) in rows for n, b, f, _ in reads])),
                              **{"%s_%s" % (v, key): val for v, ts in runs.items()
                                 for key, val in (("best_s", min(ts)), ("spread_s", max(ts) - min(ts)), ("runs_s", ts), ("stderr", outs[v][1]))})
        c = res["command"]
        slack = max(c["device_spread_s"], c["host_spread_s"])
        c["decision"] = ("device route stays the default" if c["device_best_s"] <= c["host_best_s"] + slack else "host route should be the default")
        note("command: device %.2f s (spread %.2f), host %.2f s (spread %.2f), unverified %.2f s (spread %.2f): %s" %
             (c["device_best_s"], c["device_spread_s"], c["host_best_s"], c["host_spread_s"], c["unverified_best_s"], c["unverified_spread_s"], c["decision"]))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
