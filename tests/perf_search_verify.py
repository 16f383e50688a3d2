"""Measurement of `tetrex search --verify` (txq_edit_search_device) — not collected by pytest.  The library,
the flat index and the 10 000 query proteins of tests/perf_search.py (1024 peptide bins of 200 000 residues, k = 6; proteins
of 300 residues with 3 % substitutions), run as `search -e 9 --verify`.  Reports:
  * the candidate pairs of `search -e 9` as ONE batch on the device (the candidate bins' records in HBM, median of `--reps`
    timed calls after a warm-up) against txh_edit_search on the same pairs with 1 and with 16 host threads, in the same
    session; identical results are required;
  * the wall time of the whole command with and without --verify, and how many candidate pairs are confirmed.
The host is the yardstick, not the code under test.

    python tests/perf_search_verify.py [--bins 1024] [--residues 200000] [--queries 10000] [--reps 5] [--host-pairs N]
                                       [--out profiles/search_verify.json]
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
import perf_search as P  # noqa: E402


def cli(*args):
    t = time.perf_counter()
    r = subprocess.run([P.TETREX, *args], capture_output=True, text=True, timeout=3600)
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    return time.perf_counter() - t, r.stdout, r.stderr


def note(*what):
    print("[perf_search_verify]", *what, file=sys.stderr, flush=True)


def device_name():
    """what the HIP runtime calls device 0 (through torch, which the project already uses for plumbing)"""
    import torch
    p = torch.cuda.get_device_properties(0)
    return "%s (%s)" % (p.name, getattr(p, "gcnArchName", "?"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--residues", type=int, default=200_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--errors", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-pairs", type=int, default=0, help="time the host on the first N pairs only (0: all) and scale")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_verify.json"))
    a = ap.parse_args()
    from tetrex_amd import capi, host
    capi.init(0)
    res = dict(device=device_name(), bins=a.bins, residues_per_bin=a.residues, k=6, queries=a.queries, query_length=a.length, substitutions=0.03, errors=a.errors,
               timing="device: median of %d calls after one warm-up, host clock around call + synchronize" % a.reps)
    with tempfile.TemporaryDirectory() as d:
        files, seqs = P.library(d, a.bins, a.residues, 1)
        qpath, qs = P.queries(d, seqs, a.queries, a.length, 0.03, 2)
        note("library and queries written")
        res["index"] = P.build(d, "flat", files, ["-i"])
        note("index built")
        path = os.path.join(d, "flat.ibf")
        plain_s, plain_out, _ = cli("search", "-e", str(a.errors), path, qpath)
        verify_s, verify_out, verify_err = cli("search", "-e", str(a.errors), "--verify", "-v", path, qpath)
        note("both commands ran: %.1f s and %.1f s" % (plain_s, verify_s))
        plain_rows = [l.split("\t") for l in plain_out.splitlines()]
        verify_rows = [l.split("\t") for l in verify_out.splitlines()]
        res["cli"] = dict(search_wall_s=plain_s, search_verify_wall_s=verify_s, candidate_pairs=len(plain_rows), confirmed_pairs=len(verify_rows),
                          verified_line=[l for l in verify_err.splitlines() if l.startswith("Verified:")])
        # the same pairs as one batch: patterns = the queries, one group per candidate bin
        q_of = {n: i for i, (n, _, _) in enumerate(qs)}
        b_of = {os.path.abspath(f): b for b, f in enumerate(files)}
        cand = sorted({b_of[os.path.abspath(r[1])] for r in plain_rows})
        g_of = {b: g for g, b in enumerate(cand)}
        records, groups = [], [0]
        for b in cand:
            records += [seqs[b][i:i + 400] for i in range(0, len(seqs[b]), 400)]
            groups.append(len(records))
        pairs = np.array([(q_of[r[0]], g_of[b_of[os.path.abspath(r[1])]], a.errors) for r in plain_rows], dtype=np.uint32)
        codes = np.full(256, 255, dtype=np.uint8)
        for c in range(26):
            codes[65 + c] = codes[97 + c] = c
        pat, po, txt, ro, go, pr, cd = capi.edit_arrays([s for _, _, s in qs], records, groups, pairs, codes)
        bufs = [capi.DeviceBuffer.from_numpy(x) for x in (pat, po, txt, ro, go, pr, cd)]
        out = capi.DeviceBuffer(pr.shape[0] * 12)
        work = capi.DeviceBuffer(capi.edit_workspace_bytes(pr.shape[0]))

        def run():
            capi.check(capi.lib().txq_edit_search_device(bufs[0].ptr, bufs[1].ptr, po.size - 1, pat.size, bufs[2].ptr, bufs[3].ptr, ro.size - 1,
                                                          txt.size, bufs[4].ptr, go.size - 1, bufs[5].ptr, pr.shape[0], bufs[6].ptr, out.ptr, work.ptr, None))
        note("batch of %d pairs over %d bins uploaded" % (pr.shape[0], len(cand)))
        dev_s = P.timed(capi, run, a.reps)
        note("device batch: %.4f s" % dev_s)
        got = out.to_numpy(np.uint32, (pr.shape[0], 3))
        cells = float(sum(len(qs[p][2]) * (int(ro[go[g + 1]]) - int(ro[go[g]])) for p, g, _ in pr))
        res["batch"] = dict(pairs=int(pr.shape[0]), text_bytes=int(txt.size), candidate_bins=len(cand), dp_cells=cells,
                            device_seconds=dev_s, device_cells_per_s=cells / dev_s)
        n_host = a.host_pairs or pr.shape[0]
        for threads in (1, 16):
            t = time.perf_counter()
            want = host.edit_search((pat, po), (txt, ro), go, pr[:n_host], cd, threads=threads)
            s = (time.perf_counter() - t) * pr.shape[0] / n_host
            res["batch"]["host_seconds_%d_threads" % threads] = s
            note("host, %d thread(s): %.2f s (scaled from %d pairs)" % (threads, s, n_host))
            if not np.array_equal(got[:n_host], want):
                raise SystemExit("device and host results differ")
        res["batch"]["host_pairs_timed"] = int(n_host)
        res["batch"]["device_speedup_over_16_host_threads"] = res["batch"]["host_seconds_16_threads"] / dev_s
        res["batch"]["confirmed"] = int((got[:, 0] != 0xFFFFFFFF).sum())
        for b in bufs + [out, work]:
            b.free()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
