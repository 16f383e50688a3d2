"""Measurement of `tetrex search --verify --all-targets` (txq_edit_targets_device) — not collected by pytest.
The library, the flat index and the query proteins of tests/perf_search_verify.py (peptide bins of 200 000 residues in records
of 400, k = 6; proteins of 300 residues with 3 % substitutions), run as `search -e 9 --verify --all-targets`.  Reports:
  * the candidate pairs of `search -e 9` as ONE batch through txq_edit_targets_device (the candidate bins' records in HBM, median
    of `--reps` timed calls after a warm-up), against
      (a) what the code could do for the same answer before this call existed: txq_edit_search_device with every record a
          group of its own, identical hits required, and how many pairs and units that takes;
      (b) txh_edit_targets on the same pairs with 1 and with 16 host threads, identical hits required;
  * the wall time of the whole command with --verify --all-targets and with --verify, best of 5 with the spread, and with
    --parent-tetrex the --verify of another build (the parent commit's) in the same session.
The host and the earlier call are the yardsticks, not the code under test.

    python tests/perf_search_targets.py [--bins 1024] [--residues 200000] [--queries 10000] [--reps 5] [--host-pairs N]
                                        [--copies C] [--parent-tetrex PATH] [--out profiles/search_targets.json]
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
import edit_targets_ref as T  # noqa: E402
from perf_search_verify import device_name  # noqa: E402


def cli(tetrex, *args):
    t = time.perf_counter()
    r = subprocess.run([tetrex, *args], capture_output=True, text=True, timeout=3600)
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    return time.perf_counter() - t, r.stdout, r.stderr


def best_of(n, tetrex, *args):
    """(best wall time, max - min, stdout, stderr) of n runs"""
    runs = [cli(tetrex, *args) for _ in range(n)]
    ts = [r[0] for r in runs]
    return min(ts), max(ts) - min(ts), runs[-1][1], runs[-1][2]


def note(*what):
    print("[perf_search_targets]", *what, file=sys.stderr, flush=True)


def library(d, bins, residues, seed, copies):
    """P.library; with copies > 1 every record of a bin stands `copies` times in a row (a family of identical members), so that
    a pair has that many hits: the flushes and the compaction under load"""
    if copies <= 1:
        return P.library(d, bins, residues, seed)
    files, seqs = P.library(d, bins, residues // copies // 400 * 400, seed)
    for b, f in enumerate(files):
        recs = [r for i in range(0, len(seqs[b]), 400) for r in [seqs[b][i:i + 400]] * copies]
        seqs[b] = b"".join(recs)
        with open(f, "wb") as out:
            out.write(b"".join(b">b%d_%d\n%s\n" % (b, i, r) for i, r in enumerate(recs)))
    return files, seqs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--residues", type=int, default=200_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--errors", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--copies", type=int, default=1, help="every record of a bin stands this many times in a row: that many hits a pair")
    ap.add_argument("--host-pairs", type=int, default=0, help="time the host on the first N pairs only (0: all) and scale")
    ap.add_argument("--parent-tetrex", default="", help="the tetrex binary of another build, for the --verify of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_targets.json"))
    a = ap.parse_args()
    from tetrex_amd import capi, host
    capi.init(0)
    res = dict(device=device_name().strip(), bins=a.bins, residues_per_bin=a.residues, record_length=400, copies=a.copies, k=6, queries=a.queries, query_length=a.length,
               substitutions=0.03, errors=a.errors,
               timing="device: median of %d calls after one warm-up, host clock around call + synchronize; commands: best of 5, spread = max - min" % a.reps)
    with tempfile.TemporaryDirectory() as d:
        files, seqs = library(d, a.bins, a.residues, 1, a.copies)
        qpath, qs = P.queries(d, seqs, a.queries, a.length, 0.03, 2)
        res["index"] = P.build(d, "flat", files, ["-i"])
        note("library, queries and index written")
        path = os.path.join(d, "flat.ibf")
        _, plain_out, _ = cli(P.TETREX, "search", "-e", str(a.errors), path, qpath)
        verify = best_of(5, P.TETREX, "search", "-e", str(a.errors), "--verify", "-v", path, qpath)
        every = best_of(5, P.TETREX, "search", "-e", str(a.errors), "--verify", "--all-targets", "-v", path, qpath)
        res["cli"] = dict(verify_wall_s=verify[0], verify_spread_s=verify[1], all_targets_wall_s=every[0], all_targets_spread_s=every[1],
                          candidate_pairs=len(plain_out.splitlines()), verify_rows=len(verify[2].splitlines()), all_targets_rows=len(every[2].splitlines()),
                          lines=[l for l in every[3].splitlines() if l.startswith(("Verified:", "Targets:"))])
        if a.parent_tetrex:
            parent = best_of(5, a.parent_tetrex, "search", "-e", str(a.errors), "--verify", "-v", path, qpath)
            res["cli"].update(parent_verify_wall_s=parent[0], parent_verify_spread_s=parent[1], parent_rows_identical=parent[2] == verify[2])
        note("commands ran:", json.dumps(res["cli"]))
        # the same pairs as one batch: patterns = the queries, one group per candidate bin
        plain_rows = [l.split("\t") for l in plain_out.splitlines()]
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
        n, n_slots = pr.shape[0], capi.edit_targets_slots(go, pr)
        bufs = [capi.DeviceBuffer.from_numpy(x) for x in (pat, po, txt, ro, go, pr, cd)]
        capacity = (2 * a.copies + 2) * n + 1024
        d_hits, d_total, d_status = capi.DeviceBuffer(16 * capacity), capi.DeviceBuffer(8), capi.DeviceBuffer(4 * n + 4)
        work = capi.DeviceBuffer(capi.edit_targets_workspace(n, n_slots))
        L = capi.lib()

        def run():
            capi.check(L.txq_edit_targets_device(bufs[0].ptr, bufs[1].ptr, po.size - 1, pat.size, bufs[2].ptr, bufs[3].ptr, ro.size - 1, txt.size, bufs[4].ptr,
                                                 go.size - 1, bufs[5].ptr, n, bufs[6].ptr, d_hits.ptr, capacity, d_total.ptr, d_status.ptr, n_slots, work.ptr, None))
        note("batch of %d pairs over %d bins, %d slots" % (n, len(cand), n_slots))
        dev_s = P.timed(capi, run, a.reps)
        total = int(d_total.to_numpy(np.uint64, (1,))[0])
        if total > capacity or d_status.to_numpy(np.uint32, (n,)).any():
            raise SystemExit("the hit list did not fit or a pair was refused")
        got = d_hits.to_numpy(np.uint32, (total, 4))
        cells = float(sum(len(qs[p][2]) * (int(ro[go[g + 1]]) - int(ro[go[g]])) for p, g, _ in pr))
        res["batch"] = dict(pairs=int(n), slots=int(n_slots), hits=total, text_bytes=int(txt.size), candidate_bins=len(cand), dp_cells=cells,
                            device_seconds=dev_s, device_cells_per_s=cells / dev_s)
        note("device batch: %.4f s, %d hits" % (dev_s, total))
        for b in (d_hits, d_total, d_status, work):
            b.free()
        # (a) the search call that was there before, every record a group of its own
        single_groups, single, owner = T.expand(groups, pr.tolist())
        sg, sp = np.asarray(single_groups, dtype=np.uint64), np.asarray(single, dtype=np.uint32)
        d_sg, d_sp = capi.DeviceBuffer.from_numpy(sg), capi.DeviceBuffer.from_numpy(sp)
        d_out, d_work = capi.DeviceBuffer(12 * sp.shape[0]), capi.DeviceBuffer(capi.edit_workspace_bytes(sp.shape[0]))

        def run_single():
            capi.check(L.txq_edit_search_device(bufs[0].ptr, bufs[1].ptr, po.size - 1, pat.size, bufs[2].ptr, bufs[3].ptr, ro.size - 1, txt.size, d_sg.ptr,
                                                sg.size - 1, d_sp.ptr, sp.shape[0], bufs[6].ptr, d_out.ptr, d_work.ptr, None))
        single_s = P.timed(capi, run_single, a.reps)
        if not np.array_equal(T.hits_of(d_out.to_numpy(np.uint32, (sp.shape[0], 3)), owner), got):
            raise SystemExit("the per-record call and the search call on one-record groups differ")
        # units of route (a), by the plan kernel's arithmetic (units_of: 64 lane chunks of TXQ_EDIT_CHUNK bytes): derived, not read back
        chunk = (min(max(int(os.environ.get("TXQ_EDIT_CHUNK") or 512), 16), 1 << 20) + 15) // 16 * 16
        rec_bytes = (ro[1:] - ro[:-1]).astype(np.int64)[sp[:, 1].astype(np.int64)]
        units = int(((rec_bytes + 64 * chunk - 1) // (64 * chunk)).sum())
        res["batch"].update(one_record_groups_seconds=single_s, one_record_groups_pairs=int(sp.shape[0]), one_record_groups_units_derived=units,
                            speedup_over_one_record_groups=single_s / dev_s)
        note("one-record groups: %.4f s for %d pairs" % (single_s, sp.shape[0]))
        # (b) the host twin
        n_host = a.host_pairs or n
        want_n = int((got[:, 0] < n_host).sum())
        for threads in (1, 16):
            t = time.perf_counter()
            want, _ = host.edit_targets((pat, po), (txt, ro), go, pr[:n_host], cd, threads=threads, capacity=capacity)
            s = (time.perf_counter() - t) * n / n_host
            res["batch"]["host_seconds_%d_threads" % threads] = s
            note("host, %d thread(s): %.2f s (scaled from %d pairs)" % (threads, s, n_host))
            if not np.array_equal(got[:want_n], want):
                raise SystemExit("device and host hits differ")
        res["batch"]["host_pairs_timed"] = int(n_host)
        res["batch"]["device_speedup_over_16_host_threads"] = res["batch"]["host_seconds_16_threads"] / dev_s
        for b in bufs + [d_sg, d_sp, d_out, d_work]:
            b.free()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
