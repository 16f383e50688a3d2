"""Measurement of `tetrex search --verify` on records of 513 .. 4096 letters (txq_edit_search_long_device, DESIGN.md §12 "Long
patterns") — not collected by pytest.  Two workloads, each a library of `--bins` bins whose records are longer than the
queries, indexed flat, and queries cut from the records with 3 % substitutions:
  peptide     the bins of tests/perf_search.py (200 000 residues each, k = 6) in records of 1200 residues; proteins of 1000
              residues, `search -e 30`
  nucleotide  bins of 200 000 letters (k = 16) in records of 4000 letters; reads of 3000 letters, `search -e 90`
Reports, per workload:
  * kernel: the candidate pairs of `search -e E` as ONE batch through txq_edit_search_long_device (median of `--reps` timed
    calls after a warm-up) against txh_edit_search on the same pairs with 1 and with 16 host threads, in the same session;
    identical results are required; pattern letters x text bytes per second for both;
  * command: the wall time of the whole `search --verify`, best of `--reps` and the spread (max - min) of the runs, by default
    and with TETREX_VERIFY_LONG=0 (the host route, which is what the command did before the kernel existed); identical
    stdout is required;
and once, on a text of `--sweep-bytes` random letters in records of 5000: the kernel's time at m = 600 and m = 3000 with
TXQ_EDIT_LONG_SPAN = 256, 1024, 4096, 16384 (`--sweep-pairs` pairs each, cap m / 33).
The host is the yardstick, not the code under test.

    python tests/perf_search_verify_long.py [--bins 1024] [--residues 200000] [--queries 2000] [--reads 500] [--reps 5] [--host-pairs N]
                                            [--out profiles/search_verify_long.json]
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

WORKLOADS = {  # name: (letters, k, index flags, record length, query length, errors)
    "peptide": (b"ACDEFGHIKLMNPQRSTVWY", 6, [], 1200, 1000, 30),
    "nucleotide": (b"ACGT", 16, ["-n"], 4000, 3000, 90),
}
SPANS = [256, 1024, 4096, 16384]


def note(*what):
    print("[perf_search_verify_long]", *what, file=sys.stderr, flush=True)


def device_name():
    """what the HIP runtime calls device 0 (through torch, which the project already uses for plumbing)"""
    import torch
    p = torch.cuda.get_device_properties(0)
    return "%s (%s)" % (p.name, getattr(p, "gcnArchName", "?"))


def library(d, letters, bins, residues, record, seed):
    rng = np.random.default_rng(seed)
    pool = np.frombuffer(letters, dtype=np.uint8)
    files, seqs = [], []
    for b in range(bins):
        seq = pool[rng.integers(0, pool.size, size=residues)].tobytes()
        recs = [seq[i:i + record] for i in range(0, len(seq), record)]
        p = os.path.join(d, "bin%04d.fa" % b)
        with open(p, "wb") as f:
            f.write(b"".join(b">b%d_%d\n%s\n" % (b, i, r) for i, r in enumerate(recs)))
        files.append(p)
        seqs.append(seq)
    return files, seqs


def queries(d, letters, seqs, n, record, length, subst, seed):
    rng = np.random.default_rng(seed)
    pool = np.frombuffer(letters, dtype=np.uint8)
    out = []
    for q in range(n):
        b = int(rng.integers(0, len(seqs)))
        rec = int(rng.integers(0, len(seqs[b]) // record))  # within one whole record of the bin
        at = rec * record + int(rng.integers(0, record - length + 1))
        s = bytearray(seqs[b][at:at + length])
        for i in rng.choice(length, size=int(round(subst * length)), replace=False):
            s[i] = pool[(np.flatnonzero(pool == s[i])[0] + 1 + int(rng.integers(0, pool.size - 1))) % pool.size]
        out.append(("q%d_b%d" % (q, b), b, bytes(s)))
    p = os.path.join(d, "queries.fa")
    with open(p, "wb") as f:
        f.write(b"".join(b">%s\n%s\n" % (n.encode(), s) for n, _, s in out))
    return p, out


def cli(args, env=None):
    t = time.perf_counter()
    r = subprocess.run([P.TETREX, *args], capture_output=True, text=True, timeout=3600, env=dict(os.environ, **(env or {})))
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    return time.perf_counter() - t, r.stdout, r.stderr


def class_table(dna):
    codes = np.full(256, 255, dtype=np.uint8)
    if dna:
        for c, x in enumerate(b"ACGT"):
            codes[x] = codes[x | 0x20] = c
    else:
        for c in range(26):
            codes[65 + c] = codes[97 + c] = c
    return codes


class Batch:
    """pairs on the device, ready for txq_edit_search_long_device"""

    def __init__(self, capi, patterns, records, groups, pairs, codes):
        self.capi = capi
        self.arrays = capi.edit_arrays(patterns, records, groups, pairs, codes)
        pat, po, txt, ro, go, pr, cd = self.arrays
        self.bufs = [capi.DeviceBuffer.from_numpy(x) for x in self.arrays]
        self.out = capi.DeviceBuffer(pr.shape[0] * 12)
        self.work = capi.DeviceBuffer(capi.edit_long_workspace(pr.shape[0]))
        self.cells = float(sum((int(po[p + 1]) - int(po[p])) * (int(ro[go[g + 1]]) - int(ro[go[g]])) for p, g, _ in pr))

    def run(self):
        pat, po, txt, ro, go, pr, cd = self.arrays
        b = self.bufs
        self.capi.check(self.capi.lib().txq_edit_search_long_device(b[0].ptr, b[1].ptr, po.size - 1, pat.size, b[2].ptr, b[3].ptr, ro.size - 1, txt.size,
                                                                    b[4].ptr, go.size - 1, b[5].ptr, pr.shape[0], b[6].ptr, self.out.ptr, self.work.ptr, None))

    def results(self):
        return self.out.to_numpy(np.uint32, (self.arrays[5].shape[0], 3))

    def free(self):
        for b in self.bufs + [self.out, self.work]:
            b.free()


def workload(name, a, capi, host):
    letters, k, flags, record, length, errors = WORKLOADS[name]
    dna = name == "nucleotide"
    n_queries = a.reads if dna else a.queries
    res = dict(bins=a.bins, letters_per_bin=a.residues, record_length=record, k=k, queries=n_queries, query_length=length, substitutions=0.03, errors=errors)
    with tempfile.TemporaryDirectory() as d:
        files, seqs = library(d, letters, a.bins, a.residues, record, 1)
        qpath, qs = queries(d, letters, seqs, n_queries, record, length, 0.03, 2)
        lst = os.path.join(d, "bins.lst")
        with open(lst, "w") as f:
            f.write("\n".join(files) + "\n")
        t = time.perf_counter()
        cli(["index", "-k", str(k), *flags, "-i", os.path.join(d, "flat"), lst])
        res["index_build_wall_s"] = time.perf_counter() - t
        note(name, "index built")
        path = os.path.join(d, "flat.ibf")
        base = ["search", "-e", str(errors)]
        plain_s, plain_out, _ = cli(base + [path, qpath])
        plain_rows = [l.split("\t") for l in plain_out.splitlines()]
        runs = {"device_long": [], "host": []}
        outs = {}
        for rep in range(a.reps):
            for route, env in (("device_long", {}), ("host", {"TETREX_VERIFY_LONG": "0"})):  # (interleaved: drift hits both alike)
                s, so, se = cli(base + ["--verify", "-v", path, qpath], dict(env, TETREX_TRACE="1"))
                runs[route].append(s)
                outs[route] = (so, [l for l in se.splitlines() if l.startswith("Verified:") or "verify routes" in l])
        if outs["device_long"][0] != outs["host"][0]:
            raise SystemExit("%s: the two routes print different rows" % name)
        res["command"] = dict(search_wall_s=plain_s, candidate_pairs=len(plain_rows), confirmed_pairs=len(outs["host"][0].splitlines()),
                              **{"%s_%s" % (route, key): val for route, ts in runs.items()
                                 for key, val in (("best_s", min(ts)), ("spread_s", max(ts) - min(ts)), ("runs_s", ts), ("stderr", outs[route][1]))})
        note(name, "command: device-long %.2f s (spread %.2f), host %.2f s (spread %.2f)" %
             (min(runs["device_long"]), max(runs["device_long"]) - min(runs["device_long"]), min(runs["host"]), max(runs["host"]) - min(runs["host"])))
        # the same pairs as one batch: patterns = the queries (the strand as given), one group per candidate bin
        q_of = {n: i for i, (n, _, _) in enumerate(qs)}
        b_of = {os.path.abspath(f): b for b, f in enumerate(files)}
        cand = sorted({b_of[os.path.abspath(r[1])] for r in plain_rows})
        g_of = {b: g for g, b in enumerate(cand)}
        records, groups = [], [0]
        for b in cand:
            records += [seqs[b][i:i + record] for i in range(0, len(seqs[b]), record)]
            groups.append(len(records))
        pairs = np.array([(q_of[r[0]], g_of[b_of[os.path.abspath(r[1])]], errors) for r in plain_rows], dtype=np.uint32)
        batch = Batch(capi, [s for _, _, s in qs], records, groups, pairs, class_table(dna))
        dev_s = P.timed(capi, batch.run, a.reps)
        got = batch.results()
        pat, po, txt, ro, go, pr, cd = batch.arrays
        k_res = res["kernel"] = dict(pairs=int(pr.shape[0]), text_bytes=int(txt.size), candidate_bins=len(cand), dp_cells=batch.cells,
                                     device_seconds=dev_s, device_cells_per_s=batch.cells / dev_s)
        note(name, "kernel: %d pairs, %.4f s" % (pr.shape[0], dev_s))
        n_host = min(a.host_pairs or pr.shape[0], pr.shape[0])
        for threads in (1, 16):
            t = time.perf_counter()
            want = host.edit_search((pat, po), (txt, ro), go, pr[:n_host], cd, threads=threads)
            s = (time.perf_counter() - t) * pr.shape[0] / n_host
            k_res["host_seconds_%d_threads" % threads] = s
            k_res["host_cells_per_s_%d_threads" % threads] = batch.cells / s
            note(name, "host, %d thread(s): %.2f s (scaled from %d pairs)" % (threads, s, n_host))
            if not np.array_equal(got[:n_host], want):
                raise SystemExit("%s: device and host results differ" % name)
        k_res["host_pairs_timed"] = int(n_host)
        k_res["device_speedup_over_16_host_threads"] = k_res["host_seconds_16_threads"] / dev_s
        k_res["confirmed"] = int((got[:, 0] != 0xFFFFFFFF).sum())
        batch.free()
    return res


def span_sweep(a, capi, host):
    rng = np.random.default_rng(9)
    pool = np.frombuffer(b"ACGT", dtype=np.uint8)
    text = pool[rng.integers(0, 4, size=a.sweep_bytes)].tobytes()
    records = [text[i:i + 5000] for i in range(0, len(text), 5000)]
    codes = class_table(True)
    out = dict(text_bytes=len(text), record_length=5000, pairs=a.sweep_pairs, rows=[])
    for m in (600, 3000):
        starts = rng.integers(0, len(records) - 1, size=a.sweep_pairs) * 5000 + rng.integers(0, 5000 - m, size=a.sweep_pairs)
        patterns = [text[int(s):int(s) + m] for s in starts]
        pairs = [(i, 0, m // 33) for i in range(a.sweep_pairs)]
        batch = Batch(capi, patterns, records, [0, len(records)], pairs, codes)
        want = None
        for span in SPANS:
            os.environ["TXQ_EDIT_LONG_SPAN"] = str(span)
            s = P.timed(capi, batch.run, a.reps)
            got = batch.results()
            if want is None:
                pat, po, txt, ro, go, pr, cd = batch.arrays
                want = host.edit_search((pat, po), (txt, ro), go, pr, cd, threads=16)
            if not np.array_equal(got, want):
                raise SystemExit("span %d, m = %d: device and host results differ" % (span, m))
            out["rows"].append(dict(m=m, span=span, seconds=s, cells_per_s=batch.cells / s))
            note("span sweep: m = %d, span %d: %.4f s" % (m, span, s))
        os.environ.pop("TXQ_EDIT_LONG_SPAN", None)
        batch.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--residues", type=int, default=200_000)
    ap.add_argument("--queries", type=int, default=2000, help="proteins of the peptide workload")
    ap.add_argument("--reads", type=int, default=500, help="reads of the nucleotide workload (three times as long, both strands)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-pairs", type=int, default=0, help="time the host on the first N pairs only (0: all) and scale")
    ap.add_argument("--sweep-bytes", type=int, default=2_000_000)
    ap.add_argument("--sweep-pairs", type=int, default=32)
    ap.add_argument("--workloads", default="peptide,nucleotide")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_verify_long.json"))
    a = ap.parse_args()
    from tetrex_amd import capi, host
    capi.init(0)
    res = dict(device=device_name(), timing="kernel: median of %d calls after one warm-up, host clock around call + synchronize; command: wall "
                                            "time of the process, best of %d, the two routes interleaved" % (a.reps, a.reps))
    if not a.no_sweep:
        res["span_sweep"] = span_sweep(a, capi, host)
    for name in a.workloads.split(","):
        res[name] = workload(name, a, capi, host)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
