"""Measurement of threshold membership (txq_count, `tetrex search`) on a Swissprot-shaped synthetic library — not collected
by pytest.  1024 peptide bins of 200 000 residues at k = 6, indexed flat (-i) and as the default HIBF; 10 000 query proteins
of 300 residues cut from the bins' records with 3 % substitutions.  Reports:
  * txq_count_device: values/s (median of `--reps` timed calls after a warm-up), its algorithmic bytes per value
    (h * W * 8 + 8) and the fraction of 8 TB/s, on the flat IBF and on the HIBF;
  * txq_probe_device with TXQ_PROBE_TABLE=0 on the same values in the same process (bytes per value h * W * 8 + W * 8 + 8);
  * the wall time of `tetrex search -e 9` on both indexes, the fraction of queries whose source bin is reported (must be
    1.0) and the mean number of bins reported per query.

    python tests/perf_search.py [--bins 1024] [--residues 200000] [--queries 10000] [--reps 5] [--legs flat,hibf] [--no-cli]
                                [--out profiles/search_swissprot.json]
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
HBM_BYTES_PER_S = 8e12


def library(d, bins, residues, seed):
    rng = np.random.default_rng(seed)
    files, seqs = [], []
    for b in range(bins):
        seq = AA[rng.integers(0, 20, size=residues)].tobytes()
        recs = [seq[i:i + 400] for i in range(0, len(seq), 400)]  # proteins of 400 residues
        p = os.path.join(d, "bin%04d.fa" % b)
        with open(p, "wb") as f:
            f.write(b"".join(b">b%d_%d\n%s\n" % (b, i, r) for i, r in enumerate(recs)))
        files.append(p)
        seqs.append(seq)
    return files, seqs


def queries(d, seqs, n, length, subst, seed):
    rng = np.random.default_rng(seed)
    out = []
    for q in range(n):
        b = int(rng.integers(0, len(seqs)))
        rec = int(rng.integers(0, len(seqs[b]) // 400))  # within one record of the bin (400 residues)
        at = rec * 400 + int(rng.integers(0, 400 - length + 1))
        s = bytearray(seqs[b][at:at + length])
        for i in rng.choice(length, size=int(round(subst * length)), replace=False):
            s[i] = AA[(np.flatnonzero(AA == s[i])[0] + 1 + int(rng.integers(0, 19))) % 20]
        out.append(("q%d_b%d" % (q, b), b, bytes(s)))
    p = os.path.join(d, "queries.fa")
    with open(p, "wb") as f:
        f.write(b"".join(b">%s\n%s\n" % (n.encode(), s) for n, _, s in out))
    return p, out


def build(d, name, files, flags):
    lst = os.path.join(d, "bins.lst")
    with open(lst, "w") as f:
        f.write("\n".join(files) + "\n")
    t = time.perf_counter()
    r = subprocess.run([TETREX, "index", "-k", "6", *flags, os.path.join(d, name), lst], capture_output=True, text=True, timeout=1800)
    if r.returncode != 0 or not os.path.exists(os.path.join(d, name + ".ibf")):
        raise RuntimeError(r.stderr)
    return dict(build_wall_s=time.perf_counter() - t, bytes=os.path.getsize(os.path.join(d, name + ".ibf")))


def upload(capi, host, path):
    ix = host.IndexFile.load(path)
    d = ix.describe()
    if not d["is_hibf"]:
        f = d["ibfs"][0]
        return capi.Index.upload_ibf(f["bins"], f["bin_size"], f["hash_funs"], ix.words(0)), d
    descs = []
    for i, f in enumerate(d["ibfs"]):
        nxt, tbu = ix.maps(i)
        descs.append(dict(bins=f["bins"], bin_size=f["bin_size"], hash_funs=f["hash_funs"], words=ix.words(i), next_ibf_id=nxt, tb_to_user=tbu))
    return capi.Index.upload_hibf(d["bins"], descs), d


def timed(capi, fn, reps):
    fn()
    capi.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        capi.synchronize()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--residues", type=int, default=200_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--errors", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="flat,hibf", help="which indexes: flat, hibf or both")
    ap.add_argument("--no-cli", action="store_true", help="skip the `tetrex search` runs (e.g. under a counter pass)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from tetrex_amd import capi, host
    capi.init(0)
    k = 6
    res = dict(bins=a.bins, residues_per_bin=a.residues, k=k, queries=a.queries, query_length=a.length, substitutions=0.03,
               errors=a.errors, measured_on="MI355X", timing="median of %d calls after one warm-up, host clock around call + synchronize" % a.reps)
    with tempfile.TemporaryDirectory() as d:
        files, seqs = library(d, a.bins, a.residues, 1)
        qpath, qs = queries(d, seqs, a.queries, a.length, 0.03, 2)
        vals = [host.record_values_array(s, k, dna=False) for _, _, s in qs]
        n_of = np.array([v.size for v in vals], dtype=np.int64)
        values = np.concatenate(vals)
        offsets = np.zeros(len(vals) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum(n_of)
        thr = np.maximum(n_of - k * a.errors, 0).astype(np.uint32)
        n = int(values.size)
        res["values"] = n
        for name, flags in (("flat", ["-i"]), ("hibf", [])):
            if name not in a.legs.split(","):
                continue
            r = res[name] = build(d, name, files, flags)
            ix, desc = upload(capi, host, os.path.join(d, name + ".ibf"))
            W = ix.shard_words
            h = desc["ibfs"][0]["hash_funs"] if name == "flat" else None
            dv, do, dt = capi.DeviceBuffer.from_numpy(values), capi.DeviceBuffer.from_numpy(offsets), capi.DeviceBuffer.from_numpy(thr)
            dh = capi.DeviceBuffer(len(vals) * W * 8)
            s = timed(capi, lambda: ix.count_device(dv.ptr, do.ptr, len(vals), dt.ptr, dh.ptr), a.reps)
            e = r["count_device"] = dict(seconds=s, values_per_s=n / s)
            if name == "flat":
                e["bytes_per_value"] = h * W * 8 + 8
                e["frac_of_8TBps"] = n / s * e["bytes_per_value"] / HBM_BYTES_PER_S
            got = dh.to_numpy(np.uint64, (len(vals), W))
            bits = np.unpackbits(got.view(np.uint8), axis=1, bitorder="little")[:, : a.bins]
            src = np.array([b for _, b, _ in qs])
            r["api_source_bin_reported"] = float(bits[np.arange(len(qs)), src].mean())
            r["api_mean_bins_reported"] = float(bits.sum(axis=1).mean())
            if name == "flat":
                os.environ["TXQ_PROBE_TABLE"] = "0"
                dm = capi.DeviceBuffer(n * W * 8)
                s = timed(capi, lambda: ix.probe_device(dv.ptr, n, dm.ptr), a.reps)
                r["probe_device_table0"] = dict(seconds=s, values_per_s=n / s, bytes_per_value=h * W * 8 + W * 8 + 8,
                                                frac_of_8TBps=n / s * (h * W * 8 + W * 8 + 8) / HBM_BYTES_PER_S)
                os.environ.pop("TXQ_PROBE_TABLE", None)
                r["count_over_probe_time_per_value"] = r["count_device"]["seconds"] / s
                dm.free()
            for b in (dv, do, dt, dh):
                b.free()
            ix.free()
            if a.no_cli:
                continue
            # the command line
            t = time.perf_counter()
            cp = subprocess.run([TETREX, "search", "-e", str(a.errors), "-v", os.path.join(d, name + ".ibf"), qpath],
                                capture_output=True, text=True, timeout=1800)
            wall = time.perf_counter() - t
            if cp.returncode != 0:
                raise RuntimeError(cp.stderr)
            rows = [line.split("\t") for line in cp.stdout.splitlines()]
            reported = {(q, p) for q, p in rows}
            r["cli_wall_s"] = wall
            r["cli_reported_search_time_s"] = float(cp.stderr.split("Search time:")[1].split()[0])
            r["cli_source_bin_reported"] = float(np.mean([(q, os.path.abspath(files[b])) in reported for q, b, _ in qs]))
            r["cli_mean_bins_reported"] = len(rows) / len(qs)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
