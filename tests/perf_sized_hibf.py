"""Measurement of the size-aware HIBF build (`tetrex index --layout sized`) on a Swissprot-shaped synthetic library — not
collected by pytest.  1024 peptide bins whose record counts are spread log-normally, k = 6.  Reports: the build time split
into encode / upload+sketch / union table / layout / insert / download (TETREX_TRACE lines of the CLI), the index bytes of
the sized and of the uniform tree, the measured false-positive rate of the sized tree on 2^16 absent k-mers, and the
200-motif k = 6 batch (mask stage) on both trees.

    python tests/perf_sized_hibf.py [--bins 1024] [--out profiles/sized_hibf_build.json] [--keep DIR]
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
TETREX = os.path.join(ROOT, "bin", "tetrex")
AA = np.array(list("ACDEFGHIKLMNPQRSTVWY"))


def library(d, bins, seed):
    rng = np.random.default_rng(seed)
    n_recs = np.maximum(1, np.round(rng.lognormal(3.0, 1.2, size=bins))).astype(int)
    files = []
    for b in range(bins):
        lens = np.maximum(30, rng.normal(360, 150, size=n_recs[b]).astype(int))
        seq = rng.choice(AA, size=int(lens.sum()))
        at, parts = 0, []
        for i, n in enumerate(lens):
            parts.append(">b%d_%d\n%s\n" % (b, i, "".join(seq[at:at + n])))
            at += n
        p = os.path.join(d, "bin%04d.fa" % b)
        with open(p, "w") as f:
            f.write("".join(parts))
        files.append(p)
    return files, int(n_recs.sum())


def build(d, name, files, flags):
    lst = os.path.join(d, "bins.lst")
    with open(lst, "w") as f:
        f.write("\n".join(files) + "\n")
    t = time.perf_counter()
    r = subprocess.run([TETREX, "index", "-k", "6", *flags, os.path.join(d, name), lst], capture_output=True, text=True,
                       env=dict(os.environ, TETREX_TRACE="1"), timeout=1800)
    wall = time.perf_counter() - t
    if r.returncode != 0 or not os.path.exists(os.path.join(d, name + ".ibf")):
        raise RuntimeError(r.stderr)
    stages = {}
    for m in re.finditer(r"build ms: (.*)", r.stderr):
        for key, val in re.findall(r"([a-z+]+) ([0-9.]+)", m.group(1)):
            stages[key] = float(val)
    shape = re.search(r"sized layout: (.*)", r.stderr)
    return dict(wall_s=wall, stages_ms=stages, bytes=os.path.getsize(os.path.join(d, name + ".ibf")),
                layout=shape.group(1) if shape else None)


def to_descs(ix):
    d = ix.describe()
    out = []
    for i, f in enumerate(d["ibfs"]):
        nxt, tbu = ix.maps(i)
        out.append(dict(bins=f["bins"], bin_size=f["bin_size"], hash_funs=f["hash_funs"], words=ix.words(i),
                        next_ibf_id=nxt, tb_to_user=tbu))
    return d, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--keep", default=None, help="write the library (and bins.lst) here and keep it, e.g. for a profiler run")
    a = ap.parse_args()
    from tetrex_amd import capi, host
    from motifs import random_prosite_motifs
    capi.init(0)
    res = dict(bins=a.bins, k=6)
    with tempfile.TemporaryDirectory() as tmp:
        d = a.keep or tmp
        os.makedirs(d, exist_ok=True)
        files, n_recs = library(d, a.bins, a.seed)
        res["records"] = n_recs
        res["sized"] = build(d, "sized", files, ["--layout", "sized"])
        res["uniform"] = build(d, "uniform", files, [])
        res["bytes_ratio_sized_over_uniform"] = res["sized"]["bytes"] / res["uniform"]["bytes"]
        motifs = random_prosite_motifs(200, 7)
        for name in ("sized", "uniform"):
            ix = host.IndexFile.load(os.path.join(d, name + ".ibf"))
            desc, descs = to_descs(ix)
            dx = capi.Index.upload_hibf(a.bins, descs)
            dx.query_masks(motifs, False, 6)  # warm-up
            best = None
            for _ in range(3):
                t = time.perf_counter()
                dx.query_masks(motifs, False, 6)
                dt = (time.perf_counter() - t) * 1e3
                best = dt if best is None else min(best, dt)
            res[name]["motifs200_mask_ms_best_of_3"] = best
            if name == "sized":  # false positives of the sized tree on k-mers absent from every bin
                present = np.unique(np.concatenate([host.record_values_array(line.strip(), 6, False, 0, True)
                                                     for f in files for line in open(f) if not line.startswith(">")]))
                rng = np.random.default_rng(5)
                cand = np.unique(host.record_values_array("".join(rng.choice(AA, size=400_000)), 6, False, 0, True))
                absent = cand[~np.isin(cand, present)][: 1 << 16].astype(np.uint64)
                masks = dx.probe(absent)
                bits = np.unpackbits(masks.view(np.uint8), axis=1, bitorder="little")[:, : a.bins]
                rate = bits.mean(axis=0)
                res["sized"]["fpr"] = dict(absent_kmers=int(absent.size), mean=float(rate.mean()), max=float(rate.max()))
            dx.free()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
