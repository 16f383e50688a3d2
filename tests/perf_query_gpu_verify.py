"""Measurement of `tetrex query --gpu-verify` — not collected by pytest.  Library and batch are those of
bench.py's end_to_end.with_verification: 1024 FASTA bins of 200 000 uniform random residues in 360-residue records, a flat
IBF at k = 6 written by `tetrex index -i`, 200 PROSITE-style motifs through `tetrex query -f -S`.

    python tests/perf_query_gpu_verify.py [--out profiles/query_gpu_verify.json] [--repeats 3] [--only-flag THREADS]

Each of -t 1 and -t 16 runs without and with the flag, the two variants interleaved, after one run of each that warms the
page cache; the best batch_seconds of --repeats counts.  The run without the flag is the yardstick: the verification code as
it was.  Result files of the two variants must be byte-identical.  One more run of each variant under TETREX_TRACE=1 records
where the time goes.  --only-flag N: nothing but one flagged -t N run on a library made before (for a profiler: the kernel's
bytes per second come from a kernel trace of this run, made in a run of its own)."""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from motifs import random_prosite_motifs  # noqa: E402

TETREX = os.path.join(ROOT, "bin", "tetrex")
BINS, PER_BIN, K = 1024, 200000, 6


def make_library(work):
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    rng = np.random.default_rng(11)
    files = []
    for b in range(BINS):
        seq = aa[rng.integers(0, 20, size=PER_BIN)]
        path = os.path.join(work, "bin%04d.fa" % b)
        with open(path, "wb") as f:
            for i, start in enumerate(range(0, PER_BIN, 360)):
                f.write(b">sp|%04d_%d\n" % (b, i))
                f.write(seq[start:start + 360].tobytes())
                f.write(b"\n")
        files.append(path)
    motifs = random_prosite_motifs(200, 3, wildcard=0.05, ranges=0.02, min_len=8, max_len=14)
    with open(os.path.join(work, "motifs.tsv"), "w") as f:
        for i, m in enumerate(motifs):
            f.write("M%03d\t%s\n" % (i, m))
    subprocess.run([TETREX, "index", "-k", str(K), "-i", "sp", *files], check=True, capture_output=True, cwd=work)
    return motifs


def query(work, sub, threads, flag, trace=False):
    d = os.path.join(work, sub)
    os.makedirs(d, exist_ok=True)
    for p in glob.glob(os.path.join(d, "*.tsv")):
        os.unlink(p)
    env = dict(os.environ, TETREX_TRACE="1") if trace else {k: v for k, v in os.environ.items() if k != "TETREX_TRACE"}
    r = subprocess.run([TETREX, "query", "-S", "-f", "-t", str(threads), *(["--gpu-verify"] if flag else []), os.path.join(work, "sp.ibf"),
                        os.path.join(work, "motifs.tsv")], capture_output=True, text=True, cwd=d, env=env, check=True)
    stats = [json.loads(ln) for ln in r.stderr.splitlines() if ln.startswith("{")]
    whole = [x for x in stats if "batch_seconds" in x][-1]
    out = {"batch_seconds": whole["batch_seconds"], "verify_seconds": whole["verify_seconds"],
           "mask_seconds": [x for x in stats if "mask_seconds" in x][-1]["mask_seconds"]}
    out.update({k: v for x in stats for k, v in x.items() if k == "gpu_verify"})
    if trace:
        out["trace"] = [ln for ln in r.stderr.splitlines() if ln.startswith("[tetrex] verify_batch") or ln.startswith("[tetrex] gpu-verify")]
    files = {os.path.basename(p): open(p, "rb").read() for p in sorted(glob.glob(os.path.join(d, "*.tsv")))}
    return out, files, r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_gpu_verify.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--work", default=None, help="keep the library here (made if sp.ibf is missing)")
    ap.add_argument("--only-flag", type=int, default=0)
    args = ap.parse_args()
    tmp = None if args.work else tempfile.TemporaryDirectory(prefix="tetrex_gpu_verify_")
    work = args.work or tmp.name
    os.makedirs(work, exist_ok=True)
    if not os.path.exists(os.path.join(work, "sp.ibf")):
        make_library(work)
    if args.only_flag:
        print(json.dumps(query(work, "flag", args.only_flag, True)[0]))
        return
    result = {"workload": "%d FASTA bins of %d residues (360-residue records), flat IBF k = %d, 200 PROSITE-style motifs, tetrex query -f -S" % (BINS, PER_BIN, K),
              "text_bytes": BINS * PER_BIN, "repeats": args.repeats, "runs": {}}
    for threads in (1, 16):
        best = {False: None, True: None}
        files = {}
        for rep in range(args.repeats + 1):  # (the first round warms the page cache for both variants and does not count)
            for flag in (False, True):
                out, files[flag], stdout = query(work, "flag" if flag else "plain", threads, flag)
                if rep and (best[flag] is None or out["batch_seconds"] < best[flag]["batch_seconds"]):
                    best[flag] = out
            if files[False] != files[True]:
                raise SystemExit("result files differ between the variants at -t %d" % threads)
        for flag in (False, True):
            best[flag]["trace"] = query(work, "flag" if flag else "plain", threads, flag, trace=True)[0]["trace"]
        result["runs"]["threads_%d" % threads] = {"plain": best[False], "gpu_verify": best[True], "identical_files": True,
                                                  "files_with_rows": sum(len(v) > 0 for v in files[False].values()),
                                                  "batch_speedup": best[False]["batch_seconds"] / best[True]["batch_seconds"],
                                                  "verify_speedup": best[False]["verify_seconds"] / best[True]["verify_seconds"]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result["runs"], sort_keys=True))


if __name__ == "__main__":
    main()
