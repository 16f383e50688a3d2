"""End-to-end wall time of `tetrex search`, this build against a build of another commit, for changes to the host side that
must not cost time — not collected by pytest.  The commands and workloads are those that tests/perf_search.py,
perf_search_verify.py, perf_search_targets.py, perf_translate_verify.py, perf_search_window.py and
perf_search_frame_window.py time at their defaults (their libraries and queries, built once here); each command runs once per
build as a warm-up and then `--runs` times per build, the two builds alternating so that drift hits both alike.  The bar: this
build's median lies within the other build's own run-to-run spread.  The rows of the two builds must be identical.

    python tests/perf_search_host_split.py --parent DIR [--runs 7] [--out profiles/search_host_split.json]

DIR holds the other build as DIR/bin/tetrex (with its libraries at DIR/tetrex_amd/)."""
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
import perf_search_frame_window as PF  # noqa: E402
import perf_translate as PT  # noqa: E402

AA = P.AA


def note(*what):
    print("[perf_search_host_split]", *what, file=sys.stderr, flush=True)


def once(exe, args):
    t = time.perf_counter()
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=1800)
    wall = time.perf_counter() - t
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    return wall, r.stdout, float(r.stderr.split("Search time:")[1].split()[0])


def compare(name, script, args, builds, runs, res):
    rows = {tag: once(exe, args)[1] for tag, exe in builds}  # (the warm-up)
    wall = {tag: [] for tag, _ in builds}
    inner = {tag: [] for tag, _ in builds}
    for _ in range(runs):
        for tag, exe in builds:
            w, _, s = once(exe, args)
            wall[tag].append(w)
            inner[tag].append(s)
    p, n = sorted(wall["parent"]), sorted(wall["new"])
    res["legs"][name] = dict(script=script, command="tetrex " + " ".join(os.path.basename(x) if os.sep in x else x for x in args),
                             rows=rows["new"].count("\n"), rows_identical=rows["parent"] == rows["new"], parent_wall_s=wall["parent"], new_wall_s=wall["new"],
                             parent_median_s=float(np.median(p)), parent_min_s=p[0], parent_max_s=p[-1], new_median_s=float(np.median(n)),
                             parent_search_time_median_s=float(np.median(inner["parent"])), new_search_time_median_s=float(np.median(inner["new"])),
                             new_median_within_parent_spread=bool(np.median(n) <= p[-1]))
    note("%s: parent median %.3f s [%.3f .. %.3f], new median %.3f s" % (name, np.median(p), p[0], p[-1], np.median(n)))


def index(d, name, files):
    lst = os.path.join(d, name + ".lst")
    with open(lst, "w") as f:
        f.write("\n".join(files) + "\n")
    r = subprocess.run([P.TETREX, "index", "-k", "6", "-i", os.path.join(d, name), lst], capture_output=True, text=True, timeout=1800)
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    return os.path.join(d, name + ".ibf")


def small_library(d, tag, rng, bins=1024, residues=20000):
    """the library of perf_search_window.py / perf_search_frame_window.py command()"""
    files, seqs = [], []
    os.makedirs(os.path.join(d, tag))
    for b in range(bins):
        seq = AA[rng.integers(0, 20, size=residues)].tobytes()
        p = os.path.join(d, tag, "bin%04d.fa" % b)
        with open(p, "wb") as f:
            f.write(b"".join(b">b%d_%d\n%s\n" % (b, i, seq[i:i + 2000]) for i in range(0, residues, 2000)))
        files.append(p)
        seqs.append(seq)
    return files, seqs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="a build of the commit to compare with (DIR/bin/tetrex)")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_host_split.json"))
    a = ap.parse_args()
    builds = (("parent", os.path.join(a.parent, "bin", "tetrex")), ("new", P.TETREX))
    res = dict(timing="wall time of the process; one warm-up run per build, then %d runs per build, parent and new alternating" % a.runs,
               bar="the new build's median lies within the parent's own run-to-run spread (at or below the parent's slowest run)", legs={})
    with tempfile.TemporaryDirectory() as d:
        # 1024 bins x 200 000 residues, 10 000 proteins of 300 residues, and those proteins back-translated to reads
        files, seqs = P.library(d, 1024, 200_000, 1)
        qpath, peptides = P.queries(d, seqs, 10_000, 300, 0.03, 2)
        rpath = os.path.join(d, "reads.fa")
        with open(rpath, "w") as f:
            f.write("".join(">%s\n%s\n" % (n, s) for n, _, _, s in PT.back_translate(peptides, 3)))
        flat = index(d, "flat", files)
        compare("search", "perf_search.py", ["search", "-e", "9", "-v", flat, qpath], builds, a.runs, res)
        compare("search_verify", "perf_search_verify.py", ["search", "-e", "9", "--verify", "-v", flat, qpath], builds, a.runs, res)
        compare("search_targets", "perf_search_targets.py", ["search", "-e", "9", "--verify", "--all-targets", "-v", flat, qpath], builds, a.runs, res)
        compare("translate_verify", "perf_translate_verify.py", ["search", "--translate", "-e", "9", "--verify-frames", "-v", flat, rpath], builds, a.runs, res)
        # 1024 bins x 20 000 residues, 2000 chimeras of 3000 letters
        rng = np.random.default_rng(5)
        wfiles, wseqs = small_library(d, "w", rng)
        recs = []
        for q in range(2000):
            x, y = (int(v) for v in rng.choice(1024, size=2, replace=False))
            ax, ay = int(rng.integers(0, 10)) * 2000, int(rng.integers(0, 10)) * 2000
            mid = AA[rng.integers(0, 20, size=1000)].tobytes()
            recs.append(b">c%d_b%d_b%d\n%s\n" % (q, x, y, wseqs[x][ax:ax + 1000] + mid + wseqs[y][ay:ay + 1000]))
        cpath = os.path.join(d, "chimeras.fa")
        with open(cpath, "wb") as f:
            f.write(b"".join(recs))
        compare("search_window", "perf_search_window.py", ["search", "--window", "120", "--step", "30", "-e", "4", "-v", index(d, "wflat", wfiles), cpath],
                builds, a.runs, res)
        # the same shape of library, 2000 contigs of 9000 letters with two planted stretches of 300 residues
        rng = np.random.default_rng(5)
        ffiles, fseqs = small_library(d, "f", rng)
        back = lambda pep: "".join(PF.CODON_OF[c] for c in pep.decode()).encode()
        stretch, flank = 300, (9000 - 6 * 300) // 3
        recs = []
        for q in range(2000):
            x, y = (int(v) for v in rng.choice(1024, size=2, replace=False))
            ax, ay = int(rng.integers(0, 20000 - stretch)), int(rng.integers(0, 20000 - stretch))
            parts = [PF.NT[rng.integers(0, 4, size=flank + int(rng.integers(0, 3)))].tobytes(), back(fseqs[x][ax:ax + stretch]),
                     PF.NT[rng.integers(0, 4, size=flank)].tobytes(), back(fseqs[y][ay:ay + stretch]).translate(PF.COMPLEMENT)[::-1],
                     PF.NT[rng.integers(0, 4, size=flank)].tobytes()]
            recs.append(b">c%d_b%d_b%d\n%s\n" % (q, x, y, b"".join(parts)))
        fpath = os.path.join(d, "contigs.fa")
        with open(fpath, "wb") as f:
            f.write(b"".join(recs))
        compare("search_frame_window", "perf_search_frame_window.py",
                ["search", "--translate", "--frame-window", "40", "--frame-step", "10", "-e", "2", "-v", index(d, "fflat", ffiles), fpath], builds, a.runs, res)
    res["all_within_spread"] = all(e["new_median_within_parent_spread"] for e in res["legs"].values())
    res["all_rows_identical"] = all(e["rows_identical"] for e in res["legs"].values())
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
