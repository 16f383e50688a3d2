"""Measurement of the windows of translated frames (txq_translate_windows, `tetrex search --translate --frame-window`;
DESIGN.md §18) — not collected by pytest.  One MI355X.

  (a) translation: txq_translate_windows_device against txq_translate_device on the same bytes, in the same process, in
      interleaved rounds with device events around each call; the figure of a route is its best of `--reps` rounds.  Two
      inputs: `--reads` reads of `--read-length` nt, and one contig of `--contig` nt.  The values and offsets of the two
      routes are compared.
  (b) the count: the windows of the reads through txq_count_windows_device, against the same windows written out as disjoint
      queries through txq_count_device, on the flat 1024-bin index of bench.py (S-IBF-1024); timed the same way, the hit
      matrices compared.
  (c) the command: `tetrex search --translate -e E` with and without --frame-window W --frame-step S on `--records` contigs
      of `--letters` nt (random nucleotides around a back-translated stretch of one bin and the reverse complement of a
      stretch of another) against a 1024-bin flat peptide index, wall time and rows; with `--parent DIR` (a build of the
      parent commit: DIR/bin/tetrex) the plain run of that build on the same file too, interleaved.

    python tests/perf_search_frame_window.py [--reps 5] [--window 40] [--window-step 10] [--no-kernels] [--no-cli] [--parent DIR]
                                             [--out profiles/search_frame_window.json]
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
NT = np.frombuffer(b"ACGT", dtype=np.uint8)
# one codon per residue of AA, NCBI table 1
CODON_OF = {"A": "GCT", "C": "TGC", "D": "GAT", "E": "GAA", "F": "TTC", "G": "GGC", "H": "CAT", "I": "ATC", "K": "AAA", "L": "CTG", "M": "ATG",
            "N": "AAC", "P": "CCG", "Q": "CAG", "R": "CGT", "S": "AGC", "T": "ACC", "V": "GTG", "W": "TGG", "Y": "TAC"}
COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")


def timed(torch, variants, reps):
    best = {}
    for _ in range(reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            best[name] = min(best.get(name, ms), ms)
    return best


def kernels(a, res):
    import torch
    import bench
    from tetrex_amd import capi, host
    L = capi.lib()
    k, W, S = 6, a.window, a.window_step
    rng = np.random.default_rng(11)
    stream = torch.cuda.current_stream().cuda_stream
    dev = lambda x: torch.from_numpy(x).cuda()
    codes = dev(np.ascontiguousarray(host.peptide_codes(0), dtype=np.uint8))
    out = res["translation"] = dict(k=k, window=W, step=S, timing="device events around each call, best of %d interleaved rounds in one process" % a.reps,
                                    inputs={})
    kept = None
    for name, n, length in (("reads", a.reads, a.read_length), ("contig", 1, a.contig)):
        seq = NT[rng.integers(0, 4, size=n * length)]
        rec = (np.arange(n + 1, dtype=np.uint64) * np.uint64(length))
        bound, n_win = capi.translate_bound(rec, k), capi.translate_windows_bound(rec, k, W, S)
        d_seq, d_rec = dev(np.concatenate([seq, np.zeros(16, dtype=np.uint8)])), dev(rec.view(np.int64))
        val_t, off_t = torch.zeros(bound + 1, dtype=torch.int64, device="cuda"), torch.zeros(6 * n + 1, dtype=torch.int64, device="cuda")
        val_w, off_w = torch.zeros(bound + 1, dtype=torch.int64, device="cuda"), torch.zeros(6 * n + 1, dtype=torch.int64, device="cuda")
        woff = torch.zeros(6 * n + 1, dtype=torch.int64, device="cuda")
        beg, ln = torch.zeros(n_win + 1, dtype=torch.int64, device="cuda"), torch.zeros(n_win + 2, dtype=torch.int32, device="cuda")
        variants = {
            "translate": lambda: capi.check(L.txq_translate_device(d_seq.data_ptr(), d_rec.data_ptr(), n, k, codes.data_ptr(), val_t.data_ptr(),
                                                                   off_t.data_ptr(), stream)),
            "translate_windows": lambda: capi.check(L.txq_translate_windows_device(d_seq.data_ptr(), d_rec.data_ptr(), n, k, codes.data_ptr(), W, S,
                                                                                   val_w.data_ptr(), off_w.data_ptr(), woff.data_ptr(), beg.data_ptr(),
                                                                                   ln.data_ptr(), stream)),
        }
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        n_values = int(off_t[-1])
        if not (torch.equal(off_t, off_w) and torch.equal(val_t[:n_values], val_w[:n_values]) and int(woff[-1]) == n_win):
            raise RuntimeError("%s: the two routes translate differently" % name)
        best = timed(torch, variants, a.reps)
        out["inputs"][name] = dict(records=n, length=length, values=n_values, windows=n_win, translate_ms=best["translate"],
                                   translate_windows_ms=best["translate_windows"], time_ratio=best["translate_windows"] / best["translate"],
                                   empty_windows=int((ln[:n_win] == 0).sum()))
        if name == "reads":
            kept = (val_w, beg, ln, n_win)
    # (b) the count of the reads' windows
    bins, h, rows, per_bin, bits = 1024, 3, 1247045, 200000, 20
    ix = bench.build_index(capi, torch, bins, bins, rows, h, 0, 1, per_bin, bits)
    words = ix.shard_words
    val, beg, ln, n_win = kept
    lens = ln[:n_win].to(torch.int64)
    thr = torch.clamp(lens // 2, min=1).to(torch.int32)
    off = torch.zeros(n_win + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(lens, 0)
    total = int(off[-1])
    owner = torch.repeat_interleave(torch.arange(n_win, device="cuda"), lens)
    dup = val[beg[:n_win][owner] + (torch.arange(total, device="cuda") - off[:-1][owner])].contiguous()  # the windows written out
    del owner
    hit_w = torch.zeros(n_win * words, dtype=torch.int64, device="cuda")
    hit_b = torch.zeros(n_win * words, dtype=torch.int64, device="cuda")
    variants = {
        "written_out": lambda: ix.count_device(dup.data_ptr(), off.data_ptr(), n_win, thr.data_ptr(), hit_b.data_ptr(), None, stream),
        "sliding": lambda: ix.count_windows_device(val.data_ptr(), beg.data_ptr(), ln.data_ptr(), n_win, thr.data_ptr(), hit_w.data_ptr(), None, stream),
    }
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    if not torch.equal(hit_w, hit_b):
        raise RuntimeError("the sliding count differs from txq_count_device's")
    best = timed(torch, variants, a.reps)
    res["count"] = dict(index="S-IBF-1024 of bench.py (1024 bins, h = 3, %d rows, %d values per bin)" % (rows, per_bin), windows=n_win,
                        values=int(out["inputs"]["reads"]["values"]), values_written_out=total, written_out_ms=best["written_out"],
                        sliding_ms=best["sliding"], time_ratio=best["sliding"] / best["written_out"])
    ix.free()


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
        qpath = os.path.join(d, "contigs.fa")
        with open(qpath, "wb") as f:
            f.write(b"".join(recs))
        lst = os.path.join(d, "bins.lst")
        with open(lst, "w") as f:
            f.write("\n".join(files) + "\n")
        r = subprocess.run([TETREX, "index", "-k", str(k), "-i", os.path.join(d, "flat"), lst], capture_output=True, text=True, timeout=1800)
        if r.returncode != 0:
            raise RuntimeError(r.stderr)
        index = os.path.join(d, "flat.ibf")
        plain = ["search", "--translate", "-e", str(a.errors), "-v", index, qpath]
        legs = {"frame_window": [TETREX, "search", "--translate", "--frame-window", str(a.window), "--frame-step", str(a.window_step), "-e", str(a.errors),
                                 "-v", index, qpath],
                "plain": [TETREX] + plain}
        if a.parent:
            legs["plain_parent_build"] = [os.path.join(a.parent, "bin", "tetrex")] + plain
        out = res["command"] = dict(bins=bins, residues_per_bin=residues, k=k, records=a.records, letters=a.letters, planted_residues=stretch,
                                    window=a.window, step=a.window_step, errors=a.errors,
                                    timing="wall time of the process, best of %d interleaved runs after one warm-up run each" % a.reps, legs={})
        outputs = {}
        for rep in range(a.reps + 1):
            for name, cmd in legs.items():
                t = time.perf_counter()
                cp = subprocess.run(cmd, capture_output=True, text=True, timeout=1800)
                wall = time.perf_counter() - t
                if cp.returncode != 0:
                    raise RuntimeError(cp.stderr)
                outputs[name] = cp.stdout
                if rep == 0:
                    out["legs"][name] = dict(rows=len(cp.stdout.splitlines()), stderr_tail=[l for l in cp.stderr.strip().splitlines() if "skipped" not in l][-2:])
                    continue
                e = out["legs"][name]
                e["wall_s"] = min(e.get("wall_s", wall), wall)
                e["search_time_s"] = min(e.get("search_time_s", 1e9), float(cp.stderr.split("Search time:")[1].split()[0]))
        if a.parent:
            out["plain_rows_equal_parent_build"] = outputs["plain"] == outputs["plain_parent_build"]
        found = {tuple(line.split("\t")[:2]) for line in outputs["frame_window"].splitlines()}
        both = 0
        for q in range(a.records):
            name = recs[q].split(b"\n")[0][1:].decode()
            x, y = (int(s[1:]) for s in name.split("_")[1:])
            both += (name, os.path.abspath(files[x])) in found and (name, os.path.abspath(files[y])) in found
        out["frame_window_both_bins_reported"] = both / a.records
        out["plain_records_with_a_row"] = len({line.split("\t")[0] for line in outputs["plain"].splitlines()}) / a.records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reads", type=int, default=10_000)
    ap.add_argument("--read-length", type=int, default=900)
    ap.add_argument("--contig", type=int, default=1_000_000)
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--letters", type=int, default=9000)
    ap.add_argument("--window", type=int, default=40, help="residues of a window")
    ap.add_argument("--window-step", type=int, default=10)
    ap.add_argument("--errors", type=int, default=2)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--parent", default=None, help="a build of the parent commit (DIR/bin/tetrex) for the plain run")
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
