"""Measurement of six-frame translated search (txq_translate_device, txq_hit_list_device, `tetrex search --translate`;
DESIGN.md §11) — not collected by pytest.  The index is tests/perf_search.py's: 1024 peptide bins of 200 000 residues at
k = 6, flat (-i) and as the default HIBF.  The reads: 10 000 of 900 nt, back-translated with random synonymous codons from
300-residue pieces of the library's proteins with 3 % residue substitutions, every other one reverse-complemented.  Reports:
  * txq_translate_device: median of `--reps` calls after a warm-up, its input bytes (sequence, record offsets, code table),
    its output bytes (values and offsets) and output bytes/s against 8 TB/s;
  * per index: txq_count_device on the device's values, txq_hit_list_device on its hits, and the whole device path through
    the C-ABI (bytes up, translate, offsets down, thresholds up, count, hit list, list down) on the host clock;
  * the yardstick, which is not the code under test: the same reads translated and encoded by txh_translated_values on one
    host thread, uploaded as values through capi.Index.count (what the parent's design would do), timed in the same session;
    the hits of both paths must be identical;
  * the wall time of `tetrex search --translate -e 9` and whether every read's source bin and frame is reported.
Kernel times come from a separate run of this script under a kernel trace with --kernels-only.

    python tests/perf_translate.py [--bins 1024] [--residues 200000] [--reads 10000] [--reps 7] [--legs flat,hibf]
                                   [--kernels-only] [--out profiles/search_translate.json]
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

from perf_search import HBM_BYTES_PER_S, TETREX, build, library, queries, timed, upload  # noqa: E402
import translate_ref as T  # noqa: E402


def back_translate(peptides, seed):
    """reads [(name, bin, frame index, nucleotides)] of 3 x len(peptide) nt: random synonymous codons behind i mod 3 random
    nucleotides (the last codon is cut to keep the length), every other read reverse-complemented"""
    rng = np.random.default_rng(seed)
    codons_of = {}
    for codon, aa in T.CODON.items():
        codons_of.setdefault(aa, []).append(codon)
    out = []
    for i, (name, b, pep) in enumerate(peptides):
        pick = rng.integers(0, 1 << 30, size=len(pep))
        cds = "".join(codons_of[a][p % len(codons_of[a])] for a, p in zip(pep.decode(), pick))
        shift = i % 3
        nt = "".join(rng.choice(list("ACGT"), size=shift)) + cds[:len(cds) - shift]
        frame = shift
        if (i // 3) % 2:
            nt, frame = T.reverse_complement(nt), 3 + shift
        out.append((name, b, frame, nt))
    return out


def host_translate_all(host, reads, k):
    """txh_translated_values on every read, one thread, buffers allocated once; returns (values, offsets[6 n + 1], seconds)"""
    L = host.lib()
    L.txh_translated_values.restype = C.c_int64
    L.txh_translated_values.argtypes = [C.c_uint, C.c_uint, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    raw = [s.encode() for _, _, _, s in reads]
    cap = sum(2 * len(s) for s in raw) + 8
    values = np.zeros(cap, dtype=np.uint64)
    offsets = np.zeros(6 * len(raw) + 1, dtype=np.uint64)
    seven = np.zeros(7, dtype=np.uint64)
    t = time.perf_counter()
    at = 0
    for r, s in enumerate(raw):
        n = L.txh_translated_values(k, 0, s, len(s), values.ctypes.data + 8 * at, cap - at, seven.ctypes.data)
        offsets[6 * r + 1:6 * r + 7] = seven[1:] + np.uint64(at)
        at += n
    return values[:at], offsets, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--residues", type=int, default=200_000)
    ap.add_argument("--reads", type=int, default=10_000)
    ap.add_argument("--errors", type=int, default=9)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--legs", default="flat,hibf")
    ap.add_argument("--kernels-only", action="store_true", help="only the device calls (for a run under a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from tetrex_amd import capi, host
    capi.init(0)
    Lq = capi.lib()
    k = 6
    res = dict(bins=a.bins, residues_per_bin=a.residues, k=k, reads=a.reads, read_length=900, substitutions=0.03, errors=a.errors,
               measured_on="MI355X", timing="median of %d calls after one warm-up, host clock around call + synchronize" % a.reps)
    with tempfile.TemporaryDirectory() as d:
        files, seqs = library(d, a.bins, a.residues, 1)
        _, peptides = queries(d, seqs, a.reads, 300, 0.03, 2)
        reads = back_translate(peptides, 3)
        qpath = os.path.join(d, "reads.fa")
        with open(qpath, "w") as f:
            f.write("".join(">%s\n%s\n" % (n, s) for n, _, _, s in reads))
        seq, rec = capi._records([s for _, _, _, s in reads])
        nq = 6 * len(reads)
        bound = capi.translate_bound(rec, k)
        codes = host.peptide_codes(0)
        d_seq, d_rec, d_codes = capi.DeviceBuffer.from_numpy(seq), capi.DeviceBuffer.from_numpy(rec), capi.DeviceBuffer.from_numpy(codes)
        d_val, d_off = capi.DeviceBuffer(8 * bound + 8), capi.DeviceBuffer(8 * (nq + 1))

        def translate():
            capi.check(Lq.txq_translate_device(d_seq.ptr, d_rec.ptr, len(reads), k, d_codes.ptr, d_val.ptr, d_off.ptr, None))
        s = timed(capi, translate, a.reps)
        offsets = d_off.to_numpy(np.uint64, (nq + 1,))
        n_values = int(offsets[-1])
        out_bytes = 8 * n_values + 8 * (nq + 1)
        res["translate_device"] = dict(seconds=s, input_bytes=int(seq.nbytes + rec.nbytes + 256), output_bytes=out_bytes, values=n_values,
                                       bound=bound, output_bytes_per_s=out_bytes / s, frac_of_8TBps=out_bytes / s / HBM_BYTES_PER_S,
                                       nucleotides_per_s=seq.size / s)
        n_of = np.diff(offsets.astype(np.int64))
        t_of = np.maximum(n_of - k * a.errors, 0)
        thr = np.where(t_of > 0, t_of, 0xFFFFFFFF).astype(np.uint32)  # (a frame with threshold 0 is not searched)
        if not a.kernels_only:
            hv, ho, hs = host_translate_all(host, reads, k)
            assert np.array_equal(ho, offsets) and np.array_equal(hv, d_val.to_numpy(np.uint64, (n_values,)))
            res["host_translate_one_thread_s"] = hs
        for name, flags in (("flat", ["-i"]), ("hibf", [])):
            if name not in a.legs.split(","):
                continue
            r = res[name] = build(d, name, files, flags)
            ix, desc = upload(capi, host, os.path.join(d, name + ".ibf"))
            W = ix.shard_words
            d_thr, d_hit = capi.DeviceBuffer.from_numpy(thr), capi.DeviceBuffer(nq * W * 8)
            d_total = capi.DeviceBuffer(8)
            cap = 1 << 22
            d_list = capi.DeviceBuffer(12 * cap)
            r["count_device_s"] = timed(capi, lambda: ix.count_device(d_val.ptr, d_off.ptr, nq, d_thr.ptr, d_hit.ptr), a.reps)

            def listing():
                capi.check(Lq.txq_hit_list_device(d_hit.ptr, None, nq, W, d_list.ptr, cap, d_total.ptr, None))
            r["hit_list_device_s"] = timed(capi, listing, a.reps)
            total = int(d_total.to_numpy(np.uint64, (1,))[0])
            assert total <= cap
            r["hits"] = total
            r["hit_list_bytes_back"] = 12 * total + 8
            r["hit_matrix_bytes"] = nq * W * 8
            dev_hits = d_hit.to_numpy(np.uint64, (nq, W))
            rows = d_list.to_numpy(np.uint32, (total, 3))
            bits = np.unpackbits(dev_hits.view(np.uint8), axis=1, bitorder="little")
            q, b = np.nonzero(bits)
            assert np.array_equal(rows[:, 0], q) and np.array_equal(rows[:, 1], b)
            listed = set(zip(q.tolist(), b.tolist()))
            r["api_source_bin_and_frame_reported"] = float(np.mean([(6 * i + f, bn) in listed for i, (_, bn, f, _) in enumerate(reads)]))
            if not a.kernels_only:
                # the whole device path through the C-ABI, and the yardstick, in turn
                def device_path():
                    capi.check(Lq.txq_memcpy_h2d(d_seq.ptr, seq.ctypes.data, seq.nbytes))
                    capi.check(Lq.txq_memcpy_h2d(d_rec.ptr, rec.ctypes.data, rec.nbytes))
                    translate()
                    off = d_off.to_numpy(np.uint64, (nq + 1,))
                    n = np.diff(off.astype(np.int64))
                    t = np.maximum(n - k * a.errors, 0)
                    th = np.where(t > 0, t, 0xFFFFFFFF).astype(np.uint32)
                    capi.check(Lq.txq_memcpy_h2d(d_thr.ptr, th.ctypes.data, th.nbytes))
                    ix.count_device(d_val.ptr, d_off.ptr, nq, d_thr.ptr, d_hit.ptr)
                    listing()
                    m = int(d_total.to_numpy(np.uint64, (1,))[0])
                    return d_list.to_numpy(np.uint32, (m, 3))

                def yardstick():
                    v, o, _ = host_translate_all(host, reads, k)
                    n = np.diff(o.astype(np.int64))
                    t = np.maximum(n - k * a.errors, 0)
                    return ix.count(v, o, np.where(t > 0, t, 0xFFFFFFFF).astype(np.uint32))
                r["device_path_s"] = timed(capi, device_path, a.reps)
                r["yardstick_host_translate_plus_count_s"] = timed(capi, yardstick, a.reps)
                r["hits_identical"] = bool(np.array_equal(yardstick(), dev_hits) and np.array_equal(device_path(), rows))
                assert r["hits_identical"]
                r["faster"] = "device path" if r["device_path_s"] < r["yardstick_host_translate_plus_count_s"] else "yardstick"
                t = time.perf_counter()
                cp = subprocess.run([TETREX, "search", "--translate", "-e", str(a.errors), "-v", os.path.join(d, name + ".ibf"), qpath],
                                    capture_output=True, text=True, timeout=1800)
                r["cli_wall_s"] = time.perf_counter() - t
                if cp.returncode != 0:
                    raise RuntimeError(cp.stderr)
                got = {tuple(line.split("\t")) for line in cp.stdout.splitlines()}
                r["cli_reported_search_time_s"] = float(cp.stderr.split("Search time:")[1].split()[0])
                r["cli_rows"] = len(got)
                r["cli_source_bin_and_frame_reported"] = float(np.mean([(n, os.path.abspath(files[bn]), T.FRAMES[f]) in got for n, bn, f, _ in reads]))
            for buf in (d_thr, d_hit, d_total, d_list):
                buf.free()
            ix.free()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
