"""numpy restatements for the size-aware HIBF layout (include/txq.h txq_sketch_device / txq_union_estimates_device /
txq_tree_insert_device, tetrex_amd/csrc/host/layout.hpp): the hash, the HyperLogLog registers and estimator, the part rule
of split bins, checks of a layout's structure, and what tests/test_gpu_build_kernels.py makes its inputs with: the inverse
of the hash, values crafted for a register and a rank, the sketch's slices and the chunk rule of the build."""
import math

import numpy as np

M = 4096
ALPHA_MM = 0.7213 / (1.0 + 1.079 / M) * M * M
MERGED = 0xFFFFFFFFFFFFFFFF
_U = np.uint64


def fmix(x):
    """splitmix64's finaliser."""
    x = np.array(x, dtype=np.uint64, copy=True)
    with np.errstate(over="ignore"):
        x ^= x >> _U(30)
        x *= _U(0xbf58476d1ce4e5b9)
        x ^= x >> _U(27)
        x *= _U(0x94d049bb133111eb)
        x ^= x >> _U(31)
    return x


_INV_C1 = pow(0xbf58476d1ce4e5b9, -1, 1 << 64)
_INV_C2 = pow(0x94d049bb133111eb, -1, 1 << 64)


def inv_fmix(x):
    """The inverse of fmix: each xorshift undone (y ^ y >> s ^ y >> 2s ...), each multiply by the constant's inverse mod 2^64."""
    x = np.array(x, dtype=np.uint64, copy=True)
    with np.errstate(over="ignore"):
        x ^= (x >> _U(31)) ^ (x >> _U(62))
        x *= _U(_INV_C2)
        x ^= (x >> _U(27)) ^ (x >> _U(54))
        x *= _U(_INV_C1)
        x ^= (x >> _U(30)) ^ (x >> _U(60))
    return x


def craft(reg, rank):
    """The hashed value x that sets register `reg` to exactly `rank` (1 .. 53): the top 12 bits are reg, the low 52 bits
    1 << (52 - rank), or 0 for rank 53 (x << 12 == 0).  inv_fmix(craft(reg, rank)) is the value to put in a bin."""
    reg, rank = np.asarray(reg, dtype=np.uint64), np.asarray(rank, dtype=np.uint64)
    assert np.all(reg < M) and np.all((rank >= 1) & (rank <= 53))
    low = np.where(rank < 53, _U(1) << (_U(52) - np.minimum(rank, _U(52))), _U(0))
    return (reg << _U(52)) | low


def sketch_slices(n):
    """(first, last) index of every slice of a bin of n values, as sketch_kernel cuts it: 16 workgroups at most, each with
    max(16384, ceil(n / 16)) values, a slice that would begin at or behind n not run."""
    chunk = max(16384, (n + 15) // 16)
    return [(s * chunk, min(n, (s + 1) * chunk) - 1) for s in range(16) if s * chunk < n]


def chunk_csr(flat, offsets, g0, g1):
    """Values [g0, g1) of a CSR array as a chunk of its own over all bins (index_build.cpp upload_chunk):
    offsets[b] = clamp(offsets[b], g0, g1) - g0.  Returns (values, offsets, n_values)."""
    offs = np.asarray(offsets, dtype=np.uint64)
    return flat[g0:g1], np.clip(offs, _U(g0), _U(g1)) - _U(g0), g1 - g0


def _clz64(w):
    w = np.array(w, dtype=np.uint64, copy=True)
    zero = w == 0
    n = np.zeros(w.shape, dtype=np.uint64)
    for s in (32, 16, 8, 4, 2, 1):
        m = (w >> _U(64 - s)) == 0
        n[m] += _U(s)
        w[m] <<= _U(s)
    n[zero] = 64
    return n


def registers(values):
    """4096 u8 registers of one bin: register x >> 52 of x = fmix(v) holds the max of min(clz(x << 12), 52) + 1."""
    regs = np.zeros(M, dtype=np.uint8)
    v = np.asarray(values, dtype=np.uint64)
    if v.size:
        x = fmix(v)
        rank = np.minimum(_clz64(x << _U(12)), _U(52)) + _U(1)
        np.maximum.at(regs, (x >> _U(52)).astype(np.int64), rank.astype(np.uint8))
    return regs


def estimate(regs):
    """alpha_m m^2 / sum 2^-M (the sum exact, rounded once), linear counting m ln(m / V) where E <= 2.5 m and V > 0."""
    r = np.minimum(np.asarray(regs, dtype=np.int64), 53)
    counts = np.bincount(r, minlength=54)
    total = sum(int(c) << (53 - i) for i, c in enumerate(counts) if c)
    e = ALPHA_MM / (float(total) * 2.0 ** -53)
    zeros = int(counts[0])
    if e <= 2.5 * M and zeros > 0:
        e = float(M) * math.log(float(M) / float(zeros))
    return e


def union_table(regs, order, window):
    """[s, L-1] = estimate of the union of bins order[s .. s+L-1]; 0.0 past the end."""
    B = regs.shape[0]
    out = np.zeros((B, window), dtype=np.float64)
    for s in range(B):
        acc = np.zeros(M, dtype=np.uint8)
        for L in range(1, window + 1):
            if s + L > B:
                break
            acc = np.maximum(acc, regs[int(order[s + L - 1])])
            out[s, L - 1] = estimate(acc)
    return out


def part_of(values, parts):
    """The part of a split bin that holds each value: mulhi64(fmix(v ^ 0x9e3779b97f4a7c15), parts)."""
    x = fmix(np.asarray(values, dtype=np.uint64) ^ _U(0x9e3779b97f4a7c15))
    hi, lo = x >> _U(32), x & _U(0xFFFFFFFF)
    p = _U(parts)
    # (hi * 2^32 + lo) * p >> 64 with p < 2^32: hi * p + (lo * p >> 32), then >> 32
    return (hi * p + ((lo * p) >> _U(32))) >> _U(32)


def paths(ibfs):
    """Each user bin's path from the root: [(ibf, first technical bin, parts)], from the maps alone.  Asserts that every
    user bin is exactly one run of technical bins in exactly one IBF and every IBF but the root has exactly one parent."""
    out = {}
    parent = {}

    def walk(i, stack):
        tbu, nxt = ibfs[i]["tb_to_user_bin"], ibfs[i]["next_ibf_id"]
        t, T = 0, len(tbu)
        while t < T:
            if int(tbu[t]) == MERGED:
                c = int(nxt[t])
                assert 0 < c < len(ibfs) and c not in parent, (i, t, c)
                parent[c] = (i, t)
                walk(c, stack + [(i, t, 1)])
                t += 1
                continue
            ub = int(tbu[t])
            e = t
            while e < T and int(tbu[e]) == ub:
                e += 1
            assert ub not in out, "user bin %d placed twice" % ub
            out[ub] = stack + [(i, t, e - t)]
            t = e

    walk(0, [])
    assert len(parent) == len(ibfs) - 1
    return out


def total_bits(ibfs):
    return sum(64 * ((f["bins"] + 63) // 64) * f["bin_size"] for f in ibfs)


def uniform_bits(counts, fpr=0.05):
    """Bits of the uniform two-level tree `tetrex index` writes by default (index_build.cpp build_index) for bins of
    these sizes: a child of 64 * ceil(ceil(B / t_max) / 64) user bins each, every child with the rows of the largest
    bin, the root sized by its largest merged bin."""
    def bitcount(n):
        return int(math.ceil(-n * math.log(np.float32(fpr)) / math.log(2) ** 2))
    B = len(counts)
    tmax = 64 * ((int(math.ceil(math.sqrt(B))) + 63) // 64)
    if B <= tmax:
        return 64 * ((B + 63) // 64) * max(1, bitcount(max(counts)))
    per_child = 64 * (((B + tmax - 1) // tmax + 63) // 64)
    n_child = (B + per_child - 1) // per_child
    child_rows = max(1, bitcount(max(counts)))
    merged = [sum(counts[c * per_child:(c + 1) * per_child]) for c in range(n_child)]
    return n_child * per_child * child_rows + 64 * ((n_child + 63) // 64) * max(1, bitcount(max(merged)))
