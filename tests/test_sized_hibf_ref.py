"""The helpers of tests/sized_hibf_ref.py that tests/test_gpu_build_kernels.py builds its inputs with, checked on the CPU:
the inverse of the hash, values crafted for a register and a rank, the slices sketch_kernel cuts a bin into and the chunk
rule of index_build.cpp.  With these right, what the GPU tests expect of a crafted bin is known without a GPU."""
import numpy as np
import pytest

from sized_hibf_ref import M, chunk_csr, craft, fmix, inv_fmix, registers, sketch_slices

REGS = (0, 7, 4095)
RANKS = (1, 2, 31, 52, 53)


def test_inv_fmix_undoes_fmix():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.integers(0, 1 << 64, size=100_000, dtype=np.uint64, endpoint=False),
                        np.array([0, 1, (1 << 64) - 1, 1 << 63, 1 << 52, (1 << 52) - 1], dtype=np.uint64),
                        craft(np.repeat(REGS, len(RANKS)), np.tile(RANKS, len(REGS)))])
    assert np.array_equal(fmix(inv_fmix(x)), x)
    assert np.array_equal(inv_fmix(fmix(x)), x)
    assert int(fmix(np.uint64(12345))) != 12345  # (not the identity)


@pytest.mark.parametrize("r", REGS)
@pytest.mark.parametrize("k", RANKS)
def test_a_crafted_value_sets_one_register_to_its_rank(r, k):
    x = int(craft(r, k))
    assert x >> 52 == r and x & ((1 << 52) - 1) == (1 << (52 - k) if k < 53 else 0)
    regs = registers(inv_fmix(craft([r], [k])))
    want = np.zeros(M, dtype=np.uint8)
    want[r] = k
    assert np.array_equal(regs, want)


def test_crafted_arrays_and_the_max_of_a_register():
    ranks = np.arange(1, 54)
    regs = registers(inv_fmix(craft(ranks * 70, ranks)))
    assert np.array_equal(regs[ranks * 70], ranks) and int(np.count_nonzero(regs)) == 53
    assert registers(inv_fmix(craft([5, 5, 5], [3, 53, 9])))[5] == 53


def test_sketch_slices():
    assert sketch_slices(1) == [(0, 0)]
    assert sketch_slices(16384) == [(0, 16383)]
    assert sketch_slices(16385) == [(0, 16383), (16384, 16384)]
    s = sketch_slices(262144)
    assert len(s) == 16 and s[0] == (0, 16383) and s[15] == (245760, 262143)
    s = sketch_slices(262145)  # 16 slices of 16385, the last one short
    assert len(s) == 16 and s[1] == (16385, 32769) and s[15] == (245775, 262144)
    for n in (16384, 16385, 262144, 262145, 300_000):
        s = sketch_slices(n)
        assert s[0][0] == 0 and s[-1][1] == n - 1 and all(a[1] + 1 == b[0] for a, b in zip(s, s[1:]))


def test_chunk_csr_clamps_the_offsets():
    flat = np.arange(10, dtype=np.uint64)
    offsets = np.array([0, 0, 4, 4, 9, 10, 10], dtype=np.uint64)
    v, o, n = chunk_csr(flat, offsets, 3, 7)  # cuts bins 1 and 3; bins 0, 2, 4, 5 are empty in it
    assert v.tolist() == [3, 4, 5, 6] and o.tolist() == [0, 0, 1, 1, 4, 4, 4] and n == 4 and o.dtype == np.uint64
    parts = [chunk_csr(flat, offsets, g, min(10, g + 4)) for g in (0, 4, 8)]
    for b in range(6):
        got = np.concatenate([v[int(o[b]):int(o[b + 1])] for v, o, _ in parts])
        assert got.tolist() == flat[int(offsets[b]):int(offsets[b + 1])].tolist()
