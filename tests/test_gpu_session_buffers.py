"""Two sessions open on one index at the same time: the first gets the buffers the index keeps between sessions (its
cache), the second does not and has to own everything it uses — staging sets, streams, the pinned and device buffers of its
final masks and, on a general HIBF, the layout-order rows they are gathered into.  Both must give the oracle's masks, and so
must a third session that adopts the cache afterwards.

Everything runs on one thread, on purpose.  That sessions of one index may end on several threads rests on the ownership
itself — no buffer of a session is shared with another session of the same index (tetrex_amd/csrc/txq_internal.hpp
SessionBuffers) — and not on a race that a test would have to win; this file pins down the ownership: a session without the
cache is complete."""
import numpy as np
import pytest

from helpers import NO_KMER, kmer_values, layout_hibf, make_blob

pytestmark = pytest.mark.gpu

K = 4
MOTIFS = [["LMAEGL", "WHKCQY"], ["DEFGHI", "RSTVWY"], ["NPQRST", "ACDEFG"]]  # per session: one program each
HOLDERS = {"LMAEGL": [3, 64, 250], "WHKCQY": [0, 129], "DEFGHI": [7, 8, 199], "RSTVWY": [130], "NPQRST": [5, 63, 64, 191], "ACDEFG": [17, 170]}


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


def _session_blob(motifs):
    """One program per literal motif: RESULT = the AND of its k-mers' masks, what collect() gives for a literal."""
    kmers, programs = [], []
    for m in motifs:
        first = len(kmers)
        vals = kmer_values(m, K)
        kmers += vals
        ops = [(first, 3, 1, 0)] + [(first + j, 3, 3, 0) for j in range(1, len(vals))] + [(NO_KMER, 2, 3, 2)]
        programs.append((4, ops))
    return make_blob(np.array(kmers, dtype=np.uint64), programs)


def _plant(values):
    for m, bins in HOLDERS.items():
        for b in bins:
            values[b] = np.concatenate([values[b], np.array(kmer_values(m, K), dtype=np.uint64)])


def _flat(oracle, capi):
    bins, rows, h = 260, 4099, 3
    rng = np.random.default_rng(11)
    values = [rng.integers(0, 1 << 20, size=60, dtype=np.uint64) for _ in range(bins)]
    _plant(values)
    ox = oracle.Index.ibf(bins, rows, h, dna=False, k=K)
    for b, v in enumerate(values):
        ox.emplace(v, b)
    return ox, capi.Index.upload_ibf(bins, rows, h, ox.words())


def _layout_order(oracle, capi):
    ox, descs, _ = layout_hibf(oracle, 5, 260, tmax=64, k=K, plant=_plant)
    ix = capi.Index.upload_hibf(260, descs)
    assert ix.supports_dense() == 2  # a general tree: its sessions work in layout order
    return ox, ix


@pytest.mark.parametrize("kind", ["flat", "layout-order-hibf"])
def test_a_session_without_the_cache_owns_all_it_uses(capi, oracle, kind):
    ox, ix = (_flat if kind == "flat" else _layout_order)(oracle, capi)
    want = [np.stack([ox.query(m) for m in ms]) for ms in MOTIFS]
    for ms, w in zip(MOTIFS, want):
        for m, mask in zip(ms, w):
            assert all((int(mask[b >> 6]) >> (b & 63)) & 1 for b in HOLDERS[m]), m  # (no mask is empty: nothing passes vacuously)
    a = ix.session(2)  # gets the cache
    b = ix.session(2)  # does not
    a.stage(_session_blob(MOTIFS[0]))
    b.stage(_session_blob(MOTIFS[1]))
    got_a = a.end()
    got_b = b.end()
    assert np.array_equal(got_a, want[0])
    assert np.array_equal(got_b, want[1])
    c = ix.session(2)  # adopts what a handed back
    c.stage(_session_blob(MOTIFS[2]))
    assert np.array_equal(c.end(), want[2])
    ix.free()
