"""GPU parity of the flat probe's table-only tile body (txq_probe.hip table_tile): a full tile of an answer whose 64 k-mers all lie
below the table's valid rows reads its rows and stores its masks without hashing and without a choice per lane; every other tile
(ragged, a k-mer at or above `valid`) takes the general body.

Every test is a SEQUENCE of calls on one index under TXQ_PROBE_TABLE=1, enqueued without a wait between them.  Every call's masks
and `alive` are compared bit for bit with the CPU oracle, and with the same calls on a second index under TXQ_PROBE_TABLE_TILE=0
(every tile in the general body).  Shapes: 4099 rows, h in {2, 3}, n = 70 017 (1094 full tiles and one ragged k-mer)."""
import numpy as np
import pytest

from helpers import random_words, oracle_ibf_from_words, splitmix64
from test_gpu_probe_domain_table import _alive_bits, _domain_batch
from test_gpu_probe_one_launch import _Ref

pytestmark = pytest.mark.gpu

ROWS, N = 4099, 70000 + 17
TOP = 16000  # the reference holds the oracle's mask of every value below it, made once per index
FAR = np.uint64(1) << np.uint64(40)  # at or above `valid` and beyond every capacity: gathered, never counted
# mask words, bins, shards, rank: 16 the bench's shape (LPK 8, every lane a chunk); 15 an odd tail word; 10 five chunks on LPK 8
# (masked lanes); 8 and 2 LPK 4 and 1; 32 LPK 16 (two groups of steps); the second column shard of 2048 bins (shard_word0 = 16)
WIDTHS = {"W16": (16, 1024, 1, 0), "W15": (15, 960, 1, 0), "W10": (10, 640, 1, 0), "W8": (8, 512, 1, 0), "W2": (2, 128, 1, 0),
          "W32": (32, 2048, 1, 0), "W16shard": (16, 2048, 2, 1)}


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def refs(oracle):
    """Per (width, h) the index's words and its reference, made on first use, shared and never changed."""
    made = {}

    def get(capi, width, h):
        W, bins, shards, rank = WIDTHS[width]
        if (width, h) not in made:
            words = random_words(bins, ROWS, 0.35, 300 + bins + h)
            ix = capi.Index.upload_ibf(bins, ROWS, h, words, shard_rank=rank, n_shards=shards)
            lo, nw = int(ix.info.shard_word0), ix.shard_words
            ix.free()
            assert nw == W and (lo != 0) == (rank != 0)
            made[(width, h)] = (words, _Ref(oracle_ibf_from_words(oracle, bins, ROWS, h, words), TOP, slice(lo, lo + nw)))
        return made[(width, h)]
    return get


def _upload(capi, width, h, words):
    _, bins, shards, rank = WIDTHS[width]
    return capi.Index.upload_ibf(bins, ROWS, h, words, shard_rank=rank, n_shards=shards)


def _enqueue(torch, ix, kmers, want_alive=True):
    """One txq_probe_device call on the current stream, not waited for: (masks, alive or None) device tensors."""
    n, W = kmers.size, ix.shard_words
    dk = torch.from_numpy(kmers.view(np.int64)).cuda()
    dm = torch.full((n, W), -1, dtype=torch.int64, device="cuda")
    da = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device="cuda") if want_alive else None
    ix.probe_device(dk.data_ptr(), n, dm.data_ptr(), da.data_ptr() if want_alive else None, torch.cuda.current_stream().cuda_stream)
    return dk, dm, da


def _calls(capi, torch, monkeypatch, width, h, words, batches, tile, alive=None, env=()):
    """The batches on a NEW index (the first call is a fresh one), under TXQ_PROBE_TABLE_TILE unset or =0: [(masks, alive or None)]."""
    monkeypatch.delenv("TXQ_PROBE_TABLE_KEEP", raising=False)
    monkeypatch.delenv("TXQ_PROBE_TABLE_FUSED", raising=False)
    monkeypatch.setenv("TXQ_PROBE_TABLE", "1")
    for name, value in env:
        monkeypatch.setenv(name, value)
    if tile:
        monkeypatch.delenv("TXQ_PROBE_TABLE_TILE", raising=False)
    else:
        monkeypatch.setenv("TXQ_PROBE_TABLE_TILE", "0")
    ix = _upload(capi, width, h, words)
    alive = alive or [True] * len(batches)
    got = [_enqueue(torch, ix, k, a) for k, a in zip(batches, alive)]
    torch.cuda.synchronize()
    out = [(dm.cpu().numpy().view(np.uint64), None if da is None else da.cpu().numpy().view(np.uint64)) for _, dm, da in got]
    ix.free()
    return out


def _check(capi, torch, monkeypatch, refs, width, h, batches, alive=None, env=()):
    words, ref = refs(capi, width, h)
    new = _calls(capi, torch, monkeypatch, width, h, words, batches, True, alive, env)
    old = _calls(capi, torch, monkeypatch, width, h, words, batches, False, alive, env)
    for i, (k, (m, a), (m0, a0)) in enumerate(zip(batches, new, old)):
        want = ref.masks(k)
        assert np.array_equal(m, want), (width, h, i, "masks against the oracle")
        assert np.array_equal(m, m0), (width, h, i, "masks against TXQ_PROBE_TABLE_TILE=0")
        if a is not None:
            assert np.array_equal(a, _alive_bits(want)), (width, h, i, "alive against the oracle")
            assert np.array_equal(a, a0), (width, h, i, "alive against TXQ_PROBE_TABLE_TILE=0")


def _with_fallback_tiles(k):
    """One k-mer at or above `valid` at lane 0 of tile 3, lane 63 of tile 7 and lane 31 of tile 11 (their neighbours stay whole),
    and tile 20 nothing but such k-mers."""
    k = k.copy()
    k[3 * 64] = FAR
    k[7 * 64 + 63] = FAR + np.uint64(1)
    k[11 * 64 + 31] = FAR + np.uint64(2)
    k[20 * 64:21 * 64] = FAR + np.arange(64, dtype=np.uint64) * np.uint64(977)
    return k


@pytest.mark.parametrize("h", [2, 3])
@pytest.mark.parametrize("width", list(WIDTHS))
def test_tiles(capi, torch, monkeypatch, refs, width, h):
    """A fresh call and a kept one over 4000 values (both build or read rows, and answer whole tiles from them), then on valid
    rows: a batch below 3000 (every full tile whole), the same with fallback tiles, with and without `alive`, and n = 63, 64,
    65 and 128 (no full tile, one, one and a ragged one, two)."""
    warm = _domain_batch(500, N, 4000)
    low = _domain_batch(501, N, 3000)
    mixed = _with_fallback_tiles(low)
    small = [_domain_batch(510 + n, n, 3000) for n in (63, 64, 65, 128)]
    batches = [warm, warm, low, mixed, mixed, low] + small + [_with_fallback_tiles(_domain_batch(502, 21 * 64, 3000))]
    alive = [True, True, True, True, False, False] + [True, False, True, True] + [True]
    _check(capi, torch, monkeypatch, refs, width, h, batches, alive)


@pytest.mark.parametrize("h", [2, 3])
@pytest.mark.parametrize("width", ["W16", "W10", "W32"])
def test_first_call_has_fallback_tiles(capi, torch, monkeypatch, refs, width, h):
    """The fresh call itself (sample, build, answer) on a batch with fallback tiles and a tile of misses."""
    mixed = _with_fallback_tiles(_domain_batch(520, N, 3000))
    _check(capi, torch, monkeypatch, refs, width, h, [mixed, mixed])


@pytest.mark.parametrize("width", ["W16", "W15", "W10", "W32"])
def test_growing_domains(capi, torch, monkeypatch, refs, width):
    """1000, then 3000 three times, then 16 000 three times: a launch answers whole tiles, gathers the new values in others and
    builds rows after its batch tiles."""
    batches = [_domain_batch(530 + i, N, d) for i, d in enumerate((1000, 3000, 3000, 3000, 16000, 16000, 16000))]
    _check(capi, torch, monkeypatch, refs, width, 3, batches)


@pytest.mark.parametrize("width", ["W16", "W10", "W32"])
def test_many_tiles_per_wave(capi, torch, monkeypatch, refs, width):
    """TXQ_PROBE_BLOCKS_PER_CU=1: 1024 waves stride over the tiles - 1095 of them, then 4689 (four or five per wave), whole
    tiles and fallback tiles in one wave's run."""
    warm = _domain_batch(540, N, 4000)
    big = _with_fallback_tiles(_domain_batch(541, 300000 + 17, 3000))
    big[(1024 + 5) * 64 + 9] = FAR  # the second tile of wave 5 at 1024 waves
    _check(capi, torch, monkeypatch, refs, width, 3, [warm, warm, _with_fallback_tiles(warm), big], env=(("TXQ_PROBE_BLOCKS_PER_CU", "1"),))
