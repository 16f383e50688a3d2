"""GPU parity of the flat probe's domain-table path (txq_probe.hip probe_flat): a batch whose k-mer values lie in a small
domain [0, D) is answered from a per-call table of the domain's masks instead of h row gathers per k-mer.

Every case runs the same batch under TXQ_PROBE_TABLE=1 (table whenever it fits), unset (automatic gate) and 0 (the plain
kernel) and compares masks and `alive` bit for bit with each other and with the CPU oracle.
"""
import numpy as np
import pytest

from helpers import random_words, oracle_ibf_from_words, splitmix64

pytestmark = pytest.mark.gpu

MODES = ("1", None, "0")


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _set_mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("TXQ_PROBE_TABLE", raising=False)
    else:
        monkeypatch.setenv("TXQ_PROBE_TABLE", mode)


def _oracle_masks(ox, kmers):
    """The oracle's masks of a batch with many repeats: probe each distinct value once."""
    uniq, inv = np.unique(kmers, return_inverse=True)
    return ox.probe(uniq)[inv.reshape(-1)]


def _alive_bits(masks):
    """Per 64-k-mer tile, bit i = row i of the tile is not all zero (txq_probe_device's d_alive)."""
    nz = (masks != 0).any(axis=1)
    nz = np.concatenate([nz, np.zeros((-nz.size) % 64, dtype=bool)]).reshape(-1, 64).astype(np.uint64)
    return (nz << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)


def _device_probe(torch, ix, kmers, monkeypatch, mode):
    _set_mode(monkeypatch, mode)
    n, W = kmers.size, ix.shard_words
    dk = torch.from_numpy(kmers.view(np.int64)).cuda()
    dm = torch.full((n, W), -1, dtype=torch.int64, device="cuda")
    da = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream()
    ix.probe_device(dk.data_ptr(), n, dm.data_ptr(), da.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    return dm.cpu().numpy().view(np.uint64), da.cpu().numpy().view(np.uint64)


def _check(capi, torch, oracle, monkeypatch, bins, bin_size, h, kmers, shards=1, density=0.35, seed=1):
    words = random_words(bins, bin_size, density, seed)
    ox = oracle_ibf_from_words(oracle, bins, bin_size, h, words)
    want = _oracle_masks(ox, kmers)
    cols = 0
    for r in range(shards):
        ix = capi.Index.upload_ibf(bins, bin_size, h, words, shard_rank=r, n_shards=shards)
        lo, nw = int(ix.info.shard_word0), ix.shard_words
        mine = want[:, lo:lo + nw]
        for mode in MODES:
            got, alive = _device_probe(torch, ix, kmers, monkeypatch, mode)
            assert np.array_equal(got, mine), (bins, h, kmers.size, shards, r, mode)
            assert np.array_equal(alive, _alive_bits(mine)), (bins, h, kmers.size, shards, r, mode)
        cols += nw
        ix.free()
    assert cols == (bins + 63) // 64


def _domain_batch(seed, n, domain):
    return splitmix64(seed, n) % np.uint64(domain)


@pytest.mark.parametrize("bins", [64, 65, 1024, 3000, 9000])
@pytest.mark.parametrize("h", [1, 2, 3, 4, 5])
def test_table_matches_oracle_every_hash_count_and_width(capi, torch, oracle, monkeypatch, bins, h):
    # n = 70000 over 4096 values: the automatic gate takes the table (17 repeats per value, capacity 17472 rows)
    _check(capi, torch, oracle, monkeypatch, bins, 4099, h, _domain_batch(bins + h, 70000, 4096), seed=bins * 7 + h)


@pytest.mark.parametrize("bins,shards", [(1024, 2), (1024, 3), (1000, 3), (3000, 17), (9000, 17)])
def test_table_column_shards(capi, torch, oracle, monkeypatch, bins, shards):
    # 1024 / 3: shards of 6, 5 and 5 words; 3000 / 17: shards of 2 and 3 words (odd shard_words, stride 4)
    _check(capi, torch, oracle, monkeypatch, bins, 2053, 3, _domain_batch(shards, 66000, 3000), shards=shards, seed=shards)


@pytest.mark.parametrize("n", [65537, 100003, 131071, 131072])
@pytest.mark.parametrize("domain_over_gate", [-1, 0, 1, 64])
def test_table_ragged_batches_around_the_gate(capi, torch, oracle, monkeypatch, n, domain_over_gate):
    # the automatic gate takes the table when about 4 * D k-mers lie below D (judged from a sample of the batch): domains just
    # below, at and above n / 4; values the sample missed (v >= D) take the gather inside the table path
    domain = n // 4 + domain_over_gate
    kmers = _domain_batch(n, n, domain)
    kmers[:8] = np.uint64(domain - 1)  # D is the domain itself
    _check(capi, torch, oracle, monkeypatch, 1024, 3001, 3, kmers, seed=n + domain)


def test_table_outliers_take_the_gather_inside_the_table_path(capi, torch, oracle, monkeypatch):
    kmers = _domain_batch(5, 80000, 1024)
    kmers[np.arange(37, 80000, 4099)] = (splitmix64(6, 20) >> np.uint64(20))[:kmers[37::4099].size]
    kmers[-1] = np.uint64(1) << np.uint64(63)
    _check(capi, torch, oracle, monkeypatch, 1024, 4099, 3, kmers, seed=5)
    _check(capi, torch, oracle, monkeypatch, 3000, 4099, 2, kmers, seed=6)


def test_table_host_batches_on_two_streams(capi, oracle, monkeypatch):
    bins, m, h = 1024, 8191, 3
    words = random_words(bins, m, 0.4, 11)
    ox = oracle_ibf_from_words(oracle, bins, m, h, words)
    kmers = _domain_batch(12, 3 * 262144 + 1234, 1 << 12)  # four chunks of txq_probe, alternating between its two streams
    want = _oracle_masks(ox, kmers)
    ix = capi.Index.upload_ibf(bins, m, h, words)
    for mode in MODES:
        _set_mode(monkeypatch, mode)
        assert np.array_equal(ix.probe(kmers), want), mode
    ix.free()


def test_table_sees_emplace_between_calls(capi, torch, oracle, monkeypatch):
    bins, m, h = 1024, 4099, 3
    ix = capi.Index.create_ibf(bins, m, h)
    kmers = _domain_batch(21, 70000, 2048)
    stream = torch.cuda.current_stream().cuda_stream

    def insert(seed, count):
        vals = _domain_batch(seed, count, 2048)
        bins_of = (splitmix64(seed + 1, count) % np.uint64(bins)).astype(np.uint32)
        dv = torch.from_numpy(vals.view(np.int64)).cuda()
        db = torch.from_numpy(bins_of.view(np.int32)).cuda()
        ix.emplace_device(dv.data_ptr(), db.data_ptr(), count, stream)
        torch.cuda.synchronize()

    insert(30, 3000)
    first, _ = _device_probe(torch, ix, kmers, monkeypatch, None)
    want = _oracle_masks(oracle_ibf_from_words(oracle, bins, m, h, ix.download_words_rows(m)), kmers)
    assert np.array_equal(first, want)
    insert(40, 3000)
    second, alive = _device_probe(torch, ix, kmers, monkeypatch, None)
    want2 = _oracle_masks(oracle_ibf_from_words(oracle, bins, m, h, ix.download_words_rows(m)), kmers)
    assert not np.array_equal(want, want2)
    assert np.array_equal(second, want2)
    assert np.array_equal(alive, _alive_bits(want2))
    ix.free()


def test_table_scaled_bench_shape(capi, torch, oracle, monkeypatch):
    """1024 bins, 20-bit values, n = 2^22 (the bench batch is 2^24): table and plain path agree on the whole batch on the
    device, and with the oracle on every distinct value of a sample."""
    bins, m, h, n = 1024, 1247045, 3, 1 << 22
    words = random_words(bins, m, 0.2, 31)
    ix = capi.Index.upload_ibf(bins, m, h, words)
    kmers = splitmix64(2, n) >> np.uint64(44)
    dk = torch.from_numpy(kmers.view(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    for mode in MODES:
        _set_mode(monkeypatch, mode)
        dm = torch.full((n, 16), -1, dtype=torch.int64, device="cuda")
        da = torch.full((n // 64,), -1, dtype=torch.int64, device="cuda")
        ix.probe_device(dk.data_ptr(), n, dm.data_ptr(), da.data_ptr(), stream)
        torch.cuda.synchronize()
        out[mode] = (dm, da)
    for mode in ("1", None):
        assert torch.equal(out[mode][0], out["0"][0]), mode
        assert torch.equal(out[mode][1], out["0"][1]), mode
    ox = oracle_ibf_from_words(oracle, bins, m, h, words)
    idx = np.unique(splitmix64(9, 20000) % np.uint64(n)).astype(np.int64)
    got = out[None][0][torch.from_numpy(idx).cuda()].cpu().numpy().view(np.uint64)
    assert np.array_equal(got, ox.probe(kmers[idx]))
    ix.free()
