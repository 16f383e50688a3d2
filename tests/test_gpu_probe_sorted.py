"""GPU parity of the flat probe's sorted answer (txq_probe.hip: probe_sort_count / _scan / _scatter_kernel in front of
probe_kernel<..., kAnswer>, txq_probe_plan.hpp plan_probe_sort): a one-launch call on kept rows, without `alive`, whose batch is
first partitioned into value buckets and then answered in bucket order.

Shape: 1024 bins x 4099 rows, h = 3, values below 2^12.  TXQ_PROBE_TABLE=1 gives the table 65 536 rows, buckets of 32 KiB
(TXQ_PROBE_SORT_BUCKET_KB=32: 2^8 rows) make 256 of them, of which the values use 16, and TXQ_PROBE_SORT_MIN=1 sends every batch
there.  Every call's masks are compared bit for bit with the same index under TXQ_PROBE_TABLE=0 (the plain kernel), one case
with the CPU oracle as well; which path ran is read from Index.probe_sorted(): (calls that partitioned, answers in bucket order)."""
import numpy as np
import pytest

from helpers import random_words, oracle_ibf_from_words, splitmix64
from test_gpu_probe_domain_table import _oracle_masks, _alive_bits

pytestmark = pytest.mark.gpu

BINS, ROWS, H, DOMAIN = 1024, 4099, 3, 1 << 12
ENV = {"TXQ_PROBE_TABLE": "1", "TXQ_PROBE_SORT": "1", "TXQ_PROBE_SORT_MIN": "1", "TXQ_PROBE_SORT_BUCKET_KB": "32"}


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
def words():
    return random_words(BINS, ROWS, 0.35, 177)


@pytest.fixture
def sort_env(monkeypatch):
    for name, value in ENV.items():
        monkeypatch.setenv(name, value)
    return monkeypatch


def _values(seed, n, domain=DOMAIN, lo=0):
    return (splitmix64(seed, n) % np.uint64(domain - lo)) + np.uint64(lo)


def _enqueue(torch, ix, kmers, alive=False, stream=None):
    n, W = kmers.size, ix.shard_words
    dk = torch.from_numpy(kmers.view(np.int64)).cuda()
    dm = torch.full((n, W), -1, dtype=torch.int64, device="cuda")
    da = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device="cuda") if alive else None
    stream = stream or torch.cuda.current_stream()
    ix.probe_device(dk.data_ptr(), n, dm.data_ptr(), da.data_ptr() if alive else None, stream.cuda_stream)
    return dk, dm, da


def _masks(torch, ix, kmers, **kw):
    _, dm, da = _enqueue(torch, ix, kmers, **kw)
    torch.cuda.synchronize()
    return dm.cpu().numpy().view(np.uint64), (da.cpu().numpy().view(np.uint64) if da is not None else None)


def _plain(torch, ix, kmers, env):
    """The same index under TXQ_PROBE_TABLE=0: the plain kernel (it does not touch the table)."""
    env.setenv("TXQ_PROBE_TABLE", "0")
    got, _ = _masks(torch, ix, kmers)
    env.setenv("TXQ_PROBE_TABLE", "1")
    return got


def _warm(torch, ix, domain=DOMAIN):
    """A fresh call that builds the rows [0, domain): every later call is kept."""
    k = np.arange(domain, dtype=np.uint64).repeat(2)
    k[0] = np.uint64(domain - 1)  # (the domain pass samples the head of the batch: it must see the largest value)
    _masks(torch, ix, k)
    assert ix.probe_sorted() == (0, 0)  # a fresh call is never sorted


@pytest.mark.parametrize("n", [64, 65, 4095, 4097, 3 * 4096 + 17])
def test_sizes(capi, torch, words, sort_env, n):
    ix = capi.Index.upload_ibf(BINS, ROWS, H, words)
    _warm(torch, ix)
    k = _values(n, n)
    got, _ = _masks(torch, ix, k)
    assert ix.probe_sorted() == (1, 1)
    assert np.array_equal(got, _plain(torch, ix, k, sort_env)), n
    ix.free()


def test_oracle(capi, torch, oracle, words, sort_env):
    ox = oracle_ibf_from_words(oracle, BINS, ROWS, H, words)
    ix = capi.Index.upload_ibf(BINS, ROWS, H, words)
    _warm(torch, ix)
    k = _values(7, 2 * 4096 + 100)
    got, _ = _masks(torch, ix, k)
    assert ix.probe_sorted() == (1, 1)
    assert np.array_equal(got, _oracle_masks(ox, k))
    ix.free()


def test_all_equal_and_two_buckets(capi, torch, words, sort_env):
    ix = capi.Index.upload_ibf(BINS, ROWS, H, words)
    _warm(torch, ix)
    same = np.full(4096 + 300, 1234, dtype=np.uint64)
    # buckets 2 (values 512..767) and 15 (3840..4095) only: every other bucket is empty
    two = np.where(splitmix64(8, 9000) & np.uint64(1), _values(9, 9000, 768, 512), _values(10, 9000, 4096, 3840))
    assert set((two >> np.uint64(8)).tolist()) == {2, 15}
    for i, k in enumerate((same, two)):
        got, _ = _masks(torch, ix, k)
        assert ix.probe_sorted() == (i + 1, i + 1)
        assert np.array_equal(got, _plain(torch, ix, k, sort_env)), i
    ix.free()


def test_extension_across_calls(capi, torch, words, sort_env):
    """fresh (rows [0, 1024)) -> kept with values up to 4096 (in batch order: it counts them) -> kept below 1024 (sorted, and the
    launch builds [1024, 4096) from the statistics of the call before) -> kept up to 4096 (sorted: the rows are there)."""
    ix = capi.Index.upload_ibf(BINS, ROWS, H, words)
    _warm(torch, ix, 1024)
    batches = [_values(20, 9000, 4096), _values(21, 9000, 1024), _values(22, 9000, 4096), _values(23, 5000, 4096)]
    calls = [_enqueue(torch, ix, k) for k in batches]  # enqueued without a wait between them
    torch.cuda.synchronize()
    assert ix.probe_sorted() == (4, 3)
    for i, (k, (_, dm, _)) in enumerate(zip(batches, calls)):
        assert np.array_equal(dm.cpu().numpy().view(np.uint64), _plain(torch, ix, k, sort_env)), i
    # the same sequence with TXQ_PROBE_SORT=0 extends the table by the same calls: a last sorted call finds the same rows valid
    ix2 = capi.Index.upload_ibf(BINS, ROWS, H, words)
    _warm(torch, ix2, 1024)
    sort_env.setenv("TXQ_PROBE_SORT", "0")
    for k in batches[:2]:
        _masks(torch, ix2, k)
    sort_env.setenv("TXQ_PROBE_SORT", "1")
    got, _ = _masks(torch, ix2, batches[2])
    assert ix2.probe_sorted() == (1, 1)
    assert np.array_equal(got, _plain(torch, ix2, batches[2], sort_env))
    ix.free()
    ix2.free()


def test_one_kmer_outside(capi, torch, words, sort_env):
    ix = capi.Index.upload_ibf(BINS, ROWS, H, words)
    _warm(torch, ix)
    for i, bad in enumerate((DOMAIN, 1 << 40)):  # the first value without a row; a value beyond 32 bits
        k = _values(30 + i, 2 * 4096 + 5)
        k[4321] = np.uint64(bad)
        got, _ = _masks(torch, ix, k)
        assert ix.probe_sorted() == (i + 1, 0)  # partitioned, answered in batch order
        assert np.array_equal(got, _plain(torch, ix, k, sort_env)), bad
    ix.free()


def test_alive_takes_the_batch_order(capi, torch, words, sort_env):
    ix = capi.Index.upload_ibf(BINS, ROWS, H, words)
    _warm(torch, ix)
    k = _values(40, 4096 + 70)
    got, alive = _masks(torch, ix, k, alive=True)
    assert ix.probe_sorted() == (0, 0)
    want = _plain(torch, ix, k, sort_env)
    assert np.array_equal(got, want)
    assert np.array_equal(alive, _alive_bits(want))
    ix.free()


def test_2048_bins(capi, torch, sort_env):
    w = random_words(2048, ROWS, 0.35, 178)
    ix = capi.Index.upload_ibf(2048, ROWS, H, w)
    assert ix.shard_words == 32  # LPK 16
    _warm(torch, ix)
    for i, n in enumerate((4097, 64 * 3 + 1)):
        k = _values(50 + i, n)
        got, _ = _masks(torch, ix, k)
        assert ix.probe_sorted() == (i + 1, i + 1)
        assert np.array_equal(got, _plain(torch, ix, k, sort_env)), n
    ix.free()


def test_odd_words_never_sorted(capi, torch, sort_env):
    bins = 15 * 64  # 15 mask words in rows of 16
    w = random_words(bins, ROWS, 0.35, 179)
    ix = capi.Index.upload_ibf(bins, ROWS, H, w)
    assert ix.shard_words == 15
    _warm(torch, ix)
    k = _values(60, 4097)
    got, _ = _masks(torch, ix, k)
    assert ix.probe_sorted() == (0, 0)
    assert np.array_equal(got, _plain(torch, ix, k, sort_env))
    ix.free()


def test_two_streams(capi, torch, words, sort_env):
    ix = capi.Index.upload_ibf(BINS, ROWS, H, words)
    _warm(torch, ix)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    batches = [_values(70, 3 * 4096 + 1), _values(71, 4096 - 1)]  # (the second call's scratch is the first call's)
    torch.cuda.synchronize()
    calls = []
    for s, k in zip(streams, batches):
        with torch.cuda.stream(s):
            calls.append(_enqueue(torch, ix, k, stream=s))
    torch.cuda.synchronize()
    assert ix.probe_sorted() == (2, 2)
    for k, (_, dm, _) in zip(batches, calls):
        assert np.array_equal(dm.cpu().numpy().view(np.uint64), _plain(torch, ix, k, sort_env))
    ix.free()
