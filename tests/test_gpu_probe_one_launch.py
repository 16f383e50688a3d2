"""GPU parity of the flat probe's domain table when a call on KEPT rows is ONE launch (txq_probe.hip probe_kernel<..., kAnswer>):
the answer counts the k-mers it had to gather, and the NEXT call builds their rows inside its own launch, so an extension is
read two calls after the domain grew.  In between every mask must still be right - a k-mer at or above the valid rows is gathered.

Every test is a SEQUENCE of calls on one index, enqueued without a wait between them; every call's masks and `alive` are compared
bit for bit with the CPU oracle.  Every sequence runs with TXQ_PROBE_TABLE_FUSED unset and =0 (kept calls in three launches)
and with TXQ_PROBE_TABLE unset (automatic gate) and =1.  Shapes as in test_gpu_probe_table_kept.py: 4099 rows, h = 3, n about
70 000 (capacity 17 472 rows under the automatic gate, 69 952 under =1)."""
import threading

import numpy as np
import pytest

from helpers import random_words, oracle_ibf_from_words, splitmix64
from test_gpu_probe_domain_table import _oracle_masks, _alive_bits, _domain_batch
from test_gpu_probe_table_kept import _enqueue, _same

pytestmark = pytest.mark.gpu

BINS, ROWS, H, N = 1024, 4099, 3, 70000
TOP = 60000  # the reference holds the oracle's mask of every value below it, made once per index
KNOBS = [(fused, table) for fused in (None, "0") for table in (None, "1")]
IDS = ["fused=%s,table=%s" % k for k in KNOBS]


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


class _Ref:
    """The oracle's masks of one index: the values below `top` from a table made once (never changed), others one by one."""

    def __init__(self, ox, top, cols=slice(None)):
        self.ox, self.top, self.cols = ox, top, cols
        self.table = ox.probe(np.arange(top, dtype=np.uint64))[:, cols]

    def masks(self, kmers):
        small = kmers < np.uint64(self.top)
        out = np.empty((kmers.size, self.table.shape[1]), dtype=np.uint64)
        out[small] = self.table[kmers[small].astype(np.int64)]
        if not small.all():
            out[~small] = _oracle_masks(self.ox, kmers[~small])[:, self.cols]
        return out


@pytest.fixture(scope="module")
def base(oracle):
    """The index most sequences run on: its words and its reference."""
    words = random_words(BINS, ROWS, 0.35, 77)
    return words, _Ref(oracle_ibf_from_words(oracle, BINS, ROWS, H, words), TOP)


def _setenv(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


@pytest.fixture(params=KNOBS, ids=IDS)
def knobs(request, monkeypatch):
    fused, table = request.param
    monkeypatch.delenv("TXQ_PROBE_TABLE_KEEP", raising=False)
    _setenv(monkeypatch, "TXQ_PROBE_TABLE_FUSED", fused)
    _setenv(monkeypatch, "TXQ_PROBE_TABLE", table)
    return request.param


def _run(torch, ix, ref, batches, what):
    """The batches one after the other on the current stream, then every call against the reference."""
    calls = [_enqueue(torch, ix, k) for k in batches]
    torch.cuda.synchronize()
    for i, (k, got) in enumerate(zip(batches, calls)):
        _same(got, ref.masks(k), (what, i))


def _grown_domains(seed):
    """1000, then 3000 three times, then 16 000 three times: V and E are no multiples of 64, an extension is read two calls late."""
    return [_domain_batch(seed + i, N, d) for i, d in enumerate((1000, 3000, 3000, 3000, 16000, 16000, 16000))]


def _wide(seed, n=N):
    return splitmix64(seed, n) >> np.uint64(24)  # uniform 40-bit values: (almost) none below the capacity


def test_steady_state(capi, torch, base, knobs):
    words, ref = base
    ix = capi.Index.upload_ibf(BINS, ROWS, H, words)
    k = _domain_batch(1, N, 4096)
    _run(torch, ix, ref, [k, k, k, k, k], knobs)
    ix.free()


def test_growing_domains(capi, torch, base, knobs):
    words, ref = base
    ix = capi.Index.upload_ibf(BINS, ROWS, H, words)
    _run(torch, ix, ref, _grown_domains(10), knobs)
    ix.free()


def _sample_heads(n):
    """The positions the domain pass of a batch of n k-mers reads: the first 1/16 of each of its segments (txq_probe.hip)."""
    segs = min(max(n // 1024, 1), 512)
    mask = np.zeros(n, dtype=bool)
    for seg in range(segs):
        lo, hi = n * seg // segs, n * (seg + 1) // segs
        mask[lo:lo + (hi - lo + 15) // 16] = True
    return mask


@pytest.mark.parametrize("fused", [None, "0"])
@pytest.mark.parametrize("sample_misses", [False, True])
def test_small_batch_builds_many_rows(capi, torch, base, monkeypatch, sample_misses, fused):
    """Under TXQ_PROBE_TABLE=1: a large batch over 60 000 values, a small one over 512, a small one over 60 000.  sample_misses:
    the first batch's sampled positions hold values below 1000 only, so the first call builds 1000 rows and COUNTS the rest, and
    the second call - small, its own domain tiny - builds 59 000 rows in its one launch."""
    monkeypatch.delenv("TXQ_PROBE_TABLE_KEEP", raising=False)
    monkeypatch.setenv("TXQ_PROBE_TABLE", "1")
    _setenv(monkeypatch, "TXQ_PROBE_TABLE_FUSED", fused)
    words, ref = base
    ix = capi.Index.upload_ibf(BINS, ROWS, H, words)
    first = _domain_batch(20, 300000, TOP)
    if sample_misses:
        heads = _sample_heads(first.size)
        first[heads] %= np.uint64(1000)
    _run(torch, ix, ref, [first, _domain_batch(21, N, 512), _domain_batch(22, N, TOP)], (fused, sample_misses))
    ix.free()


def test_miss_then_plain_then_extend(capi, torch, base, knobs):
    words, ref = base
    ix = capi.Index.upload_ibf(BINS, ROWS, H, words)
    # a call with no value below its capacity, one of n = 1000 (the plain kernel under the automatic gate), two that extend and read
    _run(torch, ix, ref, [_wide(30), _domain_batch(31, 1000, 3000), _domain_batch(32, N, 3000), _domain_batch(33, N, 3000),
                          _domain_batch(34, N, 3000)], knobs)
    ix.free()


def test_miss_then_emplace(capi, torch, oracle, knobs):
    ix = capi.Index.create_ibf(BINS, ROWS, H)
    main = torch.cuda.current_stream()

    def insert(seed, count):
        vals = _domain_batch(seed, count, 2048)
        bins_of = (splitmix64(seed + 1, count) % np.uint64(BINS)).astype(np.uint32)
        dv = torch.from_numpy(vals.view(np.int64)).cuda()
        db = torch.from_numpy(bins_of.view(np.int32)).cuda()
        ix.emplace_device(dv.data_ptr(), db.data_ptr(), count, main.cuda_stream)
        return dv, db

    held = [insert(40, 3000)]
    k = [_domain_batch(41, N, 2048), _domain_batch(42, N, 2048)]
    miss = _enqueue(torch, ix, _wide(43))
    warm = _enqueue(torch, ix, k[0])  # counts [0, 2048) - the rows it would have the next call build belong to the old bits
    held.append(insert(50, 3000))
    later = [_enqueue(torch, ix, b) for b in (k[0], k[1], k[0])]
    torch.cuda.synchronize()
    after = oracle_ibf_from_words(oracle, BINS, ROWS, H, ix.download_words_rows(ROWS))
    for i, (b, got) in enumerate(zip((k[0], k[1], k[0]), later)):
        _same(got, _oracle_masks(after, b), (knobs, "after", i))
    assert not np.array_equal(warm[1].cpu().numpy(), later[0][1].cpu().numpy())  # the insert changed masks of this batch
    del miss, held
    ix.free()


def test_values_around_the_capacity_in_a_kept_call(capi, torch, base, knobs):
    words, ref = base
    ix = capi.Index.upload_ibf(BINS, ROWS, H, words)
    batches = [_domain_batch(60 + i, N, 4096) for i in range(4)]
    for b in batches[1:]:  # kept calls; capacities: 17 472 rows (automatic gate), 69 952 (TXQ_PROBE_TABLE=1)
        for j, v in enumerate((17472, 17471, 69952, 69951, 1 << 63, (1 << 64) - 1, 1 << 32, (1 << 32) + 5)):
            b[100 + 977 * j] = np.uint64(v)
    _run(torch, ix, ref, batches, knobs)
    ix.free()


@pytest.mark.parametrize("table", [None, "1"])
def test_fused_and_unfused_calls_alternate(capi, torch, base, monkeypatch, table):
    """One index, the knob re-read per call as the library does: one-launch and three-launch calls follow each other."""
    monkeypatch.delenv("TXQ_PROBE_TABLE_KEEP", raising=False)
    _setenv(monkeypatch, "TXQ_PROBE_TABLE", table)
    words, ref = base
    ix = capi.Index.upload_ibf(BINS, ROWS, H, words)
    batches = [_domain_batch(70 + i, N, d) for i, d in enumerate((1000, 3000, 3000, 9000, 9000, 9000, 16000, 16000, 500, 16000))]
    calls = []
    for i, k in enumerate(batches):
        _setenv(monkeypatch, "TXQ_PROBE_TABLE_FUSED", "0" if i % 3 == 1 or i == 6 else None)
        calls.append(_enqueue(torch, ix, k))
    torch.cuda.synchronize()
    for i, (k, got) in enumerate(zip(batches, calls)):
        _same(got, ref.masks(k), (table, i))
    ix.free()


def test_two_streams_two_threads_one_index(capi, torch, base, knobs):
    words, ref = base
    ix = capi.Index.upload_ibf(BINS, ROWS, H, words)
    batches = [[_domain_batch(100 + 10 * t + i, N, d) for i, d in enumerate(ds)] for t, ds in enumerate(((1024, 12000, 3000, 12000), (9000, 500, 16000, 16000)))]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    calls, errors = [[], []], []
    start = threading.Barrier(2)

    def work(t):
        try:
            with torch.cuda.stream(streams[t]):
                start.wait(timeout=60)
                for b in batches[t]:
                    calls[t].append(_enqueue(torch, ix, b, streams[t]))
                streams[t].synchronize()
        except Exception as e:  # noqa: BLE001 (reported below, on the main thread)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for t in range(2):
        assert len(calls[t]) == len(batches[t])
        for i, (b, got) in enumerate(zip(batches[t], calls[t])):
            _same(got, ref.masks(b), (knobs, t, i))
    ix.free()


WIDTHS = [(128, 1, 0), (2112, 1, 0), (3000, 17, 0), (3000, 17, 16)]  # bins, shards, rank (1024 bins: every test above)


@pytest.fixture(scope="module")
def width_refs(oracle):
    """Per width its words and reference, made on first use and shared by the knob settings."""
    made = {}

    def get(bins, shards, rank, ix):
        key = (bins, shards, rank)
        if key not in made:
            words = random_words(bins, ROWS, 0.35, 80 + bins)
            made[key] = (words, None)
        if ix is not None and made[key][1] is None:
            lo, nw = int(ix.info.shard_word0), ix.shard_words
            made[key] = (made[key][0], _Ref(oracle_ibf_from_words(oracle, bins, ROWS, H, made[key][0]), 16000, slice(lo, lo + nw)))
        return made[key]
    return get


@pytest.mark.parametrize("bins,shards,rank", WIDTHS)
def test_widths(capi, torch, width_refs, knobs, bins, shards, rank):
    # 128 bins: stride 2; 2112 bins: 33 words, stride 34; 3000 bins over 17 shards: 3 words (rank 0) and 2 words (rank 16), stride 4 != 3
    words, _ = width_refs(bins, shards, rank, None)
    ix = capi.Index.upload_ibf(bins, ROWS, H, words, shard_rank=rank, n_shards=shards)
    assert ix.shard_words == {(128, 0): 2, (2112, 0): 33, (3000, 0): 3, (3000, 16): 2}[(bins, rank)]
    _, ref = width_refs(bins, shards, rank, ix)
    _run(torch, ix, ref, _grown_domains(90 + bins + rank), (knobs, bins, rank))
    ix.free()
