"""GPU parity of the flat probe's domain table when it is KEPT with the index between calls (txq_probe.hip probe_flat): the
rows T[v] depend on the index's bits alone, so a call only extends the table ([built, D)), and txq_emplace_device, growth of
the table and TXQ_PROBE_TABLE_KEEP=0 start it over.

Every test is a SEQUENCE of calls on one index (the calls of a sequence are enqueued without a wait between them); every call's
masks and `alive` are compared bit for bit with the CPU oracle.  Every sequence runs with TXQ_PROBE_TABLE_KEEP unset and =0 and
with TXQ_PROBE_TABLE unset (automatic gate) and =1 (table whenever it fits).  Shape: 1024 bins x 4099 rows, h = 3, n about
70 000 — the smallest batches that reach the automatic gate's 2^14-row capacity (n / 4 = 17 472 rows)."""
import threading

import numpy as np
import pytest

from helpers import random_words, oracle_ibf_from_words, splitmix64
from test_gpu_probe_domain_table import _oracle_masks, _alive_bits, _domain_batch

pytestmark = pytest.mark.gpu

BINS, ROWS, H, N = 1024, 4099, 3, 70000
KNOBS = [(keep, table) for keep in (None, "0") for table in (None, "1")]
IDS = ["keep=%s,table=%s" % k for k in KNOBS]


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
def base(oracle):
    """The index most sequences run on: its words and its oracle (made once, never changed)."""
    words = random_words(BINS, ROWS, 0.35, 77)
    return words, oracle_ibf_from_words(oracle, BINS, ROWS, H, words)


@pytest.fixture(params=KNOBS, ids=IDS)
def knobs(request, monkeypatch):
    keep, table = request.param
    for name, value in (("TXQ_PROBE_TABLE_KEEP", keep), ("TXQ_PROBE_TABLE", table)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    return request.param


def _enqueue(torch, ix, kmers, stream=None):
    """One txq_probe_device call on `stream` (default: the current one), not waited for: (masks, alive) device tensors."""
    n, W = kmers.size, ix.shard_words
    dk = torch.from_numpy(kmers.view(np.int64)).cuda()
    dm = torch.full((n, W), -1, dtype=torch.int64, device="cuda")
    da = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device="cuda")
    stream = stream or torch.cuda.current_stream()
    ix.probe_device(dk.data_ptr(), n, dm.data_ptr(), da.data_ptr(), stream.cuda_stream)
    return dk, dm, da


def _same(got, want, what):
    _, dm, da = got
    assert np.array_equal(dm.cpu().numpy().view(np.uint64), want), what
    assert np.array_equal(da.cpu().numpy().view(np.uint64), _alive_bits(want)), what


def _run(torch, ix, ox, batches, what, cols=slice(None)):
    """The batches one after the other on the current stream, then every call against the oracle."""
    calls = [_enqueue(torch, ix, k) for k in batches]
    torch.cuda.synchronize()
    for i, (k, got) in enumerate(zip(batches, calls)):
        _same(got, _oracle_masks(ox, k)[:, cols], (what, i))


def _growing_domains(seed):
    """1024 -> 4096 -> 16 000 (extensions) -> 512 (nothing to build) -> values beyond the capacity and one at 2^63 (they gather)."""
    batches = [_domain_batch(seed + i, N, d) for i, d in enumerate((1024, 4096, 16000, 512))]
    last = _domain_batch(seed + 9, N, 2048)
    last[np.arange(37, N, 4099)] = (splitmix64(seed + 10, 20) >> np.uint64(20))[:last[37::4099].size]
    last[5] = np.uint64(17472)  # the first value beyond the automatic capacity
    last[-1] = np.uint64(1) << np.uint64(63)
    return batches + [last]


def test_steady_state(capi, torch, base, knobs):
    words, ox = base
    ix = capi.Index.upload_ibf(BINS, ROWS, H, words)
    k = _domain_batch(1, N, 4096)
    _run(torch, ix, ox, [k, k, k], knobs)
    ix.free()


def test_changing_domains(capi, torch, base, knobs):
    words, ox = base
    ix = capi.Index.upload_ibf(BINS, ROWS, H, words)
    _run(torch, ix, ox, _growing_domains(10), knobs)
    ix.free()


def test_refused_first(capi, torch, base, knobs):
    words, ox = base
    ix = capi.Index.upload_ibf(BINS, ROWS, H, words)
    wide = splitmix64(20, N) >> np.uint64(24)  # uniform 40-bit values: (almost) none below the capacity
    _run(torch, ix, ox, [wide, _domain_batch(21, N, 3000), wide], knobs)
    ix.free()


def test_capacity_growth(capi, torch, base, knobs):
    words, ox = base
    ix = capi.Index.upload_ibf(BINS, ROWS, H, words)
    # the second call needs 75 000 rows (=1: 300 032): the table is reallocated and must not believe the first call's `built`
    _run(torch, ix, ox, [_domain_batch(30, N, 16000), _domain_batch(31, 300000, 60000), _domain_batch(32, N, 16000)], knobs)
    ix.free()


@pytest.mark.parametrize("second_stream", [False, True])
def test_table_warm_then_emplace(capi, torch, oracle, knobs, second_stream):
    ix = capi.Index.create_ibf(BINS, ROWS, H)
    main = torch.cuda.current_stream()

    def insert(seed, count, stream):
        vals = _domain_batch(seed, count, 2048)
        bins_of = (splitmix64(seed + 1, count) % np.uint64(BINS)).astype(np.uint32)
        dv = torch.from_numpy(vals.view(np.int64)).cuda()
        db = torch.from_numpy(bins_of.view(np.int32)).cuda()
        ix.emplace_device(dv.data_ptr(), db.data_ptr(), count, stream.cuda_stream)
        return dv, db

    held = [insert(40, 3000, main)]
    k = [_domain_batch(41 + i, N, 2048) for i in range(3)]
    warm = [_enqueue(torch, ix, b) for b in k]  # three calls warm the table
    if second_stream:  # the emplace on another stream, ordered behind the probes and before the next ones by events only
        side, after_probes, after_emplace = torch.cuda.Stream(), torch.cuda.Event(), torch.cuda.Event()
        side.wait_stream(main)  # (the inputs of insert are made on the current stream)
        after_probes.record(main)
        side.wait_event(after_probes)
        with torch.cuda.stream(side):
            held.append(insert(50, 3000, side))
        after_emplace.record(side)
        main.wait_event(after_emplace)
    else:
        held.append(insert(50, 3000, main))
    later = [_enqueue(torch, ix, b) for b in (k[0], k[1])]
    torch.cuda.synchronize()
    after = oracle_ibf_from_words(oracle, BINS, ROWS, H, ix.download_words_rows(ROWS))
    for i, got in enumerate(later):
        _same(got, _oracle_masks(after, k[i]), (knobs, "after", i))
    # the warm calls saw the first insert alone: the same index made again up to there
    ix2 = capi.Index.create_ibf(BINS, ROWS, H)
    vals = _domain_batch(40, 3000, 2048)
    bins_of = (splitmix64(41, 3000) % np.uint64(BINS)).astype(np.uint32)
    dv, db = torch.from_numpy(vals.view(np.int64)).cuda(), torch.from_numpy(bins_of.view(np.int32)).cuda()
    ix2.emplace_device(dv.data_ptr(), db.data_ptr(), 3000, main.cuda_stream)
    torch.cuda.synchronize()
    before = oracle_ibf_from_words(oracle, BINS, ROWS, H, ix2.download_words_rows(ROWS))
    for i, got in enumerate(warm):
        _same(got, _oracle_masks(before, k[i]), (knobs, "warm", i))
    assert not np.array_equal(_oracle_masks(before, k[0]), _oracle_masks(after, k[0]))
    ix.free()
    ix2.free()


def test_two_indexes(capi, torch, oracle, base, knobs):
    words_a, ox_a = base
    words_b = random_words(BINS, ROWS, 0.3, 78)
    ox_b = oracle_ibf_from_words(oracle, BINS, ROWS, H, words_b)
    a = capi.Index.upload_ibf(BINS, ROWS, H, words_a)
    b = capi.Index.upload_ibf(BINS, ROWS, H, words_b)
    k = [_domain_batch(60 + i, N, d) for i, d in enumerate((2048, 8000, 4000))]
    calls = [(ox, b_, _enqueue(torch, ix, b_)) for b_ in k for ix, ox in ((a, ox_a), (b, ox_b))]
    torch.cuda.synchronize()
    a.free()  # its table's memory may be handed to the next index
    words_c = random_words(BINS, ROWS, 0.4, 79)
    ox_c = oracle_ibf_from_words(oracle, BINS, ROWS, H, words_c)
    c = capi.Index.upload_ibf(BINS, ROWS, H, words_c)
    calls += [(ox, b_, _enqueue(torch, ix, b_)) for b_ in k[:2] for ix, ox in ((c, ox_c), (b, ox_b))]
    torch.cuda.synchronize()
    for i, (ox, b_, got) in enumerate(calls):
        _same(got, _oracle_masks(ox, b_), (knobs, i))
    b.free()
    c.free()


def test_odd_shard_width(capi, torch, oracle, knobs):
    # 3000 bins = 47 words in 17 shards: shards of 3 words (rank 0) and 2 words (rank 16); stride 4 != shard_words 3
    bins, shards = 3000, 17
    words = random_words(bins, ROWS, 0.35, 80)
    ox = oracle_ibf_from_words(oracle, bins, ROWS, H, words)
    widths = set()
    for rank in (0, shards - 1):
        ix = capi.Index.upload_ibf(bins, ROWS, H, words, shard_rank=rank, n_shards=shards)
        lo, nw = int(ix.info.shard_word0), ix.shard_words
        widths.add(nw)
        _run(torch, ix, ox, _growing_domains(81 + rank), (knobs, rank), cols=slice(lo, lo + nw))
        ix.free()
    assert widths == {2, 3}


def test_host_path_twice(capi, base, knobs):
    words, ox = base
    ix = capi.Index.upload_ibf(BINS, ROWS, H, words)
    kmers = _domain_batch(90, 3 * 262144 + 1234, 1 << 12)  # four chunks of txq_probe, alternating between its two streams
    want = _oracle_masks(ox, kmers)
    for turn in range(2):
        assert np.array_equal(ix.probe(kmers), want), (knobs, turn)
    ix.free()


def test_two_threads_one_index(capi, torch, base, knobs):
    words, ox = base
    ix = capi.Index.upload_ibf(BINS, ROWS, H, words)
    batches = [[_domain_batch(100 + 10 * t + i, N, d) for i, d in enumerate(ds)] for t, ds in enumerate(((1024, 12000, 3000), (9000, 500, 16000)))]
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
            _same(got, _oracle_masks(ox, b), (knobs, t, i))
    ix.free()
