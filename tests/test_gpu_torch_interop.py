"""libtxq.so inside a PyTorch-ROCm process: torch owns device memory and the stream
(plumbing), the HIP kernels of libtxq run on torch's stream against torch's buffers."""
import numpy as np
import pytest

from helpers import random_words, oracle_ibf_from_words, splitmix64

pytestmark = pytest.mark.gpu


def test_probe_on_torch_buffers_and_stream(oracle):
    import torch
    assert torch.cuda.is_available()
    from tetrex_amd import capi
    capi.init(0)
    bins, m, h, n = 1024, 4099, 3, 10000
    words = random_words(bins, m, 0.4, 3)
    ix = capi.Index.upload_ibf(bins, m, h, words)
    kmers = splitmix64(4, n) >> np.uint64(44)
    dk = torch.from_numpy(kmers.view(np.int64)).cuda()
    dm = torch.empty((n, ix.shard_words), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    ix.probe_device(dk.data_ptr(), n, dm.data_ptr(), None, stream)
    ev1.record()
    torch.cuda.synchronize()
    assert ev0.elapsed_time(ev1) > 0
    got = dm.cpu().numpy().view(np.uint64)
    want = oracle_ibf_from_words(oracle, bins, m, h, words).probe(kmers)
    assert np.array_equal(got, want)
    ix.free()


def test_no_device_memory_is_left_behind():
    """Indexes (flat and hierarchical), sessions, host-buffer probes and pinned buffers created and freed
    a few hundred times: the device's free memory (hipMemGetInfo through torch) ends where it started."""
    import torch
    import oracle as O
    from helpers import random_hibf
    from tetrex_amd import capi
    capi.init(0)
    words = random_words(300, 4099, 0.3, 1)
    ox, descs, values = random_hibf(O, 2, user_bins=120, levels=3)
    kmers = splitmix64(5, 5000) >> np.uint64(44)

    def cycle():
        ix = capi.Index.upload_ibf(300, 4099, 3, words)
        ix.probe(kmers)
        ix.query_masks(["LMAEG", "A.CD[EK]"], False, 4)
        ix.free()
        hx = capi.Index.upload_hibf(120, descs)
        hx.probe(kmers)
        hx.query_masks(["LMAEG"], False, 4)
        hx.free()
        hb = capi.HostBuffer((1000, 5))
        hb.free()
        db = capi.DeviceBuffer(1 << 20)
        db.free()

    for _ in range(5):
        cycle()
    torch.cuda.synchronize()
    free_before, _ = torch.cuda.mem_get_info()
    for _ in range(200):
        cycle()
    torch.cuda.synchronize()
    free_after, _ = torch.cuda.mem_get_info()
    assert free_before - free_after < (8 << 20), (free_before, free_after)


def other_owners_cycle(setenv, delenv):
    """What test_no_device_memory_is_left_behind_by_the_other_owners repeats (tests/perf_session_buffers.py times it, too);
    setenv / delenv: monkeypatch's, or os.environ's."""
    import oracle as O
    from blob_cases import MALFORMED
    from helpers import layout_hibf, make_blob, random_hibf, NO_KMER
    from motifs import random_prosite_motifs
    from tetrex_amd import capi
    capi.init(0)
    for name, value in {"TETREX_DENSE_EVIDENCE": "dense", "TETREX_DENSE_MIN": "1", "TETREX_DENSE_SPARSE_BELOW": "0", "TXQ_PROBE_TABLE": "1"}.items():
        setenv(name, value)  # lists become dense blocks (tests/test_gpu_dense.py); the domain table wherever it fits
    bins = 384
    words = random_words(bins, 4099, 0.3, 1)
    _, descs, _ = random_hibf(O, 2, user_bins=120, levels=3)
    _, general, _ = layout_hibf(O, 3, 200, tmax=64)
    assert any(np.unique(d["tb_to_user"][d["tb_to_user"] != capi.TXQ_MERGED_BIN], return_counts=True)[1].max() > 1 for d in general)  # split user bins
    kmers = splitmix64(5, 5000) >> np.uint64(44)
    more_kmers = splitmix64(6, 70000) >> np.uint64(44)
    offsets, thresholds = np.array([0, 2500, 5000], dtype=np.uint64), np.array([1, 2], dtype=np.uint32)
    begins, lens = np.array([0, 100, 400], dtype=np.uint64), np.array([200, 300, 64], dtype=np.uint32)
    motifs = random_prosite_motifs(20, 6)
    d_values = capi.DeviceBuffer.from_numpy(kmers[:64].copy())
    d_bins = capi.DeviceBuffer.from_numpy(np.arange(64, dtype=np.uint32))
    # stages of one program over n k-mers: 40 000 k-mers are more than a packed stage takes, 400 000 outgrow its blob buffer
    stage = lambda n: make_blob(splitmix64(n, n) >> np.uint64(44), [(4, [(0, 3, 1, 0), (n - 1, 3, 3, 0), (NO_KMER, 2, 3, 2)])])
    small, large = stage(40_000), stage(400_000)
    refused = MALFORMED["kind 4"]()

    def cycle():
        ix = capi.Index.upload_ibf(bins, 4099, 3, words)
        hx = capi.Index.upload_hibf(120, descs)
        for x in (ix, hx):
            x.count(kmers, offsets, thresholds, counts=True)
            x.count_windows(kmers, begins, lens, thresholds[[0, 1, 0]])
        ix.query_masks(motifs, False, 4)                 # builds the table of all k-mers' masks
        ix.emplace_device(d_values.ptr, d_bins.ptr, 64)  # ... which goes with the old bits
        ix.query_masks(motifs, False, 4)                 # ... and is built again
        ix.probe(kmers)
        ix.probe(more_kmers)                             # the domain table's rows grow
        s = ix.session(1)
        for blob in (small, small, large):               # the third stage has the first one's staging set
            s.stage(blob)
        s.end()
        setenv("TXQ_FINAL_PINNED", "0")
        s = ix.session(1)
        delenv("TXQ_FINAL_PINNED")
        s.stage(small)
        s.end()
        s = ix.session(3)
        with pytest.raises(capi.TxqError):
            s.stage(refused)
        with pytest.raises(capi.TxqError):               # (a session with a failed stage has no final masks; it is released all the same)
            s.end()
        gx = capi.Index.upload_hibf(200, general)
        gx.query_masks(motifs[:4], False, 4)
        for x in (ix, hx, gx):
            x.free()
    cycle.keep = (d_values, d_bins)
    return cycle


def test_no_device_memory_is_left_behind_by_the_other_owners(monkeypatch, capfd):
    """The same 5 + 200 cycles over what the test above does not reach: the count scratch, frontiers and host pipe (count and
    count_windows, flat and hierarchical); the table of all k-mers' masks, built by a session of 20 programs with dense steps,
    dropped by an emplace and built again; the flat probe's domain table, whose rows grow between two host-buffer probes; a
    general HIBF in layout order with split bins (side matrices at upload, the gathered rows of its sessions); a staging
    buffer that is outgrown and retired; final masks through the device buffer (TXQ_FINAL_PINNED=0); a session that ends
    after a refused stage."""
    import re
    import torch
    cycle = other_owners_cycle(monkeypatch.setenv, monkeypatch.delenv)
    monkeypatch.setenv("TXQ_TRACE", "1")  # once: the cycle does reach the table and does retire a staging buffer
    capfd.readouterr()
    cycle()
    trace = capfd.readouterr().err
    monkeypatch.delenv("TXQ_TRACE")
    assert trace.count("table of all") >= 2 and re.search(r"release: [1-9]\d* outgrown staging buffers freed", trace), trace[-4000:]
    for _ in range(4):
        cycle()
    torch.cuda.synchronize()
    free_before, _ = torch.cuda.mem_get_info()
    for _ in range(200):
        cycle()
    torch.cuda.synchronize()
    free_after, _ = torch.cuda.mem_get_info()
    assert free_before - free_after < (8 << 20), (free_before, free_after)
