"""The sessions of golden/exec_plan_sessions.json — what tests/test_exec_plan.py plans on the CPU — through a device session on
the 130-bin index of tests/blob_cases.py, beside helpers.SessionSimulator: the alive bytes of every stage and the final masks.
This ties the CPU fixture to the real path: the planned lists are what the kernels of these very stages read."""
import numpy as np
import pytest

import blob_cases
from test_exec_plan import load_fixture

pytestmark = pytest.mark.gpu


def test_fixture_sessions_on_the_device(oracle, monkeypatch):
    from tetrex_amd import capi
    capi.init(0)
    for k in ("TXQ_KMER_TABLE_MIN", "TXQ_DENSE_TREE", "TXQ_HIBF_LAYOUT_ORDER", "TXQ_FUSE_UNITS", "TXQ_SPARSE_STEPS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("TXQ_KMER_TABLE_MB", "0")  # dense steps take their rows from the index itself
    ox = blob_cases.small_oracle_index(oracle)
    bins, m, h = blob_cases.SMALL_INDEX
    ix = capi.Index.upload_ibf(bins, m, h, blob_cases.small_index_words())
    try:
        # (in the fixture's order: a session finds the blocks the one before it left with the index, as in the CPU cases)
        for name, stages in load_fixture()["sessions"].items():
            want_alive, want = blob_cases.simulate(ox, stages)
            s = ix.session(len(want))
            for st, (blob, qp, qs) in enumerate(stages):
                got = s.stage(blob, np.array(qp, dtype=np.uint32), np.array(qs, dtype=np.uint32), raw=True)
                assert got.tolist() == want_alive[st].tolist(), (name, st)
            got = s.end()
            assert got.shape == want.shape and np.array_equal(got, want), (name, np.flatnonzero((got != want).any(axis=1))[:12])
    finally:
        ix.free()
