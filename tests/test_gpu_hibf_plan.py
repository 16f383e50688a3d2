"""Ties the CPU fixture of the upload planner (test_hibf_plan.py, golden/hibf_plan_trees.json) to the real upload path: every
tree of the fixture goes through txq_index_upload / txq_index_upload_subtrees with all-zero IBFs; the index must report the
golden device_bytes, n_ibf and shard_words, answer 64 k-mers with all-zero masks — plainly and as a one-program session —
and be freed; every invalid tree must be refused with the golden code and text."""
import ctypes as C

import numpy as np
import pytest

from helpers import make_blob, splitmix64
from test_hibf_plan import load_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


def _upload(capi, case):
    """The case's tree with all-zero words (a null-map IBF as null pointers, which Index.upload_hibf cannot say)."""
    n = len(case["ibfs"])
    keep, descs, nxt, tbu = [], (capi.IbfDesc * n)(), (capi.u64p * n)(), (capi.u64p * n)()
    for i, f in enumerate(case["ibfs"]):
        w = np.zeros(f["bin_size"] * ((f["bins"] + 63) // 64), dtype=np.uint64)
        descs[i] = capi._ibf_desc(f["bins"], f["bin_size"], f["hash_funs"], w)
        keep.append(w)
        if f["next"] is not None:
            a, b = np.array(f["next"], dtype=np.uint64), np.array(f["tbu"], dtype=np.uint64)
            keep += [a, b]
            nxt[i], tbu[i] = a.ctypes.data_as(capi.u64p), b.ctypes.data_as(capi.u64p)
    desc = capi.IndexDesc(n, descs, nxt, tbu, case["user_bins"])
    h = C.c_void_p()
    entry = capi.lib().txq_index_upload_subtrees if case["mode"] else capi.lib().txq_index_upload
    capi.check(entry(C.byref(desc), case["rank"], case["n_shards"], C.byref(h)))
    return capi.Index(h.value)


def test_every_fixture_tree_uploads_as_planned_and_answers_nothing(capi, golden):
    expected = golden("hibf_plan_expected.json")
    kmers = splitmix64(1, 64) >> np.uint64(40)
    blob = make_blob(kmers, [(3, [(k, 2, 1, 2) for k in range(64)])])  # slot 2 |= ONES & M[k-mer] for each of them
    n_valid = 0
    for case in load_cases():
        want = expected[case["name"]]
        if want["rc"] != 0:
            with pytest.raises(capi.TxqError) as e:
                _upload(capi, case)
            assert (e.value.code, str(e.value)) == (want["rc"], "txq error %d: %s" % (want["rc"], want["error"])), case["name"]
            continue
        n_valid += 1
        ix = _upload(capi, case)
        got = (int(ix.info.device_bytes), int(ix.info.n_ibf), int(ix.info.shard_words), int(ix.info.shard_word0))
        assert got == (want["device_bytes"], want["n_ibf"], want["shard_words"], want["shard_word0"]), case["name"]
        masks = ix.probe(kmers)
        assert masks.shape == (64, want["shard_words"]) and not masks.any(), case["name"]
        sess = ix.session(1)
        sess.stage(blob)
        out = sess.end()
        assert out.shape == (1, want["shard_words"]) and not out.any(), case["name"]
        ix.free()
    assert n_valid >= 20
