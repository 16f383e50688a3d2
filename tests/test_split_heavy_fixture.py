"""The heavy-split tree of tests/helpers.py split_heavy_hibf has the shape the GPU tests rely on (tests/test_gpu_split_bins.py):
chunks whose split-bin entries number 64, 65, 127, 128 and more than 128, a chunk that starts inside a side word, 8-byte
chunks in the narrow variant, a heavy split three levels down — and every planted motif in its bins by the oracle.  CPU only:
the layout is recomputed by layout_split_chunks, the Python mirror of the upload rule."""
import numpy as np
import pytest

from helpers import MERGED, layout_split_chunks, split_heavy_hibf


def _depths(descs):
    depth = {0: 0}
    for i, d in enumerate(descs):  # (parents come before their children)
        for nxt, ub in zip(d["next_ibf_id"], d["tb_to_user"]):
            if int(ub) == MERGED:
                depth[int(nxt)] = depth[i] + 1
    return depth


@pytest.mark.parametrize("k", [4, 6])
@pytest.mark.parametrize("narrow", [False, True])
def test_the_heavy_split_tree_has_its_shape(oracle, narrow, k):
    ox, descs, values, planted = split_heavy_hibf(oracle, 3, k=k, narrow=narrow)
    assert descs[0]["bins"] == 256 and any(int(u) == MERGED for u in descs[0]["tb_to_user"])  # tmax = 256, gates below the root
    cwords, chunks = layout_split_chunks(descs)
    assert cwords == (1 if narrow else 2)
    counts = [len(c["entries"]) for c in chunks]
    for n in (64, 65, 127, 128):
        assert n in counts, n
    assert max(counts) >= 129
    assert any(c["bit0"] > 0 for c in chunks)
    # the root's heavy bin: its parts in all four words, its representative in the first chunk
    root = max((c for c in chunks if c["ibf"] == 0), key=lambda c: len(c["entries"]))
    assert root["chunk"] == 0 and len(root["entries"]) >= 199 and {tb >> 6 for _, tb in root["entries"]} == {0, 1, 2, 3}
    # two split bins whose representatives share a chunk, the higher one's entries reaching side bit 128 and beyond
    two = [c for c in chunks if len({ub for ub, _ in c["entries"]}) == 2 and len(c["entries"]) > 128]
    assert two and two[0]["entries"][-1][0] != two[0]["entries"][0][0]
    # a heavy split three levels down (kMaxVDepth ancestors)
    depth = _depths(descs)
    assert any(depth[c["ibf"]] == 3 and len(c["entries"]) > 128 for c in chunks)
    # every planted motif is in its bins by the oracle
    for motif, ubs in planted.items():
        want, quirks = ox.expected_mask(motif)
        assert quirks == 0
        for u in ubs:
            assert (int(want[u >> 6]) >> (u & 63)) & 1, (motif, u)
    assert len(values) == ox.bins and all(len(v) for v in values)


def test_the_mirror_matches_a_hand_computed_packing():
    """Per IBF its own side words: chunks of 2 and 3 entries share one (bit0 0 and 2); after a chunk of 69, the next chunk goes on in
    the same word at bit 5 (69 - 64); the second IBF starts again at bit 0."""
    def desc(split):
        tbu = [1000 + tb for tb in range(256)]
        for ub, tbs in split.items():
            for tb in tbs:
                tbu[tb] = ub
        return dict(bins=256, tb_to_user=np.array(tbu, dtype=np.uint64), next_ibf_id=np.zeros(256, dtype=np.uint64))
    cwords, chunks = layout_split_chunks([desc({1: [0, 1, 200], 2: [128, 129, 130, 131]}), desc({3: range(70), 4: [128, 129, 255]})])
    assert cwords == 2
    assert [(c["ibf"], c["chunk"], len(c["entries"]), c["bit0"]) for c in chunks] == [(0, 0, 2, 0), (0, 1, 3, 2), (1, 0, 69, 0), (1, 1, 2, 5)]
    assert chunks[0]["entries"] == [(1, 1), (1, 200)]  # (a part in another chunk still belongs to its representative's)
