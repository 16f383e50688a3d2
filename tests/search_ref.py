"""numpy restatement of threshold membership (include/txq.h txq_count; seqan::hibf membership_for(values, threshold)).

Every IBF's bulk_contains comes from the oracle, built from the IBF's words as the oracle builds it
(helpers.oracle_ibf_from_words); this file adds the counting and the run walk of Hibf::descend (oracle/txo_ibf.hpp) with counts
in place of one bit.  Counts are added up chunk by chunk: it never holds the masks of more than `chunk` values at once.
Results are unsharded: hits (n_queries, mask_words) uint64 and counts (n_queries, 64 * mask_words) int64."""
import numpy as np

from helpers import MERGED, oracle_ibf_from_words

CHUNK = 4096


def unpack(masks):
    """(n, W) uint64 -> (n, 64 W) uint8 bits, bit b of word w at column 64 w + b."""
    m = np.ascontiguousarray(masks, dtype="<u8")
    return np.unpackbits(m.view(np.uint8).reshape(m.shape[0], -1), axis=1, bitorder="little")


def pack(bits):
    """(n, 64 W) bool -> (n, W) uint64."""
    b = np.ascontiguousarray(bits, dtype=np.uint8)
    return np.packbits(b, axis=1, bitorder="little").view("<u8").reshape(b.shape[0], -1).copy()


def count_on(ox, values, offsets, queries=None, chunk=CHUNK):
    """counts[i][b] = how many values of query queries[i] have bit b in the oracle IBF's bulk_contains."""
    offsets = np.asarray(offsets, dtype=np.int64)
    queries = np.arange(offsets.size - 1) if queries is None else np.asarray(queries, dtype=np.int64)
    lens = offsets[queries + 1] - offsets[queries]
    out = np.zeros((queries.size, 64 * ox.words_per_mask), dtype=np.int64)
    if queries.size == 0 or lens.sum() == 0:
        return out
    idx = np.concatenate([np.arange(offsets[q], offsets[q + 1]) for q in queries])  # value positions, query by query
    owner = np.repeat(np.arange(queries.size), lens)                                 # row of `out` each belongs to
    for a in range(0, idx.size, chunk):
        b = min(a + chunk, idx.size)
        bits = unpack(ox.probe(np.asarray(values, dtype=np.uint64)[idx[a:b]])).astype(np.int64)
        rows = owner[a:b]
        starts = np.flatnonzero(np.r_[True, rows[1:] != rows[:-1]])
        out[rows[starts]] += np.add.reduceat(bits, starts, axis=0)
    return out


def flat_search(ox, bins, values, offsets, thresholds):
    counts = count_on(ox, values, offsets)
    t = np.asarray(thresholds, dtype=np.int64)[:, None]
    hits = counts >= t
    hits[:, bins:] = False
    return pack(hits), counts


class TreeRef:
    """An HIBF as upload descriptors (dicts of bins, bin_size, hash_funs, words, next_ibf_id, tb_to_user)."""

    def __init__(self, O, user_bins, descs):
        self.user_bins = user_bins
        self.descs = descs
        self.ox = [oracle_ibf_from_words(O, d["bins"], d["bin_size"], d["hash_funs"], d["words"]) for d in descs]
        self.segs = []
        for d in descs:  # segments of the walk: every merged bin alone, every run of one user bin
            tbu = np.asarray(d["tb_to_user"], dtype=np.uint64)
            merged = tbu == np.uint64(MERGED)
            new = np.ones(tbu.size, dtype=bool)
            new[1:] = merged[1:] | merged[:-1] | (tbu[1:] != tbu[:-1])
            starts = np.flatnonzero(new)
            self.segs.append((starts, merged[starts], tbu[starts], np.asarray(d["next_ibf_id"], dtype=np.int64)[starts]))

    def search(self, values, offsets, thresholds):
        nq = len(offsets) - 1
        W = (self.user_bins + 63) // 64
        counts = np.zeros((nq, 64 * W), dtype=np.int64)
        hits = np.zeros((nq, 64 * W), dtype=bool)
        t = np.asarray(thresholds, dtype=np.int64)
        level = {0: np.arange(nq)}  # IBF -> queries that visit it, level by level
        self.level_pairs = []       # (query, IBF) pairs of this descent on every level
        while level:
            self.level_pairs.append(sum(len(qs) for qs in level.values()))
            nxt = {}
            for i, qs in level.items():
                c = count_on(self.ox[i], values, offsets, qs)[:, :self.descs[i]["bins"]]
                starts, merged, ub, child = self.segs[i]
                sums = np.add.reduceat(c, starts, axis=1)
                for s in range(starts.size):
                    passed = sums[:, s] >= t[qs]
                    if merged[s]:
                        if passed.any():
                            nxt.setdefault(int(child[s]), []).append(qs[passed])
                    else:  # (a user bin whose parts are not adjacent has several runs: a hit if any run passes, its count the largest)
                        counts[qs, int(ub[s])] = np.maximum(counts[qs, int(ub[s])], sums[:, s])
                        hits[qs, int(ub[s])] |= passed
            level = {i: np.sort(np.concatenate(v)) for i, v in nxt.items()}
        return pack(hits), counts


def csr(queries):
    """list of value arrays -> (values, offsets)"""
    lens = [len(q) for q in queries]
    offsets = np.zeros(len(queries) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    values = np.concatenate([np.asarray(q, dtype=np.uint64) for q in queries]) if queries and sum(lens) else np.zeros(0, dtype=np.uint64)
    return values, offsets
