"""The yardstick of the per-record hit list (include/txq.h txq_edit_targets_device, include/txh.h txh_edit_targets): the hits
of a pair are what a search that existed before them answers when every record is a group of its own.  `expand` makes those
pairs, `hits_of` turns their (distance, record, end) answers into the ordered list (pair, distance, record, end), and
`least` is the consistency rule: the least hit of every pair, which the search calls answer on the real groups."""
import numpy as np

NONE = 0xFFFFFFFF


def expand(groups, pairs):
    """(one-record groups, pairs (pattern, record, cap) for every record of every pair's group, owner: the pair of each)"""
    single, owner = [], []
    for i, (p, g, e) in enumerate(pairs):
        for r in range(int(groups[g]), int(groups[g + 1])):
            single.append((p, r, e))
            owner.append(i)
    n_records = int(max(groups)) if len(groups) else 0
    return list(range(n_records + 1)), single, np.asarray(owner, dtype=np.int64)


def hits_of(results, owner):
    """the (n, 3) answers of the expanded pairs as the hit list: (owner, d, r, j) of those that are not NONE, in order"""
    results = np.asarray(results, dtype=np.uint32).reshape(-1, 3)
    keep = results[:, 0] != NONE
    out = np.empty((int(keep.sum()), 4), dtype=np.uint32)
    out[:, 0] = owner[keep]
    out[:, 1:] = results[keep]
    return out


def least(hits, n_pairs):
    """(n_pairs, 3): of every pair the hit of least distance, the first of equal ones; NONE three times for a pair of none"""
    out = np.full((n_pairs, 3), NONE, dtype=np.uint32)
    for pair, d, r, j in np.asarray(hits).tolist():
        if out[pair, 0] == NONE or d < out[pair, 0]:
            out[pair] = (d, r, j)
    return out


def per_pair_counts(hits, n_pairs):
    return np.bincount(np.asarray(hits, dtype=np.int64).reshape(-1, 4)[:, 0], minlength=n_pairs)
