"""numpy restatement of the similarity rearrangement of `tetrex index --layout sized --rearrange`
(tetrex_amd/csrc/host/layout.hpp rearrange_intervals / rearrange_chain, include/txq.h txq_pair_unions_device): the intervals
of the sorted order, the nearest-neighbour chain inside one interval, the pairwise union estimates, and the final order."""
import numpy as np

from sized_hibf_ref import estimate

MAX_LEN = 4096


def sorted_order(counts):
    """User bins by estimate descending, ties by id."""
    counts = np.asarray(counts, dtype=np.float64)
    return sorted(range(counts.size), key=lambda b: (-counts[b], b))


def intervals(counts, order, ratio, max_len=MAX_LEN):
    """First sorted position of every interval: an interval starts at s and takes the following positions e while
    counts[order[e]] >= ratio * counts[order[s]] and while it is shorter than max_len."""
    counts = np.asarray(counts, dtype=np.float64)
    starts, s, B = [], 0, len(order)
    while s < B:
        starts.append(s)
        floor = np.float64(ratio) * counts[order[s]]
        e = s + 1
        while e < B and e - s < max_len and counts[order[e]] >= floor:
            e += 1
        s = e
    return starts


def chain(c, u):
    """Positions of one interval in their new order: position 0 stays, then always the bin not yet placed with the largest
    J = (c_last + c_j - u[last][j]) / u[last][j] to the bin placed last (u == 0: J = 0; ties: the smaller position)."""
    c = np.asarray(c, dtype=np.float64)
    n = c.size
    u = np.asarray(u, dtype=np.float64).reshape(n, n)
    if n < 3:
        return list(range(n))
    out, left = [0], list(range(1, n))
    while left:
        last = out[-1]
        best, best_j = None, None
        for j in left:  # ascending: a tie keeps the smaller position
            uj = u[last, j]
            jac = np.float64(0.0) if uj == 0 else (c[last] + c[j] - uj) / uj
            if best is None or jac > best_j:
                best, best_j = j, jac
        out.append(best)
        left.remove(best)
    return out


def pair_unions(regs, ids):
    """[i, j] = estimate of the union of bins ids[i] and ids[j] (the diagonal: each bin's own estimate)."""
    ids = [int(i) for i in ids]
    n = len(ids)
    out = np.zeros((n, n), dtype=np.float64)
    for i in range(n):
        mx = np.maximum(regs[ids[i]][None, :], regs[ids[i:]])
        for d in range(n - i):
            out[i, i + d] = out[i + d, i] = estimate(mx[d])
    return out


def rearranged_order(counts, regs, ratio, max_len=MAX_LEN, pairs=pair_unions):
    """The order the build lays out: the sorted order with every interval of three or more bins chained.
    Returns (order, interval starts)."""
    order = sorted_order(counts)
    starts = intervals(counts, order, ratio, max_len)
    final = list(order)
    for i, s in enumerate(starts):
        e = starts[i + 1] if i + 1 < len(starts) else len(order)
        if e - s < 3:
            continue
        ids = order[s:e]
        ch = chain([counts[b] for b in ids], pairs(regs, ids))
        final[s:e] = [ids[p] for p in ch]
    return final, starts
