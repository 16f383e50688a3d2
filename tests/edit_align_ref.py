"""The yardstick of alignments (include/txq.h txq_edit_align_device, include/txh.h txh_edit_align, `tetrex search --verify
--align`): the full O(mn) matrix of Sellers' recurrence and the walk back by the three rules, in plain Python and numpy.
Nothing here is shared with the code under test, and nothing is banded.

    D[i][0] = i, D[0][j] = 0, D[i][j] = min(D[i-1][j-1] + c, D[i-1][j] + 1, D[i][j-1] + 1), c = 0 where P[i-1] and R[j-1] match

Two bytes match when their classes (codes[256]) are equal and neither is 255.  From (m, j): the diagonal where j' > 0 and
D[i-1][j'-1] + c = D[i][j'] ('=' for c = 0, 'X' for c = 1), else up where D[i-1][j'] + 1 = D[i][j'] ('I'), else left ('D')."""
import numpy as np

NONE = 0xFFFFFFFF
NOT_ALIGNED = 0xFFFFFFFE


def as_bytes(x):
    if isinstance(x, str):
        x = x.encode()
    return np.frombuffer(bytes(x), dtype=np.uint8) if not isinstance(x, np.ndarray) else x.astype(np.uint8, copy=False)


def matrix(pattern, record, codes):
    """D as an (m + 1, n + 1) array, and nomatch[i - 1][j - 1] = c"""
    codes = np.asarray(codes, dtype=np.uint8)
    pc, tc = codes[as_bytes(pattern)], codes[as_bytes(record)]
    m, n = pc.size, tc.size
    nomatch = ((pc[:, None] != tc[None, :]) | (pc[:, None] == 255)).astype(np.int64).reshape(m, n)
    idx = np.arange(n + 1, dtype=np.int64)
    D = np.zeros((m + 1, n + 1), dtype=np.int64)
    for i in range(1, m + 1):
        cand = np.empty(n + 1, dtype=np.int64)
        cand[0] = i
        cand[1:] = np.minimum(D[i - 1, :-1] + nomatch[i - 1], D[i - 1, 1:] + 1)
        D[i] = idx + np.minimum.accumulate(cand - idx)  # D[i][j] = min(cand[j], D[i][j-1] + 1)
    return D, nomatch


def walk(D, nomatch, j):
    """(start, operations from the pattern's first letter to its last) of the path that ends in (m, j)"""
    i, ops = D.shape[0] - 1, []
    while i > 0:
        if j > 0 and D[i - 1, j - 1] + nomatch[i - 1, j - 1] == D[i, j]:
            ops.append("X" if nomatch[i - 1, j - 1] else "=")
            i, j = i - 1, j - 1
        elif D[i - 1, j] + 1 == D[i, j]:
            ops.append("I")
            i -= 1
        else:
            assert j > 0 and D[i, j - 1] + 1 == D[i, j]
            ops.append("D")
            j -= 1
    return j, "".join(reversed(ops))


def runs_of(ops):
    """'==X=' -> [('=', 2), ('X', 1), ('=', 1)]"""
    out = []
    for c in ops:
        if out and out[-1][0] == c:
            out[-1] = (c, out[-1][1] + 1)
        else:
            out.append((c, 1))
    return out


def cigar(runs):
    return "".join("%d%s" % (n, c) for c, n in runs)


def align(pattern, record, codes, j=None):
    """(d, j, start, runs) of the pattern against one record; j None: the lowest end that reaches the least distance"""
    D, nomatch = matrix(pattern, record, codes)
    if j is None:
        j = int(D[-1].argmin())
    start, ops = walk(D, nomatch, j)
    return int(D[-1, j]), j, start, runs_of(ops)


def align_pairs(patterns, records, pairs, results, codes):
    """What edit_align answers for search results (n, 3): (start[n], runs[n]); a pair whose result is NONE has start NONE and no
    runs.  The triples must be genuine: D[m][j] = d is asserted."""
    starts, runs = [], []
    for (p, _, _), (d, r, j) in zip(np.asarray(pairs).reshape(-1, 3).tolist(), np.asarray(results).reshape(-1, 3).tolist()):
        if d == NONE:
            starts.append(NONE)
            runs.append([])
            continue
        dd, _, start, rr = align(patterns[p], records[r], codes, j)
        assert dd == d, (p, d, r, j, dd)
        starts.append(start)
        runs.append(rr)
    return np.array(starts, dtype=np.uint32), runs


def check_identities(m, d, j, start, runs):
    """the sums of include/txq.h, and at most 2 d + 1 runs of which no two neighbours share an operation"""
    total = {c: sum(n for cc, n in runs if cc == c) for c in "=XID"}
    assert all(n >= 1 for _, n in runs) and all(a[0] != b[0] for a, b in zip(runs, runs[1:])), runs
    assert total["="] + total["X"] + total["D"] == j - start, (runs, j, start)
    assert total["="] + total["X"] + total["I"] == m, (runs, m)
    assert total["X"] + total["I"] + total["D"] == d, (runs, d)
    assert len(runs) <= 2 * d + 1, (runs, d)
