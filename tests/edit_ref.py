"""The yardstick of approximate matching by edit distance (include/txq.h txq_edit_search, include/txh.h txh_edit_search,
`tetrex search --verify`): Sellers' dynamic program, restated in numpy.  Nothing here is shared with the code under test.

    D[i][0] = i, D[0][j] = 0, D[i][j] = min(D[i-1][j-1] + [no match], D[i-1][j] + 1, D[i][j-1] + 1)

Two bytes match when their classes (codes[256]) are equal and neither is 255.  A row is computed from the one before it
without a Python loop over j: with cand[j] = min(D[i-1][j-1] + [no match], D[i-1][j] + 1) (cand[0] = i) the insertion term
D[i][j] = min(cand[j], D[i][j-1] + 1) unrolls to D[i][j] = j + min over k <= j of (cand[k] - k), a running minimum."""
import numpy as np

NONE = 0xFFFFFFFF


def letter_codes(letters, extra=None):
    """a class table: letter i of `letters` is class i in either case, every other byte 255; extra: {byte: class}"""
    codes = np.full(256, 255, dtype=np.uint8)
    for i, c in enumerate(letters):
        codes[ord(c.upper())] = i
        codes[ord(c.lower())] = i
    for k, v in (extra or {}).items():
        codes[ord(k.upper())] = v
        codes[ord(k.lower())] = v
    return codes


def as_bytes(x):
    if isinstance(x, str):
        x = x.encode()
    return np.frombuffer(bytes(x), dtype=np.uint8) if not isinstance(x, np.ndarray) else x.astype(np.uint8, copy=False)


def last_rows(patterns, text, codes):
    """D[m][0..n] of B patterns of one length m (a (B, m) uint8 array) against one record: a (B, n + 1) integer array"""
    pc = np.asarray(codes, dtype=np.uint8)[np.atleast_2d(patterns)]
    tc = np.asarray(codes, dtype=np.uint8)[as_bytes(text)]
    B, m = pc.shape
    n = tc.size
    dt = np.int16 if n + m < 30000 else np.int32  # (every value and every cand[k] - k lies in [-n, n + m])
    idx = np.arange(n + 1, dtype=dt)
    prev = np.zeros((B, n + 1), dtype=dt)
    for i in range(1, m + 1):
        c = pc[:, i - 1:i]
        nomatch = ((c != tc[None, :]) | (c == 255)).astype(dt)
        cand = np.empty((B, n + 1), dtype=dt)
        cand[:, 0] = i
        cand[:, 1:] = np.minimum(prev[:, :-1] + nomatch, prev[:, 1:] + 1)
        prev = idx + np.minimum.accumulate(cand - idx, axis=1)
    return prev


def group_results(patterns, records, r0, r1, caps, codes):
    """(distance, record, end) of B patterns of one length against records r0 .. r1 - 1 (record indexes are those of
    `records`), caps[B]: a (B, 3) uint32 array, NONE three times where the least distance is above the cap"""
    patterns = np.atleast_2d(patterns)
    B = patterns.shape[0]
    best = np.full(B, np.iinfo(np.int64).max, dtype=np.int64)
    rec = np.full(B, NONE, dtype=np.int64)
    end = np.full(B, NONE, dtype=np.int64)
    for r in range(r0, r1):
        row = last_rows(patterns, records[r], codes)
        d = row.min(axis=1)
        j = row.argmin(axis=1)  # (the first of equal values)
        better = d < best
        best[better], rec[better], end[better] = d[better], r, j[better]
    out = np.full((B, 3), NONE, dtype=np.uint32)
    ok = best <= np.asarray(caps, dtype=np.int64)
    out[ok, 0], out[ok, 1], out[ok, 2] = best[ok], rec[ok], end[ok]
    return out


def search(patterns, records, groups, pairs, codes):
    """The whole contract: patterns and records are lists of bytes/str, groups offsets into the records, pairs rows of
    (pattern, group, cap).  Pairs of one group and pattern length are computed together.  Returns (n, 3) uint32."""
    pats = [as_bytes(p) for p in patterns]
    recs = [as_bytes(r) for r in records]
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 3)
    out = np.full((pairs.shape[0], 3), NONE, dtype=np.uint32)
    batches = {}
    for i, (p, g, e) in enumerate(pairs):
        batches.setdefault((int(g), pats[p].size), []).append(i)
    for (g, m), rows in batches.items():
        assert m >= 1
        for at in range(0, len(rows), 256):
            part = rows[at:at + 256]
            block = np.stack([pats[pairs[i, 0]] for i in part])
            out[part] = group_results(block, recs, int(groups[g]), int(groups[g + 1]), pairs[part, 2], codes)
    return out


def distance(pattern, text, codes):
    """d(P, R) and the lowest end position that reaches it"""
    row = last_rows(as_bytes(pattern)[None, :], text, codes)[0]
    return int(row.min()), int(row.argmin())
