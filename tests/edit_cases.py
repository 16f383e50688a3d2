"""Inputs shared by tests/test_edit_cpu.py and tests/test_gpu_edit.py: for every pattern length one pattern, records of
length 0, 1, m - 1, m and a long one that holds edited copies of the pattern, in four groups (the fourth with empty
records between records that have bytes), and the caps
0, 1, 3, m - 1, m, m + 5 for every (pattern, group).  Alphabets of 4 and 20 letters; about one byte in 25 has no class."""
import numpy as np

import edit_ref as E

ALPHABETS = {"dna": "ACGT", "peptide": "ACDEFGHIKLMNPQRSTVWY"}


def random_text(rng, letters, n, junk=0.04):
    """n bytes: letters in either case, and bytes of class 255 ('#', '-', digits) with probability `junk`"""
    pool = np.frombuffer((letters + letters.lower()).encode(), dtype=np.uint8)
    out = pool[rng.integers(0, pool.size, size=n)].copy()
    bad = np.frombuffer(b"#-0189 ", dtype=np.uint8)
    at = rng.random(n) < junk
    out[at] = bad[rng.integers(0, bad.size, size=int(at.sum()))]
    return out


def edited(rng, letters, seq, edits):
    """`edits` substitutions, insertions and deletions at random places"""
    s = list(seq)
    pool = (letters + letters.lower()).encode()
    for _ in range(edits):
        kind = int(rng.integers(0, 3))
        at = int(rng.integers(0, max(len(s), 1)))
        if kind == 0 and s:
            s[at] = pool[int(rng.integers(0, len(pool)))]
        elif kind == 1:
            s.insert(at, pool[int(rng.integers(0, len(pool)))])
        elif s:
            del s[at]
    return np.array(s, dtype=np.uint8)


def caps_of(m):
    return [0, 1, 3, m - 1, m, m + 5]


def build(lengths, alphabet, seed, long_bytes=1200):
    """(patterns, records, groups, pairs, codes) over all `lengths`"""
    letters = ALPHABETS[alphabet]
    rng = np.random.default_rng(seed)
    codes = E.letter_codes(letters)
    patterns, records, groups, pairs = [], [], [0], []
    for m in lengths:
        p = random_text(rng, letters, m, junk=0.02)
        long = [random_text(rng, letters, int(rng.integers(0, long_bytes // 3)))]
        for edits in (4, 2, 0, 1, 3):  # the exact copy is neither the first nor the last
            long += [edited(rng, letters, p, edits), random_text(rng, letters, int(rng.integers(0, long_bytes // 6)))]
        # groups (consecutive records): the short records; the one of m bytes; the long one with an empty one behind it
        g = len(groups) - 1
        records += [np.zeros(0, np.uint8), random_text(rng, letters, 1), random_text(rng, letters, m - 1)]
        groups.append(len(records))
        records += [np.concatenate([edited(rng, letters, p, 1), random_text(rng, letters, 1)])[:m]]
        groups.append(len(records))
        records += [np.concatenate(long), np.zeros(0, np.uint8)]
        groups.append(len(records))
        # a fourth: empty records BETWEEN two that have bytes (one, then two), the exact copy behind them; the record in the
        # middle holds an exact copy as well, so that the first and the last tie where the first holds one by chance or by m = 1
        records += [np.concatenate([random_text(rng, letters, 20), edited(rng, letters, p, 2), random_text(rng, letters, 9)]), np.zeros(0, np.uint8),
                    np.concatenate([random_text(rng, letters, 5), p, random_text(rng, letters, 30)]), np.zeros(0, np.uint8), np.zeros(0, np.uint8),
                    np.concatenate([random_text(rng, letters, 40), p, random_text(rng, letters, 3)])]
        groups.append(len(records))
        pat = len(patterns)
        patterns.append(p)
        for e in caps_of(m):
            pairs += [(pat, g, e), (pat, g + 1, e), (pat, g + 2, e), (pat, g + 3, e)]
    groups.append(len(records))  # a last group of no records
    pairs += [(0, len(groups) - 2, 1000)]
    return patterns, records, groups, pairs, codes
