"""Python restatement of `tetrex search --window W [--step S] -e E --verify-windows` (csrc/host/search_cmd.cpp search_windowed,
DESIGN.md §19): the window layout and thresholds are tests/search_window_ref.py's, the distances tests/edit_ref.py's, and the
merge of confirmed windows into rows is restated here.  Nothing is shared with the code under test.

A hit (window, bin) — the window's count of k-mers in the bin reaches its threshold — is a candidate; it is CONFIRMED when the
window's letters are within E edits of a substring of one record of the bin (case-insensitive; on a nucleotide index on
either strand, the lower distance winning and + on a tie).  Every maximal run of consecutive confirmed windows of a (record,
bin, strand) is a row."""
import numpy as np

import edit_ref as E
from search_window_ref import windows_of, threshold_of


def revcomp(s):
    """the reverse complement as the command makes it: U is T, every other byte becomes N (which matches nothing)"""
    table = {"A": "T", "C": "G", "G": "C", "T": "A", "U": "A"}
    return "".join(table.get(c.upper(), "N") for c in reversed(s))


def merge_confirmed(windows, k, confirmed, with_counts=False):
    """The rows of one (record, bin).  windows: windows_of's list; confirmed: {window index: (count, distance, target,
    target_end, strand)} of the confirmed windows (strand "+" or "-"; "" where the index has one strand).  Every maximal run of
    consecutive windows of one strand is a row (begin, end[, "count/w"], distance, target, target_end[, strand]): begin and end
    the 1-based inclusive letters of the run's union, count/w of the run's best window by count (the earliest on a tie),
    distance, target and target_end of its window of least distance (the earliest on a tie).  Rows ascend by begin, + before -."""
    rows = []
    for strand in sorted({c[4] for c in confirmed.values()}, key=lambda s: s == "-"):
        js = sorted(j for j in confirmed if confirmed[j][4] == strand)
        i = 0
        while i < len(js):
            e = i + 1
            while e < len(js) and js[e] == js[e - 1] + 1:
                e += 1
            run = js[i:e]
            best = max(run, key=lambda j: (confirmed[j][0], -j))
            near = min(run, key=lambda j: (confirmed[j][1], j))
            row = (windows[run[0]][0] + 1, windows[run[-1]][0] + windows[run[-1]][1])
            if with_counts:
                row += ("%d/%d" % (confirmed[best][0], windows[best][1] - k + 1),)
            row += tuple(confirmed[near][1:4])
            if strand:
                row += (strand,)
            rows.append((run[0], strand == "-", row))
            i = e
    rows.sort(key=lambda r: (r[0], r[1]))
    return [r[2] for r in rows]


def window_distances(records, k, W, S, errors, bins, codes, dna):
    """Every searched window of every query against every bin, by the dynamic program.  records: [(name, letters)]; bins: a list
    of [(target name, letters)] per bin.  Returns {(record, window, bin): (distance, target, target_end, strand)} for the
    windows within `errors` of the bin (strand "" unless dna), and the number of searched windows."""
    patterns, owner = [], []
    for r, (_, letters) in enumerate(records):
        for j, (b, n) in enumerate(windows_of(len(letters), k, W, S)):
            if threshold_of(n - k + 1, k, errors) == 0:
                continue
            for strand in ("+", "-") if dna else ("",):
                patterns.append(revcomp(letters[b:b + n]) if strand == "-" else letters[b:b + n])
                owner.append((r, j, strand))
    targets = [t for recs in bins for t in recs]
    groups = np.concatenate([[0], np.cumsum([len(recs) for recs in bins])])
    pairs = [(p, u, errors) for p in range(len(patterns)) for u in range(len(bins))]
    res = E.search(patterns, [t[1] for t in targets], groups, pairs, codes).reshape(len(patterns), len(bins), 3)
    out = {}
    for p, (r, j, strand) in enumerate(owner):
        for u in range(len(bins)):
            d, t, end = (int(x) for x in res[p, u])
            if d == E.NONE:
                continue
            have = out.get((r, j, u))
            if have is None or d < have[0]:  # (+ comes first: it wins a tie)
                out[(r, j, u)] = (d, targets[t][0], end, strand)
    return out, len({(r, j) for r, j, _ in owner})


def rows_of(records, k, W, S, n_bins, distances, hit_counts=None, with_counts=False):
    """All rows of a query file.  distances: window_distances' dict; hit_counts: {(record, window, bin): count} of the filter's
    hits (the candidates), or None: every searched window within E edits of a bin is a hit there — the filter's guarantee
    (q-gram lemma; a Bloom filter drops nothing) —, so the rows without counts follow from the distances alone.  Returns
    ([(name, bin, begin, end[, count/w], distance, target, target_end[, strand])], the number of confirmed candidates) in the
    order of the command: by record, bin in index order, begin."""
    rows, n_confirmed = [], 0
    for r, (name, letters) in enumerate(records):
        wins = windows_of(len(letters), k, W, S)
        for u in range(n_bins):
            confirmed = {j: (hit_counts[(r, j, u)] if hit_counts else 0,) + distances[(r, j, u)] for j in range(len(wins))
                         if (hit_counts is None or (r, j, u) in hit_counts) and (r, j, u) in distances}
            n_confirmed += len(confirmed)
            for row in merge_confirmed(wins, k, confirmed, with_counts):
                rows.append((name, u) + row)
    return rows, n_confirmed
