"""Python restatement of `tetrex search ... --verify-windows --window-targets` (csrc/host/search_cmd.cpp): the
window layout and thresholds are tests/search_window_ref.py's, the distances tests/edit_ref.py's (every record of a bin a group
of its own, as tests/edit_targets_ref.py makes them), and the merge of target hits into rows is restated here on top of
tests/verify_windows_ref.py's merge of one list of windows.  Nothing is shared with the code under test.

A TARGET HIT is (window, bin, record r of the bin) with d(window, r) <= E; on a nucleotide index the better strand of the two,
+ on equal distance.  For every (record, bin, target) — and strand — every maximal run of consecutive windows that hit the
target is a row; the rows of a (record, bin) come by target in the order of the bin's file, then by begin, + before -."""
import numpy as np

import edit_ref as E
from search_window_ref import windows_of, threshold_of
from verify_windows_ref import merge_confirmed, revcomp


def merge_targets(windows, k, hits, with_counts=False):
    """The rows of one (record, bin).  hits: {(window index, target index): (count, distance, target, target_end, strand)} —
    the target index is the record's place in the bin's file.  Rows as merge_confirmed writes them, for every target in turn."""
    rows = []
    for t in sorted({key[1] for key in hits}):
        rows += merge_confirmed(windows, k, {j: v for (j, u), v in hits.items() if u == t}, with_counts)
    return rows


def target_distances(records, k, W, S, errors, bins, codes, dna):
    """Every searched window of every query against every record of every bin, by the dynamic program.  records: [(name,
    letters)]; bins: a list of [(target name, letters)] per bin.  Returns {(record, window, bin, target index): (distance, target
    name, target_end, strand)} for the targets within `errors` (strand "" unless dna: else the better one, + on a tie), and the
    number of searched windows."""
    patterns, owner = [], []
    for r, (_, letters) in enumerate(records):
        for j, (b, n) in enumerate(windows_of(len(letters), k, W, S)):
            if threshold_of(n - k + 1, k, errors) == 0:
                continue
            for strand in ("+", "-") if dna else ("",):
                patterns.append(revcomp(letters[b:b + n]) if strand == "-" else letters[b:b + n])
                owner.append((r, j, strand))
    targets = [(u, t, name, letters) for u, recs in enumerate(bins) for t, (name, letters) in enumerate(recs)]
    pairs = [(p, g, errors) for p in range(len(patterns)) for g in range(len(targets))]
    res = E.search(patterns, [x[3] for x in targets], list(range(len(targets) + 1)), pairs, codes).reshape(len(patterns), len(targets), 3)
    out = {}
    for p, (r, j, strand) in enumerate(owner):
        for g, (u, t, name, _) in enumerate(targets):
            d, _, end = (int(x) for x in res[p, g])
            if d == E.NONE:
                continue
            have = out.get((r, j, u, t))
            if have is None or d < have[0]:  # (+ comes first: it wins a tie)
                out[(r, j, u, t)] = (d, name, end, strand)
    return out, len({(r, j) for r, j, _ in owner})


def rows_of(records, k, W, S, n_bins, distances, hit_counts=None, with_counts=False):
    """All rows of a query file.  distances: target_distances' dict; hit_counts as in verify_windows_ref.rows_of (None: every
    window within E edits of a record of a bin is a hit of the filter there).  Returns ([(name, bin, begin, end[, count/w],
    distance, target, target_end[, strand])], the number of confirmed candidates (window, bin), the number of target hits) in
    the order of the command: by record, bin in index order, target in the order of the bin's file, begin."""
    rows, confirmed, n_targets = [], set(), 0
    by_pair = {}
    for (r, j, u, t), v in distances.items():
        if hit_counts is None or (r, j, u) in hit_counts:
            by_pair.setdefault((r, u), {})[(j, t)] = ((hit_counts[(r, j, u)] if hit_counts else 0,) + v)
            confirmed.add((r, j, u))
            n_targets += 1
    for r, (name, letters) in enumerate(records):
        wins = windows_of(len(letters), k, W, S)
        for u in range(n_bins):
            for row in merge_targets(wins, k, by_pair.get((r, u), {}), with_counts):
                rows.append((name, u) + row)
    return rows, len(confirmed), n_targets


def nearest_of(distances):
    """{(record, window, bin): (distance, target, target_end, strand)}: of every window's target hits in a bin the least by
    (distance, then target order) — what --verify-windows attributes to the window (invariant (b) of DESIGN.md §22; on a
    nucleotide index up to the strand-tie case of §16)"""
    out = {}
    for (r, j, u, t), v in sorted(distances.items(), key=lambda x: (x[0][:3], x[1][0], x[0][3])):
        out.setdefault((r, j, u), v)
    return out


def union_of(rows):
    """{(name, bin): sorted list of disjoint (begin, end) intervals that the rows' begin..end cover} (invariant (a))"""
    spans = {}
    for r in rows:
        spans.setdefault((r[0], r[1]), []).append((int(r[2]), int(r[3])))
    out = {}
    for key, iv in spans.items():
        merged = []
        for b, e in sorted(iv):
            if merged and b <= merged[-1][1] + 1:
                merged[-1][1] = max(merged[-1][1], e)
            else:
                merged.append([b, e])
        out[key] = [tuple(x) for x in merged]
    return out


# ---- `--translate --frame-window --verify-frame-windows --window-targets`: the same on the windows of the six frames ----------

def frame_target_distances(records, k, W, S, errors, bins):
    """tests/verify_frame_windows_ref.py window_distances per TARGET: every searched window of every frame of every nucleotide
    query against every record of every bin.  Returns {(record, frame, window, bin, target index): (distance, target name,
    target_end)} and the number of searched windows (§20's stop rule decides what is searched)."""
    import frame_window_ref as F
    import verify_frame_windows_ref as RF
    from translate_ref import translate_frame
    patterns, owner = [], []
    for r, (_, seq) in enumerate(records):
        for f in range(6):
            residues = translate_frame(seq, f)
            for j, ((a, n), (_, w)) in enumerate(zip(F.windows_of(len(residues), k, W, S), F.window_ranges(seq, f, k, W, S))):
                if RF.stop_threshold(w, residues[a:a + n].count("*"), k, errors) == RF.NOT_SEARCHED:
                    continue
                patterns.append(residues[a:a + n])
                owner.append((r, f, j))
    targets = [(u, t, name, letters) for u, recs in enumerate(bins) for t, (name, letters) in enumerate(recs)]
    pairs = [(p, g, errors) for p in range(len(patterns)) for g in range(len(targets))]
    res = E.search(patterns, [x[3] for x in targets], list(range(len(targets) + 1)), pairs, RF.PEPTIDE_CODES).reshape(len(patterns), len(targets), 3)
    out = {}
    for p, (r, f, j) in enumerate(owner):
        for g, (u, t, name, _) in enumerate(targets):
            d, _, end = (int(x) for x in res[p, g])
            if d != E.NONE:
                out[(r, f, j, u, t)] = (d, name, end)
    return out, len(owner)


def frame_rows_of(records, k, W, S, n_bins, distances):
    """All rows of a nucleotide query file: ([(name, bin, frame name, begin, end, distance, target, target_end)], confirmed
    candidates, target hits), by record, frame, bin in index order, target in the order of the bin's file, begin"""
    import frame_window_ref as F
    from translate_ref import FRAMES
    by = {}
    for (r, f, j, u, t), v in distances.items():
        by.setdefault((r, f, u), {})[(j, t)] = (0,) + v + ("",)
    rows = []
    for r, (name, seq) in enumerate(records):
        for f in range(6):
            wins = F.frame_windows(len(seq), f, k, W, S)
            for u in range(n_bins):
                for row in merge_targets(wins, k, by.get((r, f, u), {})):
                    rows.append((name, u, FRAMES[f]) + F.residues_on_record(len(seq), f, row[0] - 1, row[1]) + tuple(row[2:]))
    return rows, len({key[:4] for key in distances}), len(distances)


def frame_nearest_of(distances):
    """nearest_of for frame windows: {(record, frame, window, bin): (distance, target, target_end)}"""
    out = {}
    for key, v in sorted(distances.items(), key=lambda x: (x[0][:4], x[1][0], x[0][4])):
        out.setdefault(key[:4], v)
    return out
