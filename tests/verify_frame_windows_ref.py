"""Python restatement of `tetrex search --translate --frame-window W [--frame-step S] -e E --verify-frame-windows`
(csrc/host/search_cmd.cpp search_translated_windowed, include/txq.h txq_frame_window_letters), on top of
tests/frame_window_ref.py (frames, windows, w), tests/edit_ref.py (distances; `*` has no class, so it matches nothing) and
tests/verify_windows_ref.py (merge_confirmed).  Nothing is shared with the code under test.

A window of l residues with s stops and w stop-free k-mers is searched with t = w - k (E - s) where s <= E and that is above 0.
A hit (window, bin) is a candidate; it is CONFIRMED when the window's residue letters are within E edits of a substring of one
record of the bin.  Every maximal run of consecutive confirmed windows of a (record, frame, bin) is a row."""
import numpy as np

import edit_ref as E
import frame_window_ref as F
from translate_ref import FRAMES, translate_frame
from verify_windows_ref import merge_confirmed

NOT_SEARCHED = 0xFFFFFFFF
PEPTIDE_CODES = E.letter_codes("ABCDEFGHIJKLMNOPQRSTUVWXYZ")  # BinVerifier's peptide table: every letter a class, * none


def stop_threshold(w, s, k, errors):
    """t of a window of w stop-free k-mers and s stops; NOT_SEARCHED: the window is not searched"""
    if s > errors:
        return NOT_SEARCHED
    t = w - k * (errors - s)
    return t if t > 0 else NOT_SEARCHED


def plain_threshold(w, k, errors):
    """§18's t = max(w - k E, 0), in the same form"""
    t = w - k * errors
    return t if t > 0 else NOT_SEARCHED


def window_letters(records, k, W, S, errors):
    """What txq_translate_frames and txq_frame_window_letters give for a list of nucleotide records: (frames as one string,
    frame_offsets[6 n + 1], win_offsets[6 n + 1], begins, lens, stops, ws, thresholds), begins indexing the frames string."""
    frames, frame_offsets, win_offsets = [], [0], [0]
    begins, lens, stops, ws, thresholds = [], [], [], [], []
    for seq in records:
        for f in range(6):
            residues = translate_frame(seq, f)
            ranges = F.window_ranges(seq, f, k, W, S)
            for (a, n), (_, w) in zip(F.windows_of(len(residues), k, W, S), ranges):
                s = residues[a:a + n].count("*")
                begins.append(frame_offsets[-1] + a)
                lens.append(n)
                stops.append(s)
                ws.append(w)
                thresholds.append(stop_threshold(w, s, k, errors))
            frames.append(residues)
            frame_offsets.append(frame_offsets[-1] + len(residues))
            win_offsets.append(len(begins))
    return ("".join(frames), np.array(frame_offsets, dtype=np.uint64), np.array(win_offsets, dtype=np.uint64), np.array(begins, dtype=np.uint64),
            np.array(lens, dtype=np.uint32), np.array(stops, dtype=np.uint32), np.array(ws, dtype=np.uint32), np.array(thresholds, dtype=np.uint32))


def window_distances(records, k, W, S, errors, bins, codes=PEPTIDE_CODES, plain=False):
    """Every searched window of every frame of every query against every bin, by the dynamic program.  records: [(name,
    nucleotides)]; bins: a list of [(target name, letters)] per bin.  Returns {(record, frame, window, bin): (distance, target,
    target_end)} for the windows within `errors` of the bin, and the number of searched windows.  plain: §18's threshold
    decides what is searched (windows with more than E stops too: none of them can be within E)."""
    patterns, owner = [], []
    for r, (_, seq) in enumerate(records):
        for f in range(6):
            residues = translate_frame(seq, f)
            for j, ((a, n), (_, w)) in enumerate(zip(F.windows_of(len(residues), k, W, S), F.window_ranges(seq, f, k, W, S))):
                s = residues[a:a + n].count("*")
                t = plain_threshold(w, k, errors) if plain else stop_threshold(w, s, k, errors)
                if t == NOT_SEARCHED:
                    continue
                patterns.append(residues[a:a + n])
                owner.append((r, f, j))
    targets = [t for recs in bins for t in recs]
    groups = np.concatenate([[0], np.cumsum([len(recs) for recs in bins])])
    pairs = [(p, u, errors) for p in range(len(patterns)) for u in range(len(bins))]
    res = E.search(patterns, [t[1] for t in targets], groups, pairs, codes).reshape(len(patterns), len(bins), 3)
    out = {}
    for p, (r, f, j) in enumerate(owner):
        for u in range(len(bins)):
            d, t, end = (int(x) for x in res[p, u])
            if d != E.NONE:
                out[(r, f, j, u)] = (d, targets[t][0], end)
    return out, len(owner)


def rows_of(records, k, W, S, n_bins, distances, hit_counts=None, with_counts=False):
    """All rows of a query file.  distances: window_distances' dict; hit_counts: {(record, frame, window, bin): count} of the
    filter's hits (the candidates), or None: every searched window within E edits of a bin is a hit there — the guarantee of
    the threshold —, so the rows without counts follow from the distances alone.  Returns ([(name, bin, frame
    name, begin, end[, count/w], distance, target, target_end)], the number of confirmed candidates) in the order of the
    command: by record, frame, bin in index order, begin (nucleotides, 1-based inclusive, on the record as given)."""
    rows, n_confirmed = [], 0
    for r, (name, seq) in enumerate(records):
        L = len(seq)
        for f in range(6):
            wins = F.frame_windows(L, f, k, W, S)
            ws = [w for _, w in F.window_ranges(seq, f, k, W, S)] if with_counts else None
            for u in range(n_bins):
                confirmed = {j: (hit_counts[(r, f, j, u)] if hit_counts else 0,) + distances[(r, f, j, u)] + ("",) for j in range(len(wins))
                             if (hit_counts is None or (r, f, j, u) in hit_counts) and (r, f, j, u) in distances}
                n_confirmed += len(confirmed)
                if not confirmed:
                    continue
                merged = merge_confirmed(wins, k, confirmed)
                # count/w: merge_confirmed takes w from a window's letters, here it is the window's stop-free k-mers
                counted = merge_confirmed([(a, w + k - 1) for (a, _), w in zip(wins, ws)], k, confirmed, True) if with_counts else merged
                for row, crow in zip(merged, counted):
                    at = F.residues_on_record(L, f, row[0] - 1, row[1])
                    rows.append((name, u, FRAMES[f]) + at + ((crow[2],) if with_counts else ()) + tuple(row[2:]))
    return rows, n_confirmed
