"""Python restatement of `tetrex search --translate --frame-window W [--frame-step S]` (csrc/host/search_cmd.cpp
search_translated_windowed, include/txq.h txq_translate_windows), on top of tests/translate_ref.py (frames,
genetic code, values) and tests/search_window_ref.py (how R letters are cut into windows, thresholds).

A frame of R residues is cut like a record of R letters under --window: W and S count residues.  Window [a, a + l) owns the
frame's k-mer positions [a, a + l - k + 1); with V(c) = the number of stop-free k-mers of the frame at positions below c (brute
force over the frame's letters here) these are the frame's values [V(a), V(a + l - k + 1)), w = the difference of them.  The
window's threshold is threshold_of(w); a window with t = 0 is not searched.  Rows: per (record, frame, bin) every maximal run
of consecutive hit windows, as 1-based inclusive nucleotide positions on the record as given."""
import numpy as np

from search_window_ref import windows_of, threshold_of
from translate_ref import FRAMES, translate_frame, reverse_complement, normalise


def frame_len(L, o):
    return (L - o) // 3 if L >= o else 0


def frame_windows(L, f, k, W, S):
    """the (begin, len) list, in residues, of frame f of a record of L bytes"""
    return windows_of(frame_len(L, f % 3), k, W, S)


def stop_free(residues, k):
    """valid[c]: the k-mer at residue position c of the frame holds no stop"""
    return [("*" not in residues[c:c + k]) for c in range(len(residues) - k + 1)]


def window_ranges(seq, f, k, W, S):
    """[(V(a), w)] of the windows of frame f of a record: the first value, relative to the frame's first, and the value count"""
    residues = translate_frame(seq, f)
    valid = stop_free(residues, k)
    V = [0]
    for ok in valid:
        V.append(V[-1] + int(ok))
    return [(V[a], V[a + n - k + 1] - V[a]) for a, n in windows_of(len(residues), k, W, S)]


def translate_windows(records, k, W, S):
    """(offsets[6 n + 1], win_offsets[6 n + 1], begins, lens) as txq_translate_windows gives them: begins absolute in the values
    of all frames back to back"""
    offsets, win_offsets, begins, lens = [0], [0], [], []
    for seq in records:
        for f in range(6):
            residues = translate_frame(seq, f)
            for b, w in window_ranges(seq, f, k, W, S):
                begins.append(offsets[-1] + b)
                lens.append(w)
            win_offsets.append(len(begins))
            offsets.append(offsets[-1] + sum(stop_free(residues, k)))
    return (np.array(offsets, dtype=np.uint64), np.array(win_offsets, dtype=np.uint64), np.array(begins, dtype=np.uint64),
            np.array(lens, dtype=np.uint32))


def window_count(lengths, k, W, S):
    return sum(2 * len(windows_of(frame_len(L, o), k, W, S)) for L in lengths for o in range(3))


def residues_on_record(L, f, ra, rb):
    """the residues [ra, rb) of frame f of a record of L bytes as (begin, end), 1-based inclusive nucleotides of the record"""
    o = f % 3
    if f < 3:
        return o + 3 * ra + 1, o + 3 * rb
    return L - o - 3 * rb + 1, L - o - 3 * ra


def cut_and_translate(seq, f, begin, end):
    """the letters begin .. end of the record, reverse-complemented on a reverse frame, translated in frame +1"""
    piece = normalise(seq)[begin - 1:end]
    return translate_frame(piece if f < 3 else reverse_complement(piece), 0)


def merge_rows(L, f, windows, ws, hit_counts, with_counts=False):
    """The rows of one (record, frame, bin).  windows: frame_windows' list; ws: the windows' value counts; hit_counts:
    {window index: count} of the windows in which the bin is hit.  Every maximal run of consecutive hit windows is one row
    (begin, end[, "count/w"]): the nucleotides of the run's residues and, with counts, count/w of the run's best window — the
    highest count, the earliest window on a tie.  Rows ascend by the run's first window."""
    rows = []
    js = sorted(hit_counts)
    i = 0
    while i < len(js):
        e = i + 1
        while e < len(js) and js[e] == js[e - 1] + 1:
            e += 1
        run = js[i:e]
        best = max(run, key=lambda j: (hit_counts[j], -j))
        row = residues_on_record(L, f, windows[run[0]][0], windows[run[-1]][0] + windows[run[-1]][1])
        if with_counts:
            row += ("%d/%d" % (hit_counts[best], ws[best]),)
        rows.append(row)
        i = e
    return rows


def search_rows(records, k, W, S, count_fn, n_bins, errors=None, fraction=None, with_counts=False):
    """All rows of a query file.  records: [(name, nucleotides)]; count_fn(record index, frame, window index) -> the counts per
    bin of the window's values.  Returns (rows, (no_kmer, unsearched), windows searched): rows (name, bin, frame name, begin,
    end[, "count/w"]) in the order of the command — record, frame, bin in index order, begin; no_kmer: the records with no k-mer
    in any window; unsearched: the other records none of whose windows has a threshold above 0."""
    rows, no_kmer, unsearched, n_searched = [], [], [], 0
    for r, (name, seq) in enumerate(records):
        L = len(seq)
        any_kmer = searched = False
        mine = []
        for f in range(6):
            wins = frame_windows(L, f, k, W, S)
            ws = [w for _, w in window_ranges(seq, f, k, W, S)]
            per_bin = [dict() for _ in range(n_bins)]
            for j, w in enumerate(ws):
                any_kmer = any_kmer or w > 0
                t = threshold_of(w, k, errors, fraction) if w else 0
                if t == 0:
                    continue
                searched = True
                n_searched += 1
                counts = count_fn(r, f, j)
                for u in range(n_bins):
                    if counts[u] >= t:
                        per_bin[u][j] = int(counts[u])
            for u in range(n_bins):
                for row in merge_rows(L, f, wins, ws, per_bin[u], with_counts):
                    mine.append((name, u, FRAMES[f]) + row)
        if not any_kmer:
            no_kmer.append(name)
        elif not searched:
            unsearched.append(name)
        rows.extend(mine)
    return rows, (no_kmer, unsearched), n_searched
