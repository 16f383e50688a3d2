"""Python restatement of the host side of `tetrex search --window W [--step S]` (csrc/host/search_cmd.cpp search_windowed, whose window layout and run merge are csrc/host/search_plan.hpp's; DESIGN.md
§17): how a record is cut into windows, what a window's threshold is, and how the hit windows of a (record, bin) become rows.
Positions are letters; a window of l letters has w = l - k + 1 values, value i being the k-mer that starts at letter i."""
import math


def windows_of(L, k, W, S):
    """The (begin, len) list of a record of L letters: begin the 0-based letter offset, len in letters.  L < k: none (the
    record is skipped).  L <= W: the whole record.  Otherwise offsets 0, S, 2 S, ... while offset + W <= L, and one more at
    L - W where the last of these ends before L."""
    assert k >= 1 and W >= k and 1 <= S <= W
    if L < k:
        return []
    if L <= W:
        return [(0, L)]
    out = [(at, W) for at in range(0, L - W + 1, S)]
    if out[-1][0] + W < L:
        out.append((L - W, W))
    return out


def threshold_of(w, k, errors=None, fraction=None):
    """t of a window of w values: -e E gives max(w - k E, 0), --threshold F gives ceil(F w).  0: the window is not searched."""
    if fraction is not None:
        return int(math.ceil(fraction * w))
    return max(w - k * errors, 0)


def merge_rows(windows, k, hit_counts, with_counts=False):
    """The rows of one (record, bin).  windows: windows_of's list; hit_counts: {window index: count} of the windows in which the
    bin is hit.  Every maximal run of consecutive hit windows is one row (begin, end[, "count/w"]): the 1-based inclusive
    letter positions of the run's union and, with counts, count/w of the run's best window — the highest count, the earliest
    window on a tie.  Rows ascend by begin."""
    rows = []
    js = sorted(hit_counts)
    i = 0
    while i < len(js):
        e = i + 1
        while e < len(js) and js[e] == js[e - 1] + 1:
            e += 1
        run = js[i:e]
        best = max(run, key=lambda j: (hit_counts[j], -j))
        begin = windows[run[0]][0] + 1
        end = windows[run[-1]][0] + windows[run[-1]][1]
        row = (begin, end)
        if with_counts:
            row += ("%d/%d" % (hit_counts[best], windows[best][1] - k + 1),)
        rows.append(row)
        i = e
    return rows


def search_rows(records, k, W, S, count_fn, n_bins, errors=None, fraction=None, with_counts=False):
    """All rows of a query file.  records: [(name, letters)]; count_fn(record index, begin, len) -> the counts per bin of the
    window's values (a sequence of n_bins numbers).  Returns ([(name, bin, begin, end[, "count/w"])], notes) in the order of
    the command: by record, bin in index order, begin; notes: the names of the records skipped (L < k) and of those with a
    window that was not searched."""
    rows, skipped, unsearched = [], [], []
    for r, (name, letters) in enumerate(records):
        wins = windows_of(len(letters), k, W, S)
        if not wins:
            skipped.append(name)
            continue
        per_bin = [dict() for _ in range(n_bins)]
        any_unsearched = False
        for j, (b, n) in enumerate(wins):
            t = threshold_of(n - k + 1, k, errors, fraction)
            if t == 0:
                any_unsearched = True
                continue
            counts = count_fn(r, b, n)
            for u in range(n_bins):
                if counts[u] >= t:
                    per_bin[u][j] = int(counts[u])
        if any_unsearched:
            unsearched.append(name)
        for u in range(n_bins):
            for row in merge_rows(wins, k, per_bin[u], with_counts):
                rows.append((name, u) + row)
    return rows, (skipped, unsearched)
