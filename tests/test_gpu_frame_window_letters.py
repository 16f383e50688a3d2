"""GPU parity of txq_frame_window_letters (include/txq.h; `tetrex search --translate --frame-window --verify-frame-windows`,
DESIGN.md §20): begins, lengths, stops and thresholds of every window against tests/verify_frame_windows_ref.py, exactly.
Records of every length 0 .. 90 nt (R < k, R <= W, a tail window, window begins at every alignment modulo 16), stop-dense
records, lower case, U and N; k = 3 and 6 with (W, S) = (8, 3), (8, 1), (8, 8) and (40, 10); E = 0 .. 3, so windows with s = E,
s = E + 1 and t <= 0 all occur; the frames buffer at an odd alignment and ending exactly at the last frame; one record of
2 x 10^5 nt with S = 1, whose 4 x 10^5 windows are more than one pass of the kernel's capped grid (1024 blocks of 256 lanes); the _device call on a
stream of torch's making behind the two translation calls with no host wait in between; the host twin's refusals."""
import numpy as np
import pytest

import verify_frame_windows_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(8, 3), (8, 1), (8, 8), (40, 10)]


@pytest.fixture(scope="module")
def capi():
    from tetrex_amd import capi as c
    c.init(0)
    return c


def _records():
    rng = np.random.default_rng(77)
    nt = lambda L: "".join(rng.choice(list("ACGT"), size=L))
    records = [nt(L) for L in range(0, 91)]
    records += [("TAA" * 40)[:L] for L in (0, 24, 25, 26, 89, 90)]
    records += [("TAATGA" * 20)[o:o + 84] for o in range(3)]
    records += ["".join(rng.choice(["TAA", "TGA", "TAG", "GCT", "AAA", "CTG"], size=30, p=[0.1, 0.1, 0.1, 0.3, 0.2, 0.2])) + "AC"[:o] for o in range(3) for _ in range(4)]
    records += [nt(90).lower(), nt(90).replace("T", "U"), nt(87).lower().replace("t", "u")]
    records += ["".join(rng.choice(list("ACGTN"), size=90, p=[0.24, 0.24, 0.24, 0.24, 0.04])) for _ in range(3)]
    return records


RECORDS = _records()
_want = {}


def want(k, W, S, E):
    """the restatement's arrays, computed once per case and left unchanged"""
    if (k, W, S, E) not in _want:
        arrays = R.window_letters(RECORDS, k, W, S, E)
        for a in arrays[1:]:
            a.setflags(write=False)
        _want[(k, W, S, E)] = arrays
    return _want[(k, W, S, E)]


def _codes():
    from tetrex_amd import host
    return host.peptide_codes(0)


@pytest.mark.parametrize("W,S", SHAPES)
@pytest.mark.parametrize("k", [3, 6])
def test_host_twin_equals_restatement(capi, k, W, S):
    values, offsets, win_offsets, _, win_lens = capi.translate_windows(RECORDS, k, _codes(), W, S)
    frames, frame_offsets = capi.translate_frames(RECORDS)
    rec = np.concatenate([[0], np.cumsum([len(r) for r in RECORDS])]).astype(np.uint64)
    seen = set()
    for E in range(4):
        w_frames, w_foff, w_woff, w_beg, w_len, w_stops, w_ws, w_thr = want(k, W, S, E)
        assert frames.tobytes().decode() == w_frames and np.array_equal(frame_offsets, w_foff) and np.array_equal(win_offsets, w_woff)
        assert np.array_equal(win_lens, w_ws)
        beg, lens, stops, thr = capi.frame_window_letters(rec + np.uint64(5), k, W, S, frames, frame_offsets, win_offsets, win_lens, E)
        assert np.array_equal(beg, w_beg) and np.array_equal(lens, w_len)
        assert np.array_equal(stops, w_stops), np.flatnonzero(stops != w_stops)[:5]
        assert np.array_equal(thr, w_thr), np.flatnonzero(thr != w_thr)[:5]
        # the cases the rule has: s = E, s = E + 1, searched with a stop, t <= 0 with s <= E
        for name, there in (("s=E", (w_stops == E) & (E > 0)), ("s=E+1", w_stops == E + 1), ("searched with a stop", (w_stops > 0) & (w_thr != R.NOT_SEARCHED)),
                            ("t<=0", (w_stops <= E) & (w_thr == R.NOT_SEARCHED))):
            if np.any(there):
                seen.add(name)
    assert seen == {"s=E", "s=E+1", "searched with a stop", "t<=0"}, seen
    if (W, S) == (8, 1):  # window begins at every alignment modulo 16
        assert len({int(b) % 16 for b in want(k, W, S, 0)[3]}) == 16


@pytest.mark.parametrize("frames_at", [0, 1, 7, 15])
def test_device_call_on_a_stream_at_an_odd_alignment(capi, frames_at):
    """translate_windows, translate_frames and the new call queued on one stream of torch's making with no host wait between
    them; the frames buffer begins frames_at bytes behind a 16-byte boundary and its allocation ends 0 to 15 bytes behind the
    last frame, so a 16-byte load that is not clipped to frames_bytes leaves what the call was given"""
    import torch
    k, W, S, E = 6, 40, 10, 2
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    w_frames, w_foff, w_woff, w_beg, w_len, w_stops, w_ws, w_thr = want(k, W, S, E)
    frames, foff, woff, wlens, beg, lens, stops, thr = capi.frame_window_letters_device(RECORDS, k, _codes(), W, S, E, frames_at=frames_at,
                                                                                        stream=stream.cuda_stream)
    assert frames.tobytes().decode() == w_frames and np.array_equal(foff, w_foff) and np.array_equal(woff, w_woff) and np.array_equal(wlens, w_ws)
    assert np.array_equal(beg, w_beg) and np.array_equal(lens, w_len) and np.array_equal(stops, w_stops) and np.array_equal(thr, w_thr)


def test_a_buffer_cut_short_is_not_read_behind_its_end(capi):
    """frames_bytes below the bound: the windows that leave it are not searched and keep 0 stops, the others are unchanged"""
    k, W, S, E = 3, 8, 3, 1
    w_frames, w_foff, w_woff, w_beg, w_len, w_stops, w_ws, w_thr = want(k, W, S, E)
    cut = len(w_frames) - len(w_frames) // 3 - 5
    frames, foff, woff, wlens, beg, lens, stops, thr = capi.frame_window_letters_device(RECORDS, k, _codes(), W, S, E, frames_at=3, capacity=cut)
    inside = w_beg + w_len.astype(np.uint64) <= np.uint64(cut)
    assert 0 < int(inside.sum()) < inside.size
    assert np.array_equal(beg, w_beg) and np.array_equal(lens, w_len)
    assert np.array_equal(stops, np.where(inside, w_stops, 0)) and np.array_equal(thr, np.where(inside, w_thr, R.NOT_SEARCHED))


def test_more_windows_than_one_pass_of_the_grid(capi):
    """one record of 2 x 10^5 nt, S = 1: about 4 x 10^5 windows — more than the 1024 x 256 lanes of a pass of the capped grid, so
    lanes take a second window — against prefix sums over the restatement's frames"""
    from translate_ref import translate_frame
    k, W, S, E = 6, 40, 1, 2
    rng = np.random.default_rng(9)
    seq = "".join(rng.choice(list("ACGT"), size=200000))
    values, offsets, win_offsets, _, win_lens = capi.translate_windows([seq], k, _codes(), W, S)
    frames, frame_offsets = capi.translate_frames([seq])
    assert win_lens.size > 1024 * 256
    beg, lens, stops, thr = capi.frame_window_letters(np.array([0, len(seq)], dtype=np.uint64), k, W, S, frames, frame_offsets, win_offsets, win_lens, E)
    at = 0
    for f in range(6):
        residues = np.frombuffer(translate_frame(seq, f).encode(), dtype=np.uint8)
        assert np.array_equal(frames[int(frame_offsets[f]):int(frame_offsets[f + 1])], residues)
        n = residues.size - W + 1  # S = 1: a window at every residue, no tail window
        assert int(win_offsets[f + 1] - win_offsets[f]) == n
        pref = np.concatenate([[0], np.cumsum(residues == ord("*"))])
        w_stops = (pref[W:] - pref[:-W]).astype(np.uint32)
        sl = slice(at, at + n)
        assert np.array_equal(beg[sl], np.arange(n, dtype=np.uint64) + frame_offsets[f]) and np.all(lens[sl] == W)
        assert np.array_equal(stops[sl], w_stops)
        t = win_lens[sl].astype(np.int64) - k * (E - w_stops.astype(np.int64))
        assert np.array_equal(thr[sl], np.where((w_stops > E) | (t <= 0), R.NOT_SEARCHED, t).astype(np.uint32))
        at += n
    assert at == win_lens.size and np.any(thr != R.NOT_SEARCHED) and np.any(stops > E)


def test_host_twin_refuses_bad_arguments(capi):
    k, W, S = 3, 8, 3
    _, _, win_offsets, _, win_lens = capi.translate_windows(RECORDS[:20], k, _codes(), W, S)
    frames, frame_offsets = capi.translate_frames(RECORDS[:20])
    rec = np.concatenate([[0], np.cumsum([len(r) for r in RECORDS[:20]])]).astype(np.uint64)
    good = dict(rec_offsets=rec, k=k, window=W, step=S, frames=frames, frame_offsets=frame_offsets, win_offsets=win_offsets, win_lens=win_lens, edits=1)
    capi.frame_window_letters(**good)
    for change in (dict(k=0), dict(k=13), dict(window=2), dict(step=0), dict(step=9), dict(rec_offsets=rec[::-1].copy()),
                   dict(win_offsets=win_offsets[::-1].copy()), dict(frame_offsets=frame_offsets + np.uint64(1)), dict(n_windows=int(win_lens.size) - 1)):
        with pytest.raises(capi.TxqError) as e:
            capi.frame_window_letters(**dict(good, **change))
        assert e.value.code == -1, change
    L = capi.lib()
    assert L.txq_frame_window_letters_device(None, 1, k, W, S, None, 0, None, None, None, 0, 1, None, None, None, None, None) == -1
    assert L.txq_frame_window_letters(None, 0, k, W, S, None, 0, None, None, None, 0, 1, None, None, None, None) == -1
