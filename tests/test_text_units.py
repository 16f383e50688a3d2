"""What the text kernels share (csrc/txq_text.hpp) without a GPU: tests/native/text_units_dump.cpp, built with the address and
undefined-behaviour sanitizers, answers one command per line.  The expected values are worked out here from what the functions
promise: the pair that owns a unit, the record that holds a byte, the checks of a group in their order, the unit arithmetic,
and the clipped 16-byte load on host memory.

The sanitizer sees every byte read behind a text and every byte read in front of one that begins at a multiple of 8 bytes.
In front of a text that begins elsewhere, the up to 7 bytes that share its 8-byte granule cannot be poisoned: they hold 0xEE,
which is neither a text byte nor a fill, so a block that took one of them in is caught by its value."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("text_units") / "text_units_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "native", "text_units_dump.cpp")], check=True, timeout=600)

    def run(lines):
        r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


def _words(*xs):
    return " ".join(str(int(x)) for x in xs)


# units per pair: refused pairs and regex pairs of empty groups have 0 (at the front, in the middle, at the end), a regex
# group of records without bytes has 1
UNITS = [[0, 0, 3, 0, 1, 0, 0, 2, 0], [0, 5], [5, 0], [1], [0, 0, 1, 0, 0], [1, 0, 1, 2, 0, 1], [0, 1, 1, 1, 0], [7]]


def test_pair_of_unit(dump):
    lines, want = [], []
    for units in UNITS:
        pref = [0]
        for n in units:
            pref.append(pref[-1] + n)
        for u in range(pref[-1]):
            lines.append("pair " + _words(len(units), *pref, u))
            want.append(next(i for i in range(len(units)) if pref[i] <= u < pref[i + 1]))
    assert len(lines) == sum(sum(u) for u in UNITS)
    assert [int(x) for x in dump(lines)] == want


# record offsets with empty records at the start, in runs and at the end; (r0, r1) ranges with r0 > 0 among them
RECORDS = [([0, 0, 0, 5, 5, 5, 9, 12, 12, 12], [(0, 9), (2, 9), (3, 7), (1, 6), (5, 6), (0, 4)]),
           ([3, 8], [(0, 1)]),
           ([0, 5, 5, 5], [(0, 3), (0, 1)]),
           ([2, 2, 2, 3], [(0, 3), (1, 3), (2, 3)])]


def test_record_of(dump):
    lines, want = [], []
    for rec, ranges in RECORDS:
        for r0, r1 in ranges:
            for x in range(rec[r0], rec[r1]):
                lines.append("record " + _words(len(rec) - 1, *rec, r0, r1, x))
                want.append(max(r for r in range(r0, r1) if rec[r] <= x))
    assert len(lines) > 60
    assert [int(x) for x in dump(lines)] == want


def _group(g, grp, rec, text_bytes):
    return "group " + _words(g, len(grp) - 1, *grp, len(rec) - 1, *rec, text_bytes)


def test_view_group(dump):
    grp, rec = [0, 2, 2, 5], [0, 4, 4, 10, 10, 17]
    accepted = [(_group(0, grp, rec, 17), (1, 0, 2, 0, 4)),
                (_group(2, grp, rec, 17), (1, 2, 5, 4, 17)),           # ge == text_bytes
                (_group(2, grp, rec, 1000), (1, 2, 5, 4, 17)),
                (_group(1, grp, rec, 17), (1, 2, 2, 4, 4)),            # r0 == r1: a group of no records
                (_group(0, [1, 2], rec, 17), (1, 1, 2, 4, 4)),         # gs == ge: a record of no bytes
                (_group(0, [5, 5], rec, 17), (1, 5, 5, 17, 17)),       # r0 == r1 == n_rec
                (_group(0, [0, 0], [0], 0), (1, 0, 0, 0, 0))]          # no records at all
    refused = [_group(3, grp, rec, 17),                                # g >= n_grp
               _group(0xFFFFFFFF, grp, rec, 17),
               _group(0, [3, 1], rec, 17),                             # r0 > r1
               _group(0, [0, 6], rec, 17),                             # r1 > n_rec: rec[6] does not exist
               _group(0, [7, 9], rec, 17),
               _group(0, [0, 1], [9, 4, 12], 12),                      # gs > ge
               _group(2, grp, rec, 16),                                # ge > text_bytes
               _group(0, [0, 1], [0, 1 << 63], (1 << 63) - 1)]
    out = dump([line for line, _ in accepted] + refused)
    for (line, want), got in zip(accepted, out):
        assert tuple(int(x) for x in got.split()) == want, line
    for line, got in zip(refused, out[len(accepted):]):
        assert got.split()[0] == "0", line


def test_units_of_and_chunk_bounds(dump):
    lines, want = [], []
    for lanes, chunk in ((64, 16), (64, 512), (256, 256), (4, 16)):
        for bytes_, units in ((0, 0), (1, 1), (lanes * chunk, 1), (lanes * chunk + 1, 2)):
            lines.append("units " + _words(bytes_, lanes, chunk))
            want.append(str(units))
            gs, ge = 100, 100 + bytes_
            for slice_, lane in ((0, 0), (0, 1), (0, lanes - 1), (1, 0), (1, lanes - 1)):
                ca = gs + (slice_ * lanes + lane) * chunk
                lines.append("chunk " + _words(gs, ge, slice_, lanes, lane, chunk))
                want.append(_words(ca, min(ca + chunk, ge)))
    assert dump(lines) == want
    # the chunks of a text's units that have bytes (ca < ge) tile it in order, the last one cut at ge
    gs, ge, lanes, chunk = 7, 7 + 4 * 16 + 1, 4, 16
    out = dump(["chunk " + _words(gs, ge, s, lanes, l, chunk) for s in range(2) for l in range(lanes)])
    cuts = [tuple(int(x) for x in o.split()) for o in out]
    owned = [c for c in cuts if c[0] < ge]
    assert owned[0][0] == gs and owned[-1][1] == ge and all(a[1] == b[0] for a, b in zip(owned, owned[1:])) and len(owned) == 5
    assert all(ca >= ge and cb == ge for ca, cb in cuts[5:])


@pytest.mark.parametrize("fill", [0, ord("N")])
def test_clipped_load(dump, fill):
    cases = [(residue, n) for residue in range(16) for n in (1, 15, 16, 17, 33)]
    out = dump(["load " + _words(residue, n, fill) for residue, n in cases])
    whole_blocks = 0
    for (residue, n), line in zip(cases, out):
        text = [128 + (37 * j + 11) % 100 for j in range(n)]
        blocks = line.split(";")
        assert len(blocks) == (residue + n + 15) // 16, (residue, n)  # every block that meets the text, from the one that holds lo
        for k, block in enumerate(blocks):
            t0, whole, hexa = block.split()
            t0, got = int(t0), list(bytes.fromhex(hexa))
            assert t0 == (16 * k - residue) % (1 << 64), (residue, n, k)
            want = [text[16 * k + i - residue] if residue <= 16 * k + i < residue + n else fill for i in range(16)]
            assert got == want, (residue, n, k)
            assert int(whole) == (16 * k >= residue and 16 * k + 16 <= residue + n), (residue, n, k)
            whole_blocks += int(whole)
            for i in range(16):
                t = (t0 + i) % (1 << 64)
                if 16 * k + i >= residue:
                    assert t == 16 * k + i - residue  # the true index, also behind the text
                else:
                    assert t >= n                     # below lo: beyond any bound a caller keeps its indices under
    assert whole_blocks >= 16
