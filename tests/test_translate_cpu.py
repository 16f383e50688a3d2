"""Six-frame translation on the CPU: the restatement of tests/translate_ref.py against pinned literals, the
host's txh_translated_values against the restatement bit for bit, txq_translate_bound against its formula, and what
`tetrex search --translate` refuses before it touches a GPU."""
import os
import subprocess

import numpy as np
import pytest

import translate_ref as T
from conftest import GOLDEN, ROOT

TETREX = os.path.join(ROOT, "bin", "tetrex")

PINNED = "ATGGCCATTGTAATGGGCCGCTGAAAGGGTGCCCGATAG"
PINNED_FRAMES = {"+1": "MAIVMGR*KGAR*", "+2": "WPL*WAAERVPD", "+3": "GHCNGPLKGCPI",
                 "-1": "LSGTLSAAHYNGH", "-2": "YRAPFQRPITMA", "-3": "IGHPFSGPLQWP"}


def _run(*args):
    r = subprocess.run([TETREX, *args], capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


def test_pinned_translations():
    from tetrex_amd import host
    assert T.TABLE1 == "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
    for f, name in enumerate(T.FRAMES):
        assert T.translate_frame(PINNED, f) == PINNED_FRAMES[name], name
        assert host.translate_frame(PINNED, f) == PINNED_FRAMES[name], name
        # lower case and U read the same; an ambiguous byte makes its codon X in both strands
        assert T.translate_frame(PINNED.lower().replace("t", "u"), f) == PINNED_FRAMES[name]
        assert host.translate_frame(PINNED.lower().replace("t", "u"), f) == PINNED_FRAMES[name]
    assert T.translate_frame("ATGNCCATT", 0) == "MXI" and T.translate_frame("ATGNCCATT", 3) == "NXH"
    assert host.FRAMES == T.FRAMES


def check_record(seq, k, reduction):
    from tetrex_amd import host
    want_v, want_o = T.translated_values(seq, k, reduction)
    got_v, got_o = host.translated_values(seq, k, reduction)
    assert np.array_equal(got_o, want_o), (seq, k, reduction)
    assert np.array_equal(got_v, want_v), (seq, k, reduction)
    L = len(seq)
    assert int(want_o[-1]) <= T.bound([L], k)
    for f in range(6):  # a frame without a stop has every window
        if "*" not in T.translate_frame(seq, f):
            assert int(want_o[f + 1] - want_o[f]) == max(0, (L - f % 3) // 3 - k + 1)


@pytest.mark.parametrize("k", [1, 3, 5, 6, 12])
@pytest.mark.parametrize("reduction", [0, 1, 2])
def test_host_values_equal_restatement_short_and_special(k, reduction):
    rng = np.random.default_rng(100 * k + reduction)
    for L in range(0, 3 * k + 7):
        check_record("".join(rng.choice(list("ACGT"), size=L)), k, reduction)
    body = "".join(rng.choice(list("ACGT"), size=40 * k))
    check_record(body.lower(), k, reduction)
    check_record(body.replace("T", "U"), k, reduction)
    check_record(body[:10 * k] + "N" * (3 * k + 2) + body[10 * k:] + "NN" + body[:7] + "n" * 50, k, reduction)
    check_record("TAA" * (2 * k + 3), k, reduction)   # all stops in +1, none elsewhere
    check_record("TAATAGTGA" * (k + 1) + "T", k, reduction)
    check_record("N" * (6 * k + 1), k, reduction)
    check_record("ACGT-acgu RYKM*" * (k + 2), k, reduction)  # bytes that are no nucleotide letters


@pytest.mark.parametrize("k,reduction", [(3, 0), (6, 0), (5, 1), (12, 2)])
def test_host_values_equal_restatement_random_records(k, reduction):
    rng = np.random.default_rng(k)
    for _ in range(200):
        L = int(rng.integers(20, 2001))
        s = rng.choice(list("ACGT"), size=L)
        s[rng.random(L) < 0.01] = "N"
        check_record("".join(s), k, reduction)


def test_bound_equals_formula():
    from tetrex_amd import capi
    rng = np.random.default_rng(1)
    for k in (1, 3, 6, 12):
        lengths = [0, 1, 2, 3 * k - 1, 3 * k, 3 * k + 1, 3 * k + 2, 3 * k + 3] + [int(x) for x in rng.integers(0, 3000, size=50)]
        offsets = np.concatenate([[7], 7 + np.cumsum(lengths)]).astype(np.uint64)  # (the first record need not start at 0)
        assert capi.translate_bound(offsets, k) == T.bound(lengths, k)
        records = ["".join(rng.choice(list("ACGT"), size=L)) for L in lengths]
        assert int(T.translate_records(records, k)[1][-1]) <= T.bound(lengths, k)
    assert capi.translate_bound(np.array([0], dtype=np.uint64), 6) == 0
    with pytest.raises(capi.TxqError):
        capi.translate_bound(np.array([0, 5, 3], dtype=np.uint64), 6)  # offsets not ascending


def test_k_outside_1_to_12_is_refused():
    from tetrex_amd import capi, host
    import ctypes as C
    for k in (0, 13, 32):
        with pytest.raises(host.HostError):
            host.translated_values("ACGT" * 30, k)
        with pytest.raises(capi.TxqError) as e:
            capi.translate_bound(np.array([0, 100], dtype=np.uint64), k)
        assert e.value.code == -1
        # the argument checks come before anything that needs a GPU
        seq = np.frombuffer(b"ACGT" * 30, dtype=np.uint8)
        rec = np.array([0, 120], dtype=np.uint64)
        out = np.zeros(512, dtype=np.uint64)
        off = np.zeros(7, dtype=np.uint64)
        L = capi.lib()
        assert L.txq_translate(seq.ctypes.data, rec.ctypes.data_as(capi.u64p), 1, k, host.peptide_codes().ctypes.data,
                               out.ctypes.data_as(capi.u64p), off.ctypes.data_as(capi.u64p)) == -1
        assert L.txq_translate_device(C.c_void_p(8), C.c_void_p(8), 1, k, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), None) == -1
    L = capi.lib()
    assert L.txq_translate_device(None, None, 1, 6, None, None, None, None) == -1
    assert L.txq_translate(None, None, 1, 6, None, None, None) == -1
    assert L.txq_hit_list_device(None, None, 1, 1, None, 0, None, None) == -1
    with pytest.raises(host.HostError):
        host.translated_values("ACGT" * 30, 6, reduction=3)


def test_code_tables_are_the_encoders():
    """the 256-byte table handed to the device folds exactly as record_values does"""
    from tetrex_amd import host
    for reduction in (0, 1, 2):
        codes = host.peptide_codes(reduction)
        for letter in "ACDEFGHIKLMNPQRSTVWYX":
            assert host.record_values(letter, 1, dna=False, reduction=reduction) == [int(codes[ord(letter)])]
        assert int(codes.max()) < 32


def test_translate_on_a_nucleotide_index_is_refused(tmp_path):
    q = tmp_path / "q.fa"
    q.write_text(">a\nACGTACGTACGTACGTACGTAGGCTAGCTAGGATCGATCGA\n")
    rc, so, se = _run("search", "--translate", os.path.join(GOLDEN, "ibf_idx.ibf"), str(q))
    assert rc == 1 and so == ""
    assert "peptide index" in se and "nucleotide index" in se
    assert "txq" not in se and "HIP" not in se  # refused before the device is asked for


@pytest.mark.parametrize("flags", [["--translate", "-e", "1", "--threshold", "0.5"], ["--translate", "--threshold", "0"],
                                   ["--translate", "-e", "-1"], ["--translate", "--bogus"], ["--translate=1", "--bogus"]], ids=str)
def test_translate_parses_alongside_the_option_refusals(tmp_path, flags):
    q = tmp_path / "q.fa"
    q.write_text(">a\nACGTACGTACGTACGTACGT\n")
    rc, so, se = _run("search", *flags, str(tmp_path / "missing.ibf"), str(q))
    assert "[Search Parser Error]" in se and "Index not valid" not in se and so == "", se
    assert rc != 0


def test_translate_flag_is_known(tmp_path):
    """with valid options the flag gets as far as the index file (which is missing here): it is not an unknown option"""
    q = tmp_path / "q.fa"
    q.write_text(">a\nACGTACGTACGTACGTACGT\n")
    rc, so, se = _run("search", "--translate", "-e", "1", "--counts", str(tmp_path / "missing.ibf"), str(q))
    assert rc == 1 and "[Search Parser Error]" not in se and "Index not valid" in se
