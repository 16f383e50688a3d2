"""What `tetrex search --translate --verify-frames` decides without a GPU: the option checks, which are made
before the index is read, the refusal of a nucleotide index, and txq_translate_frames_bound against Python."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TETREX = os.path.join(ROOT, "bin", "tetrex")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _run(*args):
    r = subprocess.run([TETREX, *args], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("flags,words", [(["--verify-frames", "-e", "2"], ["--verify-frames", "--translate"]),
                                         (["--translate", "--verify-frames"], ["--verify-frames", "-e"]),
                                         (["--translate", "--verify-frames", "--threshold", "0.5"], ["--verify-frames", "--threshold"]),
                                         (["--translate", "-e", "2", "--verify-frames", "--verify"], ["--verify-frames", "--verify"]),
                                         (["--verify", "--translate", "-e", "2", "--verify-frames"], ["--verify-frames", "--verify"])], ids=str)
def test_cli_refuses_verify_frames_without_its_conditions(tmp_path, flags, words):
    """--verify-frames needs --translate and -e and excludes --threshold and --verify: one parser error that names
    --verify-frames, before the index is read (the index named here does not exist), with a non-zero exit"""
    q = tmp_path / "q.fa"
    q.write_text(">a\nACGTACGTACGTACGTACGTAGGCTAGCTAGGATCGATCGA\n")
    rc, so, se = _run("search", *flags, str(tmp_path / "missing.ibf"), str(q))
    lines = [l for l in se.splitlines() if l.startswith("[Search Parser Error]")]
    assert len(lines) == 1 and "Unknown option" not in se and "Index not valid" not in se and so == "", se
    for w in words:
        assert w in lines[0], se
    assert rc != 0


def test_verify_frames_on_a_nucleotide_index_is_refused(tmp_path):
    q = tmp_path / "q.fa"
    q.write_text(">a\nACGTACGTACGTACGTACGTAGGCTAGCTAGGATCGATCGA\n")
    rc, so, se = _run("search", "--translate", "--verify-frames", "-e", "1", os.path.join(GOLDEN, "ibf_idx.ibf"), str(q))
    assert rc == 1 and so == ""
    assert "peptide index" in se and "nucleotide index" in se
    assert "txq" not in se and "HIP" not in se  # refused before the device is asked for


def test_frames_bound_equals_python():
    from tetrex_amd import capi
    lengths = list(range(0, 51))
    rec = np.concatenate([[7], 7 + np.cumsum(lengths)]).astype(np.uint64)  # (the first record need not begin at byte 0)
    want = [sum(2 * ((L - o) // 3) for o in range(3) if L >= o) for L in lengths]
    assert capi.translate_frames_bound(rec) == sum(want)
    for i, L in enumerate(lengths):
        assert capi.translate_frames_bound(rec[i:i + 2]) == want[i], L
    assert capi.translate_frames_bound(np.zeros(1, dtype=np.uint64)) == 0
    with pytest.raises(capi.TxqError):
        capi.translate_frames_bound(np.array([0, 9, 4], dtype=np.uint64))
    # null pointers are refused before any device is asked for
    L = capi.lib()
    assert L.txq_translate_frames_bound(None, 1) == 0xFFFFFFFFFFFFFFFF
    assert L.txq_translate_frames_device(None, None, 1, None, 0, None, None) == -1
    assert L.txq_translate_frames(None, None, 1, None, 0, None) == -1
