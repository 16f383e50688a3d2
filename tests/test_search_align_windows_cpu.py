"""`tetrex search --align-windows` as far as it goes with no index and no device: what the parser refuses, and
that the two full commands pass it and stop at the index file."""
import os
import subprocess

import pytest

from conftest import ROOT

TETREX = os.path.join(ROOT, "bin", "tetrex")


def _run(*args):
    r = subprocess.run([TETREX, "search", *args, "no_such_index.ibf", "no_such_queries.fa"], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("args", [
    ("--align-windows",),
    ("-e", "2", "--verify", "--align-windows"),
    ("--window", "60", "-e", "2", "--align-windows"),
    ("--translate", "--frame-window", "40", "-e", "2", "--align-windows"),
], ids=["alone", "with_verify", "window_unverified", "frame_window_unverified"])
def test_align_windows_needs_verified_windows(args):
    rc, so, se = _run(*args)
    lines = [line for line in se.splitlines() if line.startswith("[Search Parser Error]")]
    assert rc == 1 and so == "" and len(lines) == 1 and "Index not valid" not in se and "Unknown option" not in se, se
    assert "--align-windows" in lines[0] and "--verify-windows" in lines[0] and "--verify-frame-windows" in lines[0], se


@pytest.mark.parametrize("args", [
    ("--window", "60", "--step", "15", "-e", "2", "--verify-windows", "--align-windows"),
    ("--window", "60", "-e", "2", "--verify-windows", "--align-windows", "--counts"),
    ("--translate", "--frame-window", "40", "--frame-step", "10", "-e", "2", "--verify-frame-windows", "--align-windows"),
    ("--translate", "--frame-window", "40", "-e", "2", "--verify-frame-windows", "--align-windows", "--counts"),
], ids=["windows", "windows_counts", "frame_windows", "frame_windows_counts"])
def test_the_full_commands_get_as_far_as_the_index(args):
    rc, so, se = _run(*args)
    assert rc == 1 and so == "" and "Index not valid" in se and "[Search Parser Error]" not in se, se


@pytest.mark.parametrize("args", [
    ("--window", "60", "-e", "2", "--verify-windows", "--align"),
    ("--translate", "--frame-window", "40", "-e", "2", "--verify-frame-windows", "--align"),
], ids=["windows", "frame_windows"])
def test_align_next_to_verified_windows_names_the_flag_that_is_meant(args):
    rc, so, se = _run(*args)
    assert rc == 1 and so == "" and se.startswith("[Search Parser Error] ") and "--align:" in se and "--align-windows" in se and "Index not valid" not in se, se
