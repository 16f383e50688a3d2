"""`tetrex query --gpu-verify` on the GPU box: the flag changes where the time goes, not one byte of the
result — stdout and every output file are compared with a run without it — and its -S line shows that the device did the
work: a silent fallback to the host would pass the parity and fail the counters."""
import glob
import json
import os
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from family_fasta import family_library
from motifs import PEPTIDE_QUERIES

pytestmark = pytest.mark.gpu
TETREX = os.path.join(ROOT, "bin", "tetrex")
BATCH = PEPTIDE_QUERIES + ["A.{15}C"]
# on a reduced index the front-end compiles no {m,n}: the motifs it does compile, and the too-large one spelled out
MURPHY_BATCH = [rx for rx in PEPTIDE_QUERIES if "{" not in rx] + ["A" + "." * 15 + "C"]


def run(*args, cwd=None):
    r = subprocess.run([TETREX, *args], capture_output=True, cwd=cwd, timeout=300)
    return r.returncode, r.stdout, r.stderr.decode(errors="replace")


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    d = tmp_path_factory.mktemp("toy")
    files = sorted(glob.glob(os.path.join(GOLDEN, "dna_example_split", "*.fa")))
    rc, _, se = run("index", "-n", "-k", "3", "-i", str(d / "toy"), *files)
    assert rc == 0, se
    return str(d / "toy.ibf")


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """64 small peptide bins in 8 families, and three indexes over them: flat, default HIBF, flat with the Murphy reduction"""
    d = tmp_path_factory.mktemp("lib")
    names, _, _ = family_library(str(d), families=8, members=8, seed=3, core=(600, 1200), own=(200, 600), empty=(5,))
    files = [str(d / n) for n in names]
    out = {}
    for key, flags in (("flat", ["-i"]), ("hibf", []), ("murphy", ["-i", "-r", "murphy"])):
        rc, _, se = run("index", "-k", "3", *flags, str(d / key), *files)
        assert rc == 0, se
        out[key] = str(d / (key + ".ibf"))
    return out


def both(tmp_path, index, query, *flags, batch=False, status=0):
    """the same query without and with --gpu-verify, each in a directory of its own: (stdout, files, stderr) twice"""
    res = []
    for name, extra in (("plain", []), ("gpu", ["--gpu-verify"])):
        d = tmp_path / name
        d.mkdir()
        if batch:
            (d / "motifs.tsv").write_text("".join("m%02d\t%s\n" % (i, rx) for i, rx in enumerate(query)))
        rc, so, se = run("query", *(["-f"] if batch else []), *flags, *extra, index, str(d / "motifs.tsv") if batch else query, cwd=str(d))
        assert rc == status, se
        files = {os.path.basename(p): open(p, "rb").read() for p in sorted(glob.glob(str(d / "*"))) if not p.endswith("motifs.tsv")}
        res.append((so, files, se))
    return res


def gpu_verify_line(stderr):
    lines = [json.loads(l) for l in stderr.splitlines() if l.startswith('{"gpu_verify"')]
    assert len(lines) == 1, stderr[-2000:]
    return lines[0]["gpu_verify"]


@pytest.mark.parametrize("motif", ["A(C+|G+)T", "GATTACA"])
def test_dna_rows_of_both_strands_are_unchanged(toy, tmp_path, motif):
    (so, files, _), (so_gpu, files_gpu, se_gpu) = both(tmp_path, toy, motif, "-S", "-o", "hits.tsv")
    assert so_gpu == so and files_gpu == files
    if motif == "A(C+|G+)T":  # three candidate bins of one record each (the reference's README example), both strands
        assert len(files["hits.tsv"].splitlines()) == 6 and b"REVERSE STRAND HIT" in so
        g = gpu_verify_line(se_gpu)
        assert g["pairs_device"] == 3 and g["pairs_host"] == 0 and g["automata_host"] == 0 and g["automata_lds"] == 2
        assert g["records_total"] == 6 and 3 <= g["records_flagged"] <= 6


def test_single_peptide_query_to_stdout(library, tmp_path):
    (so, files, _), (so_gpu, files_gpu, _) = both(tmp_path, library["flat"], "[ST].[RK]", "-t", "2")
    assert so_gpu == so and so.count(b"\n") > 20 and files == files_gpu == {}


@pytest.mark.parametrize("index,threads", [("flat", "1"), ("flat", "4"), ("hibf", "4"), ("murphy", "1")])
def test_batch_files_are_unchanged_and_the_device_did_the_work(library, tmp_path, index, threads):
    from tetrex_amd import host
    batch = MURPHY_BATCH if index == "murphy" else BATCH
    (so, files, se), (so_gpu, files_gpu, se_gpu) = both(tmp_path, library[index], batch, "-S", "-t", threads, batch=True)
    assert so_gpu == so
    assert sorted(files_gpu) == sorted(files) and all(files_gpu[n] == files[n] for n in files)
    assert sum(len(v) > 0 for v in files.values()) >= 5
    # the existing -S lines are still there, and one more
    assert [l.split(":")[0] for l in se.splitlines() if l.startswith("{")] == ['{"queries"', '{"batch_seconds"']
    assert [l.split(":")[0] for l in se_gpu.splitlines() if l.startswith("{")] == ['{"queries"', '{"gpu_verify"', '{"batch_seconds"']
    g = gpu_verify_line(se_gpu)
    # motifs whose automaton is too large stay on the host — exactly those, with exactly their candidate pairs
    reduced = (lambda rx: rx) if index != "murphy" else (lambda rx: "".join(chr(host.reduce_table(1)[ord(c)]) if c.isalpha() else c for c in rx))
    too_large = [i for i, rx in enumerate(batch) if host.regex_automaton("(" + reduced(rx) + ")", True) is None]
    assert too_large == [len(batch) - 1]
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r"^(m\d+)\tBin Count: (\d+)\t", se_gpu, flags=re.M)}
    assert len(counts) == len(batch) and g["automata_host"] == 1
    assert g["pairs_host"] == counts["m%02d" % too_large[0]]
    assert g["pairs_device"] == sum(counts.values()) - g["pairs_host"] > 0
    assert g["automata_lds"] + g["automata_l2"] == len(counts) - 1
    assert 0 < g["records_flagged"] < g["records_total"]


def test_full_batch_on_the_murphy_index(library, tmp_path):
    """the whole batch on the reduced index: the front-end refuses its {m,n} motifs there (exit status 1, no file for them),
    with and without the flag; the others' files are unchanged and their pairs ran on the device"""
    (so, files, se), (so_gpu, files_gpu, se_gpu) = both(tmp_path, library["murphy"], BATCH, "-S", "-t", "4", batch=True, status=1)
    assert so_gpu == so and sorted(files_gpu) == sorted(files) and all(files_gpu[n] == files[n] for n in files)
    assert se.count("[Error] query not searchable") == se_gpu.count("[Error] query not searchable") > 0
    g = gpu_verify_line(se_gpu)
    assert g["pairs_device"] > 0 and g["automata_host"] == 0 and g["pairs_host"] == 0


def test_refused_with_conjunction(toy):
    rc, so, se = run("query", "--gpu-verify", "-c", toy, "ACT:AGT")
    assert rc == 0 and so == b"" and se.startswith("[Error TetRex Query module ") and len(se.splitlines()) == 1
