"""`tetrex search --window`, `--verify-windows --window-targets` and `--translate --frame-window` on the HIBFs that `tetrex index`
builds from generated FASTA (the default layout and `--layout sized`): the sliding count on a tree (include/txq.h
txq_count_windows) must not change a byte of any command's output.  Every command is run with
TXQ_COUNT_WINDOWS_TREE=0 (the windows as independent queries), with the variable unset, with TXQ_COUNT_WINDOWS_UNIT=3, and with
TXQ_COUNT_WINDOWS_TREE=1 at either unit size, and the outputs are compared as bytes.  What the rows must BE is held by tests/test_gpu_search_window.py,
tests/test_gpu_search_window_targets.py and tests/test_gpu_search_frame_window.py on the same layouts, against the Python
references; this file holds the routes to each other.  Queries: chimeric peptide records — stretches of two bins with 0 to 2
edits between random letters — and contigs that carry such stretches back-translated on either strand."""
import os
import subprocess

import numpy as np
import pytest

import translate_ref as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TETREX = os.path.join(ROOT, "bin", "tetrex")
AMINO = "ACDEFGHIKLMNPQRSTVWY"
K, W, S, EDITS, BINS = 6, 60, 15, 2, 40
FW = 40
LAYOUTS = {"default": [], "sized": ["--layout", "sized"]}
ROUTES = {"independent": {"TXQ_COUNT_WINDOWS_TREE": "0"}, "default": {}, "unit3": {"TXQ_COUNT_WINDOWS_UNIT": "3"},
          "sliding": {"TXQ_COUNT_WINDOWS_TREE": "1"}, "sliding_unit3": {"TXQ_COUNT_WINDOWS_TREE": "1", "TXQ_COUNT_WINDOWS_UNIT": "3"}}
CODONS_OF = {}
for _codon, _aa in T.CODON.items():
    CODONS_OF.setdefault(_aa, []).append(_codon)


def _run(*args, env=None):
    base = {k: v for k, v in os.environ.items() if k not in ("TXQ_COUNT_WINDOWS_TREE", "TXQ_COUNT_WINDOWS_UNIT")}
    r = subprocess.run([TETREX, *args], capture_output=True, text=True, timeout=600, env=dict(base, **(env or {})))
    return r.returncode, r.stdout, r.stderr


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    d = tmp_path_factory.mktemp("search_window_tree")
    rng = np.random.default_rng(77)
    rand = lambda n, res=AMINO: "".join(rng.choice(list(res), size=n))
    seqs, files = [], []
    for b in range(BINS):  # bins of very different sizes: the sized layout splits and merges
        recs = [rand(int(rng.integers(3 * W, 5 * W))) for _ in range(1 + (b % 5 == 0) * 6)]
        seqs.append(recs)
        p = d / ("bin%02d.fa" % b)
        p.write_text("".join(">b%d_%d\n%s\n" % (b, i, r) for i, r in enumerate(recs)))
        files.append(str(p))

    def stretch(b, n, edits):
        rec = seqs[b][int(rng.integers(0, len(seqs[b])))]
        at = int(rng.integers(0, len(rec) - n + 1))
        s = list(rec[at:at + n])
        for _ in range(edits):
            s[int(rng.integers(1, n - 1))] = AMINO[int(rng.integers(0, 20))]
        return "".join(s)
    back = lambda pep: "".join(CODONS_OF[a][int(rng.integers(0, len(CODONS_OF[a])))] for a in pep)
    peptides, contigs = [], []
    for q in range(8):
        a, b = (int(x) for x in rng.choice(BINS, size=2, replace=False))
        peptides.append(("chimera%d" % q, rand(int(rng.integers(0, 2 * S))) + stretch(a, 2 * W + S, q % 3) + rand(W) + stretch(b, W + 2 * S, (q + 1) % 3) + rand(S)))
        contigs.append(("contig%d" % q, rand(int(rng.integers(60, 90)), "ACGT") + back(stretch(a, 2 * FW, q % 3)) + rand(70, "ACGT")
                        + T.reverse_complement(back(stretch(b, 2 * FW, (q + 1) % 3))) + rand(int(rng.integers(60, 90)), "ACGT")))
    pf, cf = d / "peptides.fa", d / "contigs.fa"
    pf.write_text("".join(">%s\n%s\n" % r for r in peptides))
    cf.write_text("".join(">%s\n%s\n" % r for r in contigs))
    indexes = {}
    for lay, flags in LAYOUTS.items():
        rc, so, se = _run("index", "-k", str(K), *flags, str(d / lay), *files)
        assert rc == 0 and os.path.exists(d / (lay + ".ibf")), se
        indexes[lay] = str(d / (lay + ".ibf"))
    return dict(indexes=indexes, peptides=str(pf), contigs=str(cf))


COMMANDS = {
    "window": lambda s: ("--window", str(W), "--step", str(S), "-e", str(EDITS), "--counts", s["peptides"]),
    "verify_window_targets": lambda s: ("--window", str(W), "--step", str(S), "-e", str(EDITS), "--counts", "--verify-windows", "--window-targets", s["peptides"]),
    "frame_window": lambda s: ("--translate", "--frame-window", str(FW), "-e", str(EDITS), "--counts", s["contigs"]),
}


@pytest.mark.parametrize("command", list(COMMANDS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_routes_write_identical_bytes(setup, layout, command):
    *flags, queries = COMMANDS[command](setup)
    out = {}
    for route, env in ROUTES.items():
        rc, so, se = _run("search", *flags, setup["indexes"][layout], queries, env=env)
        assert rc == 0, (route, se)
        out[route] = so
    assert out["independent"], "no rows"
    assert len(out["independent"].splitlines()) >= 8  # (every query record carries two planted stretches)
    for route in ROUTES:
        assert out[route] == out["independent"], route
