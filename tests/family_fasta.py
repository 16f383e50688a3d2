"""A seeded FASTA library of peptide families for the tests and measurements of `tetrex index --layout sized --rearrange`:
every member of a family carries the family's core sequence with a few per cent of substitutions, plus sequence of its own;
core and own lengths are spread so that the size-sorted order interleaves the families; a few files hold nothing to index."""
import os

import numpy as np

AA = np.array(list("ACDEFGHIKLMNPQRSTVWY"))


def family_library(d, families=32, members=8, seed=1, core=(3000, 6000), own=(500, 2500), substitutions=0.03, empty=(5, 77, 140, 201)):
    """Writes families * members files f0000.fa ... into directory d.  Returns (file names relative to d, records per file,
    family of each file; -1 for the empty ones, which hold one record shorter than any k)."""
    rng = np.random.default_rng(seed)
    names, recs, fam = [], [], []
    for f in range(families):
        core_seq = rng.choice(AA, size=int(rng.integers(core[0], core[1])))
        for m in range(members):
            b = f * members + m
            mine = core_seq.copy()
            hit = rng.random(mine.size) < substitutions
            mine[hit] = rng.choice(AA, size=int(hit.sum()))
            own_seq = rng.choice(AA, size=int(rng.integers(own[0], own[1])))
            seqs = ["".join(mine), "".join(own_seq)] if b not in empty else ["ACD"]
            name = "f%04d.fa" % b
            with open(os.path.join(d, name), "w") as out:
                out.write("".join(">b%d_%d\n%s\n" % (b, i, s) for i, s in enumerate(seqs)))
            names.append(name)
            recs.append(seqs)
            fam.append(f if b not in empty else -1)
    return names, recs, fam
