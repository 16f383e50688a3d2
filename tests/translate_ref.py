"""Python restatement of six-frame translated search (`tetrex search --translate`; include/txq.h txq_translate).

Nucleotides A C G T U in either case (U reads as T), any other byte ambiguous.  Frame f = 0..5 is +1 +2 +3 -1 -2 -3: frames +1..+3
read the record from offset 0, 1, 2, frames -1..-3 its reverse complement (ambiguous stays ambiguous) from offset 0, 1, 2; a
frame with offset o over L bytes has (L - o) // 3 codons.  NCBI table 1; a codon with an ambiguous byte is X; stops are *.
The values of a frame: host.record_values_array (the index's own encoder) on every maximal stop-free segment of at least k
residues, concatenated.  Query 6 r + f is frame f of record r.  Thresholds: the plain rules with n = n_f; a frame with n_f = 0
or t = 0 reports nothing.  Counting itself is tests/search_ref.py's."""
import numpy as np

from helpers import oracle_ibf_from_words
from search_ref import TreeRef, flat_search, csr, unpack

FRAMES = ("+1", "+2", "+3", "-1", "-2", "-3")
TABLE1 = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"  # T, C, A, G order
_ORDER = "TCAG"
CODON = {a + b + c: TABLE1[16 * i + 4 * j + l] for i, a in enumerate(_ORDER) for j, b in enumerate(_ORDER) for l, c in enumerate(_ORDER)}
_COMPLEMENT = {"A": "T", "T": "A", "C": "G", "G": "C"}
_LETTER = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "a": "A", "c": "C", "g": "G", "t": "T", "u": "T"}


def _text(seq):
    return seq.decode("latin-1") if isinstance(seq, (bytes, bytearray)) else seq


def normalise(seq):
    """upper case, U -> T, every other byte -> N (byte by byte: the length never changes)"""
    return "".join(_LETTER.get(c, "N") for c in _text(seq))


def reverse_complement(seq):
    return "".join(_COMPLEMENT.get(c, "N") for c in reversed(normalise(seq)))


def translate_frame(seq, f):
    s = normalise(seq) if f < 3 else reverse_complement(seq)
    o = f % 3
    return "".join(CODON.get(s[p:p + 3], "X") for p in range(o, len(s) - 2, 3))


def frame_values(seq, f, k, reduction=0):
    from tetrex_amd import host
    parts = [host.record_values_array(seg, k, dna=False, reduction=reduction) for seg in translate_frame(seq, f).split("*") if len(seg) >= k]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)


def translated_values(seq, k, reduction=0):
    """(values, offsets[7]) of one record: the six frames one after the other"""
    return csr([frame_values(seq, f, k, reduction) for f in range(6)])


def translate_records(records, k, reduction=0):
    """(values, offsets[6 n + 1]) of a list of records: query 6 r + f"""
    return csr([frame_values(s, f, k, reduction) for s in records for f in range(6)])


def bound(lengths, k):
    return sum(2 * max(0, (L - o) // 3 - k + 1) for L in lengths for o in range(3) if L >= o)


def expected_rows(oracle, index_path, records, k, reduction, threshold_of):
    """rows (name, bin path, frame, count, n_f) of `tetrex search --translate` for records [(name, sequence)] on an index file,
    and the names of the records none of whose frames is searched"""
    from tetrex_amd import host
    ix = host.IndexFile.load(index_path)
    d = ix.describe()
    queries, owner = [], []
    skipped = []
    for name, s in records:
        searched = False
        for f in range(6):
            v = frame_values(s, f, k, reduction)
            t = threshold_of(v.size) if v.size else 0
            if t > 0:
                searched = True
                queries.append((v, t))
                owner.append((name, f))
        if not searched:
            skipped.append(name)
    values, offsets = csr([v for v, _ in queries])
    thr = np.array([t for _, t in queries], dtype=np.uint32)
    if d["is_hibf"]:
        descs = []
        for i, f in enumerate(d["ibfs"]):
            nxt, tbu = ix.maps(i)
            descs.append(dict(bins=f["bins"], bin_size=f["bin_size"], hash_funs=f["hash_funs"], words=ix.words(i), next_ibf_id=nxt, tb_to_user=tbu))
        hits, counts = TreeRef(oracle, d["bins"], descs).search(values, offsets, thr)
    else:
        f = d["ibfs"][0]
        hits, counts = flat_search(oracle_ibf_from_words(oracle, f["bins"], f["bin_size"], f["hash_funs"], ix.words(0)), f["bins"], values, offsets, thr)
    bits = unpack(hits)
    rows = []
    for q, (name, f) in enumerate(owner):
        for u in np.flatnonzero(bits[q]):
            rows.append((name, d["paths"][u], FRAMES[f], int(counts[q, u]), int(queries[q][0].size)))
    return rows, skipped
