"""ctypes view of the C++ host front-end (include/txh.h, tetrex_amd/libtetrex_host.so)."""
import ctypes as C
import os
import struct

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# TETREX_HOST_LIB: load another build of the same library (e.g. an AddressSanitizer build on the CPU)
LIB_PATH = os.environ.get("TETREX_HOST_LIB") or os.path.join(_HERE, "libtetrex_host.so")
_LIB = None
i32p = C.POINTER(C.c_int32)
u64p = C.POINTER(C.c_uint64)


class HostError(RuntimeError):
    pass


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: run `make`" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.txh_last_error.restype = C.c_char_p
        L.txh_translate.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
        L.txh_preprocess.argtypes = [C.c_char_p, C.c_int, C.c_uint, C.c_uint, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
        L.txh_kgraph.argtypes = [C.c_char_p, C.c_uint, C.c_int, i32p, i32p, i32p, C.c_int32]
        L.txh_compile_batch.argtypes = [C.POINTER(C.c_char_p), C.c_size_t, C.c_int, C.c_uint, C.c_uint, C.c_uint64,
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
        L.txh_blob_data.restype = C.c_void_p
        L.txh_blob_data.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
        L.txh_blob_stats.argtypes = [C.c_void_p, u64p, C.c_size_t]
        L.txh_blob_free.argtypes = [C.c_void_p]
        L.txh_record_values.restype = C.c_int64
        L.txh_record_values.argtypes = [C.c_int, C.c_uint, C.c_uint, C.c_char_p, C.c_size_t, C.c_int, u64p, C.c_size_t]
        _LIB = L
    return _LIB


def _err():
    return HostError(lib().txh_last_error().decode(errors="replace"))


def translate(rx):
    buf = C.create_string_buffer(1 << 16)
    if lib().txh_translate(rx.encode(), buf, len(buf)) < 0:
        raise _err()
    return buf.value.decode()


def preprocess(rx, dna, k, reduction=0):
    a = C.create_string_buffer(1 << 16)
    b = C.create_string_buffer(1 << 16)
    if lib().txh_preprocess(rx.encode(), int(dna), k, reduction, a, len(a), b, len(b)) < 0:
        raise _err()
    return a.value.decode(), b.value.decode()


def kgraph(postfix, k, reduced=False):
    cap = 1 << 18
    lab, na, nb = (C.c_int32 * cap)(), (C.c_int32 * cap)(), (C.c_int32 * cap)()
    n = lib().txh_kgraph(postfix.encode(), k, int(reduced), lab, na, nb, cap)
    if n < 0:
        raise _err()
    return dict(labels=list(lab[:n]), succ=list(zip(na[:n], nb[:n])))


def kgraph_fused(postfix, k):
    """The k-graph the expansion works on: unions of single residues fused into class nodes (include/txh.h)."""
    L = lib()
    i32p = C.POINTER(C.c_int32)
    L.txh_kgraph_fused.argtypes = [C.c_char_p, C.c_uint, i32p, i32p, i32p, C.c_int32, C.c_char_p, C.c_size_t]
    cap = 1 << 18
    lab, na, nb = (C.c_int32 * cap)(), (C.c_int32 * cap)(), (C.c_int32 * cap)()
    buf = C.create_string_buffer(1 << 20)
    n = L.txh_kgraph_fused(postfix.encode(), k, lab, na, nb, cap, buf, len(buf))
    if n < 0:
        raise _err()
    return dict(labels=list(lab[:n]), succ=list(zip(na[:n], nb[:n])), members=buf.value.decode().split("\n")[:n])


def kgraph_dot(postfix, k, reduced=False, augment=False):
    L = lib()
    L.txh_kgraph_dot.argtypes = [C.c_char_p, C.c_uint, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(1 << 22)
    if L.txh_kgraph_dot(postfix.encode(), k, int(reduced), int(augment), buf, len(buf)) < 0:
        raise _err()
    return buf.value.decode()


def compile_batch(regexes, dna, k, reduction, bins):
    """Returns (blob bytes, status list, stats array [n,4] = ops, slots, states, probe ops)."""
    n = len(regexes)
    arr = (C.c_char_p * n)(*[r.encode() for r in regexes])
    status = (C.c_int * n)()
    h = C.c_void_p()
    rc = lib().txh_compile_batch(arr, n, int(dna), k, reduction, bins, C.byref(h), status)
    if rc < 0:
        raise _err()
    try:
        size = C.c_size_t()
        p = lib().txh_blob_data(h, C.byref(size))
        blob = C.string_at(p, size.value)
        stats = np.zeros((n, 4), dtype=np.uint64)
        if n and lib().txh_blob_stats(h, stats.ctypes.data_as(u64p), n) != 0:
            raise _err()
    finally:
        lib().txh_blob_free(h)
    return blob, list(status), stats


STAGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_size_t,
                       C.POINTER(C.c_uint8))


class GapOptions(C.Structure):
    _fields_ = [("augment", C.c_int), ("dgram_loaded", C.c_int), ("min_gap", C.c_uint64), ("max_gap", C.c_uint64)]


def dgram_values(seq, min_gap, max_gap):
    L = lib()
    L.txh_dgram_values.restype = C.c_int64
    L.txh_dgram_values.argtypes = [C.c_char_p, C.c_size_t, C.c_uint64, C.c_uint64, u64p, C.c_size_t]
    s = seq.encode() if isinstance(seq, str) else seq
    cap = max(1, len(s) * (max_gap - min_gap + 1))
    out = np.zeros(cap, dtype=np.uint64)
    n = L.txh_dgram_values(s, len(s), min_gap, max_gap, out.ctypes.data_as(u64p), cap)
    return out[:n].copy()


class DenseOptions(C.Structure):
    _fields_ = [("enabled", C.c_int), ("min_states", C.c_uint32), ("sparse_below", C.c_uint32), ("max_blocks", C.c_uint32),
                ("slot_bytes", C.c_uint64), ("pool_bytes", C.c_uint64), ("tracked", C.c_int)]


def run_staged(regexes, dna, k, reduction, bins, stage, ops_per_query_per_stage=0, ops_per_stage=0, gaps=None, dense=None):
    """Drive the C++ staged expansion with a Python executor.

    stage(blob: bytes, query_program: list, query_slot: list) -> iterable of answers: False/0 = the slot has no bit set,
    True/1 = alive, or 1 + floor(log2(bits set)) as txq_session_stage answers (what the expansion reads mask fills from).
    dense: None, or dict(min_states=, sparse_below=, max_blocks=, slot_bytes=, pool_bytes=, tracked=) to switch dense DP
    steps on (the executor then gets version-4 blobs); tracked: 1 = the executor keeps live lists, 2 = every query uses them."""
    L = lib()
    L.txh_run_staged_dense.argtypes = [C.POINTER(C.c_char_p), C.c_size_t, C.c_int, C.c_uint, C.c_uint, C.c_uint64, C.c_size_t,
                                       C.c_size_t, C.POINTER(GapOptions), C.POINTER(DenseOptions), STAGE_FN, C.c_void_p,
                                       C.POINTER(C.c_int), u64p]
    d = None
    if dense is not None:
        d = DenseOptions(1, dense.get("min_states", 0), dense.get("sparse_below", 0), dense.get("max_blocks", 0),
                         dense.get("slot_bytes", 0), dense.get("pool_bytes", 0), int(dense.get("tracked", 0)))
    g = None
    if gaps is not None:  # dict(augment=, dgram_loaded=, min_gap=, max_gap=)
        g = GapOptions(int(gaps.get("augment", 0)), int(gaps.get("dgram_loaded", 0)), gaps.get("min_gap", 0), gaps.get("max_gap", 0))
    n = len(regexes)
    arr = (C.c_char_p * n)(*[r.encode() for r in regexes])
    status = (C.c_int * n)()
    stats = (C.c_uint64 * 8)()
    err = []

    def cb(user, blob, size, qp, qs, nq, alive):
        try:
            res = stage(C.string_at(blob, size), [qp[i] for i in range(nq)], [qs[i] for i in range(nq)])
            for i, a in enumerate(res):
                alive[i] = min(255, int(a))
            return 0
        except Exception as e:  # noqa: BLE001 - reported through the return code
            err.append(e)
            return -1

    rc = L.txh_run_staged_dense(arr, n, int(dna), k, reduction, bins, ops_per_query_per_stage, ops_per_stage,
                                C.byref(g) if g is not None else None, C.byref(d) if d is not None else None, STAGE_FN(cb), None,
                                status, stats)
    if err:
        raise err[0]
    if rc < 0:
        raise _err()
    keys = ("stages", "ops", "kmers", "states", "pruned", "feedback_queries", "expand_us", "execute_us")
    return list(status), dict(zip(keys, (int(x) for x in stats)))


def join_shard_masks(mask_words, shard_word0, shard_masks):
    """host/compiler.hpp join_shard_masks: shard r = array [n, words_r] holding words [shard_word0[r], +words_r) of every mask."""
    L = lib()
    L.txh_join_shard_masks.argtypes = [C.c_size_t, C.c_uint64, C.c_size_t, u64p, u64p, C.POINTER(u64p), u64p]
    R = len(shard_masks)
    parts = [np.ascontiguousarray(m, dtype=np.uint64) for m in shard_masks]
    n = parts[0].shape[0] if R else 0
    w0 = np.array(shard_word0, dtype=np.uint64)
    ws = np.array([p.shape[1] for p in parts], dtype=np.uint64)
    ptrs = (u64p * R)(*[p.ctypes.data_as(u64p) for p in parts])
    out = np.zeros((n, mask_words), dtype=np.uint64)
    if L.txh_join_shard_masks(n, mask_words, R, w0.ctypes.data_as(u64p), ws.ctypes.data_as(u64p), ptrs, out.ctypes.data_as(u64p)) != 0:
        raise _err()
    return out


def regex_find_all(pattern, text, posix):
    """The verification matcher (host/matcher.hpp): [(start, length), ...] of successive non-overlapping matches."""
    L = lib()
    L.txh_regex_find_all.restype = C.c_int64
    L.txh_regex_find_all.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_size_t, u64p, C.c_size_t]
    t = text.encode() if isinstance(text, str) else text
    cap = 2 * (len(t) + 2)
    out = np.zeros(cap, dtype=np.uint64)
    n = L.txh_regex_find_all(pattern.encode(), int(posix), t, len(t), out.ctypes.data_as(u64p), cap)
    if n < 0:
        raise _err()
    return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)]


def regex_required_literal(pattern, posix=True):
    """The matcher's prefilter string for `pattern` (host/matcher.hpp required_literal)."""
    L = lib()
    L.txh_regex_required_literal.restype = C.c_int64
    L.txh_regex_required_literal.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(4096)
    n = L.txh_regex_required_literal(pattern.encode(), int(posix), buf, 4096)
    if n < 0:
        raise _err()
    return buf.raw[:n].decode()


REGEX_REFUSED = 0xFFFFFFFE
REGEX_UNBOUNDED = 0xFFFFFFFF


def regex_automaton(pattern, posix, strand=0, byte_map=None):
    """txh_regex_automaton: the pattern as the flat automaton of include/txq_regex.h (bytes), or None where it has more than
    65 535 states.  strand 1: the reversed pattern; byte_map: 256 bytes applied to the text first (None: the identity)."""
    L = lib()
    L.txh_regex_automaton.restype = C.c_int64
    L.txh_regex_automaton.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    bm = None if byte_map is None else np.ascontiguousarray(byte_map, dtype=np.uint8)
    if bm is not None and bm.size != 256:
        raise HostError("regex_automaton: byte_map must have 256 entries")
    cap = 1 << 16
    for _ in range(2):
        out = np.zeros(cap, dtype=np.uint8)
        n = L.txh_regex_automaton(pattern.encode(), int(posix), int(strand), None if bm is None else bm.ctypes.data, out.ctypes.data, cap)
        if n < 0:
            raise _err()
        if n == 0:
            return None
        if n <= cap:
            return out[:n].tobytes()
        cap = int(n)
    raise HostError("regex_automaton: the blob changed its size")


def reduce_table(reduction):
    """txh_reduce_table: byte -> letter of a peptide reduction (1 murphy, 2 li), as 256 uint8"""
    L = lib()
    L.txh_reduce_table.argtypes = [C.c_uint, C.c_void_p]
    out = np.zeros(256, dtype=np.uint8)
    if L.txh_reduce_table(reduction, out.ctypes.data) < 0:
        raise _err()
    return out


def regex_automaton_header(blob):
    """the header fields of an automaton blob (include/txq_regex.h) as a dict"""
    f = struct.unpack_from("<8I", blob, 0)
    return dict(magic=f[0], n_states=f[1], n_classes=f[2], start_begin=f[3], start_mid=f[4], lmax=f[5], total_bytes=f[6])


def regex_filter_arrays(automata, records, groups, pairs):
    """the arguments of regex_filter as contiguous arrays: (arena, automaton offsets, text, record offsets, group offsets,
    pairs (n, 2) uint32, bitmap word offsets, bitmap words).  An automaton starts at a multiple of 16 bytes of the arena;
    a pair that names a group out of range gets no words."""
    if isinstance(automata, tuple):
        arena, ao = automata
    else:
        blobs = [bytes(a) + b"\0" * (-len(a) % 16) for a in automata]
        arena, ao = _byte_records(blobs)
    txt, ro = records if isinstance(records, tuple) else _byte_records(records)
    arena, txt = np.ascontiguousarray(arena, dtype=np.uint8), np.ascontiguousarray(txt, dtype=np.uint8)
    ao, ro = np.ascontiguousarray(ao, dtype=np.uint64), np.ascontiguousarray(ro, dtype=np.uint64)
    go = np.ascontiguousarray(groups, dtype=np.uint64)
    pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    if ao.size < 1 or ro.size < 1 or go.size < 1 or int(ao[-1]) > arena.size or int(ro[-1]) > txt.size:
        raise HostError("regex_filter: offsets and bytes disagree")
    words = [(int(go[g + 1]) - int(go[g]) + 31) // 32 if g + 1 < go.size and go[g + 1] >= go[g] else 0 for g in pr[:, 1].tolist()]
    oo = np.zeros(pr.shape[0] + 1, dtype=np.uint64)
    oo[1:] = np.cumsum(words, dtype=np.uint64)
    return arena, ao, txt, ro, go, pr, oo, int(oo[-1])


def regex_filter_unpack(go, pr, oo, out, status):
    """per pair a boolean array over its group's records (empty for a refused pair)"""
    res = []
    for i, (_, g) in enumerate(pr.tolist()):
        if status[i] != 0:
            res.append(np.zeros(0, dtype=bool))
            continue
        n = int(go[g + 1]) - int(go[g])
        w = out[int(oo[i]):int(oo[i + 1])]
        res.append(np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool))
    return res


def regex_filter(automata, records, groups, pairs, max_serial=0, return_status=False):
    """txh_regex_filter: which records of a group does an automaton match (include/txh.h)?  automata: blobs of
    regex_automaton; records: list of bytes/str, or (uint8 array, uint64 offsets); groups: uint64 offsets into the records;
    pairs: rows of (automaton, group).  Returns one boolean array per pair (and the status array if asked for)."""
    L = lib()
    L.txh_regex_filter.argtypes = [C.c_void_p, u64p, C.c_size_t, C.c_size_t, C.c_void_p, u64p, C.c_size_t, C.c_size_t, u64p, C.c_size_t,
                                   C.c_void_p, C.c_size_t, u64p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p]
    arena, ao, txt, ro, go, pr, oo, n_words = regex_filter_arrays(automata, records, groups, pairs)
    out = np.zeros(max(1, n_words), dtype=np.uint32)
    status = np.zeros(max(1, pr.shape[0]), dtype=np.uint32)
    rc = L.txh_regex_filter(arena.ctypes.data, ao.ctypes.data_as(u64p), ao.size - 1, arena.size, txt.ctypes.data, ro.ctypes.data_as(u64p),
                            ro.size - 1, txt.size, go.ctypes.data_as(u64p), go.size - 1, pr.ctypes.data, pr.shape[0], oo.ctypes.data_as(u64p),
                            out.ctypes.data, n_words, max_serial, status.ctypes.data)
    if rc < 0:
        raise _err()
    status = status[:pr.shape[0]]
    res = regex_filter_unpack(go, pr, oo, out, status)
    return (res, status) if return_status else res


def record_values(seq, k, dna=True, reduction=0, wraparound=False):
    s = seq.encode() if isinstance(seq, str) else seq
    cap = len(s) + 2
    out = np.zeros(cap, dtype=np.uint64)
    n = lib().txh_record_values(int(dna), k, reduction, s, len(s), int(wraparound), out.ctypes.data_as(u64p), cap)
    return [int(x) for x in out[:n]]


def record_values_array(seq, k, dna=True, reduction=0, wraparound=False):
    """record_values as a uint64 numpy array (no per-value Python objects: for whole sequences)."""
    s = seq.encode() if isinstance(seq, str) else seq
    cap = len(s) + 2
    out = np.zeros(cap, dtype=np.uint64)
    n = lib().txh_record_values(int(dna), k, reduction, s, len(s), int(wraparound), out.ctypes.data_as(u64p), cap)
    return out[:n].copy()


FRAMES = ("+1", "+2", "+3", "-1", "-2", "-3")


def translate_frame(seq, frame):
    """One of the six frames (0..5 = +1 +2 +3 -1 -2 -3) of a nucleotide record as residue letters (NCBI table 1; X for a codon
    with an ambiguous byte, * for a stop)."""
    L = lib()
    L.txh_translate_frame.restype = C.c_int64
    L.txh_translate_frame.argtypes = [C.c_char_p, C.c_size_t, C.c_uint, C.c_char_p, C.c_size_t]
    s = seq.encode() if isinstance(seq, str) else bytes(seq)
    buf = C.create_string_buffer(len(s) // 3 + 1)
    n = L.txh_translate_frame(s, len(s), frame, buf, len(buf))
    if n < 0:
        raise _err()
    return buf.raw[:n].decode()


def translated_values(seq, k, reduction=0):
    """txh_translated_values: the k-mer values of the six frames of one nucleotide record for a peptide index, frame after
    frame.  Returns (values uint64[], offsets uint64[7])."""
    L = lib()
    L.txh_translated_values.restype = C.c_int64
    L.txh_translated_values.argtypes = [C.c_uint, C.c_uint, C.c_char_p, C.c_size_t, u64p, C.c_size_t, u64p]
    s = seq.encode() if isinstance(seq, str) else bytes(seq)
    cap = 2 * len(s) + 8
    out = np.zeros(cap, dtype=np.uint64)
    off = np.zeros(7, dtype=np.uint64)
    n = L.txh_translated_values(k, reduction, s, len(s), out.ctypes.data_as(u64p), cap, off.ctypes.data_as(u64p))
    if n < 0:
        raise _err()
    assert n <= cap
    return out[:n].copy(), off


def peptide_codes(reduction=0):
    """The 256-byte residue code table of the peptide encoder (what capi.translate takes as `codes`)."""
    L = lib()
    L.txh_peptide_codes.argtypes = [C.c_uint, C.POINTER(C.c_uint8)]
    out = np.zeros(256, dtype=np.uint8)
    if L.txh_peptide_codes(reduction, out.ctypes.data_as(C.POINTER(C.c_uint8))) < 0:
        raise _err()
    return out


def edit_search(patterns, records, groups, pairs, codes, threads=1):
    """txh_edit_search: approximate matching by edit distance on the host (include/txh.h).  patterns, records: lists of
    bytes/str, or (uint8 array, uint64 offsets); groups: uint64 offsets into the records; pairs: (n, 3) of (pattern, group,
    cap); codes: the 256-byte class table.  Returns an (n, 3) uint32 array of (distance, record, end)."""
    L = lib()
    L.txh_edit_search.argtypes = [C.c_void_p, u64p, C.c_size_t, C.c_void_p, u64p, C.c_size_t, u64p, C.c_size_t, C.c_void_p, C.c_size_t,
                                  C.c_void_p, C.c_uint, C.c_void_p]
    pat, po = patterns if isinstance(patterns, tuple) else _byte_records(patterns)
    txt, ro = records if isinstance(records, tuple) else _byte_records(records)
    pat, txt = np.ascontiguousarray(pat, dtype=np.uint8), np.ascontiguousarray(txt, dtype=np.uint8)
    po, ro = np.ascontiguousarray(po, dtype=np.uint64), np.ascontiguousarray(ro, dtype=np.uint64)
    go = np.ascontiguousarray(groups, dtype=np.uint64)
    pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 3)
    cd = np.ascontiguousarray(codes, dtype=np.uint8)
    if cd.size != 256 or po.size < 1 or ro.size < 1 or go.size < 1 or int(po[-1]) > pat.size or int(ro[-1]) > txt.size:
        raise HostError("edit_search: offsets, bytes and class table disagree")
    out = np.zeros((pr.shape[0], 3), dtype=np.uint32)
    rc = L.txh_edit_search(pat.ctypes.data, po.ctypes.data_as(u64p), po.size - 1, txt.ctypes.data, ro.ctypes.data_as(u64p), ro.size - 1,
                           go.ctypes.data_as(u64p), go.size - 1, pr.ctypes.data, pr.shape[0], cd.ctypes.data, threads, out.ctypes.data)
    if rc < 0:
        raise _err()
    return out


def edit_targets(patterns, records, groups, pairs, codes, threads=1, capacity=None):
    """txh_edit_targets: every record of a pair's group within the cap, on the host (include/txh.h; the semantics are in
    include/txq.h at txq_edit_targets_device).  The arguments of edit_search.  Returns (hits, total): hits an (n, 4) uint32 array
    of (pair, distance, record, end) by pair, then by record, and total the number of hits; with a capacity only the first
    `capacity` rows are returned, total still counting all."""
    L = lib()
    L.txh_edit_targets.argtypes = [C.c_void_p, u64p, C.c_size_t, C.c_void_p, u64p, C.c_size_t, u64p, C.c_size_t, C.c_void_p, C.c_size_t,
                                   C.c_void_p, C.c_uint, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
    pat, po = patterns if isinstance(patterns, tuple) else _byte_records(patterns)
    txt, ro = records if isinstance(records, tuple) else _byte_records(records)
    pat, txt = np.ascontiguousarray(pat, dtype=np.uint8), np.ascontiguousarray(txt, dtype=np.uint8)
    po, ro = np.ascontiguousarray(po, dtype=np.uint64), np.ascontiguousarray(ro, dtype=np.uint64)
    go = np.ascontiguousarray(groups, dtype=np.uint64)
    pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 3)
    cd = np.ascontiguousarray(codes, dtype=np.uint8)
    if cd.size != 256 or po.size < 1 or ro.size < 1 or go.size < 1 or int(po[-1]) > pat.size or int(ro[-1]) > txt.size:
        raise HostError("edit_targets: offsets, bytes and class table disagree")
    room = 1024 if capacity is None else int(capacity)
    while True:
        hits, total = np.zeros((room, 4), dtype=np.uint32), C.c_uint64(0)
        rc = L.txh_edit_targets(pat.ctypes.data, po.ctypes.data_as(u64p), po.size - 1, txt.ctypes.data, ro.ctypes.data_as(u64p), ro.size - 1,
                                go.ctypes.data_as(u64p), go.size - 1, pr.ctypes.data, pr.shape[0], cd.ctypes.data, threads, hits.ctypes.data, room,
                                C.byref(total))
        if rc < 0:
            raise _err()
        if capacity is not None or total.value <= room:
            return hits[:min(total.value, room)].copy(), int(total.value)
        room = int(total.value)


EDIT_ALIGN_OPS = "=XID"


def decode_alignments(words, max_errors):
    """The answers of edit_align in the layout of include/txq.h (2 max_errors + 3 uint32 a pair) as (start uint32[n], list of
    [(op, length), ...]) with op one of "=XID"; a pair whose start is 0xFFFFFFFF or 0xFFFFFFFE has no runs."""
    words = np.asarray(words, dtype=np.uint32).reshape(-1, 2 * int(max_errors) + 3)
    runs = []
    for row in words:
        n = int(row[1]) if int(row[0]) < 0xFFFFFFFE else 0
        runs.append([(EDIT_ALIGN_OPS[int(w) & 3], int(w) >> 2) for w in row[2:2 + n]])
    return words[:, 0].copy(), runs


def edit_align(patterns, records, groups, pairs, results, codes, max_errors, threads=1, raw=False):
    """txh_edit_align: start and alignment of the pairs a search confirmed, on the host (include/txh.h; the semantics are in
    include/txq.h at txq_edit_align_device).  The arguments of edit_search, then results, the (n, 3) array a search returned, and
    max_errors, which sizes the answers.  Returns (start uint32[n], list of [(op, length), ...]); raw=True: the (n, 2 max_errors
    + 3) uint32 words instead (a pair that is not aligned keeps the 0xA5A5A5A5 fill behind its marker)."""
    L = lib()
    L.txh_edit_align.argtypes = [C.c_void_p, u64p, C.c_size_t, C.c_void_p, u64p, C.c_size_t, u64p, C.c_size_t, C.c_void_p, C.c_size_t,
                                 C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_void_p]
    pat, po = patterns if isinstance(patterns, tuple) else _byte_records(patterns)
    txt, ro = records if isinstance(records, tuple) else _byte_records(records)
    pat, txt = np.ascontiguousarray(pat, dtype=np.uint8), np.ascontiguousarray(txt, dtype=np.uint8)
    po, ro = np.ascontiguousarray(po, dtype=np.uint64), np.ascontiguousarray(ro, dtype=np.uint64)
    go = np.ascontiguousarray(groups, dtype=np.uint64)
    pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 3)
    res = np.ascontiguousarray(results, dtype=np.uint32).reshape(-1, 3)
    cd = np.ascontiguousarray(codes, dtype=np.uint8)
    if (cd.size != 256 or po.size < 1 or ro.size < 1 or go.size < 1 or int(po[-1]) > pat.size or int(ro[-1]) > txt.size
            or res.shape != pr.shape or not 0 <= int(max_errors) <= 1 << 24):
        raise HostError("edit_align: offsets, bytes, results and class table disagree")
    out = np.full((pr.shape[0], 2 * int(max_errors) + 3), 0xA5A5A5A5, dtype=np.uint32)
    rc = L.txh_edit_align(pat.ctypes.data, po.ctypes.data_as(u64p), po.size - 1, txt.ctypes.data, ro.ctypes.data_as(u64p), ro.size - 1,
                          go.ctypes.data_as(u64p), go.size - 1, pr.ctypes.data, pr.shape[0], res.ctypes.data, cd.ctypes.data, int(max_errors),
                          threads, out.ctypes.data)
    if rc < 0:
        raise _err()
    return out if raw else decode_alignments(out, max_errors)


def _byte_records(records):
    recs = [r.encode() if isinstance(r, str) else bytes(r) for r in records]
    offsets = np.zeros(len(recs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in recs])
    return np.frombuffer(b"".join(recs), dtype=np.uint8), offsets


def parse_blob(blob):
    """Decode a txq_program.h blob (version 1, 2 or 4): (kmers uint64[], [(n_slots, ops array [n,4] =
    kmer,dst,a,b)]).  Version-2/4 ops are in level order, which is also a valid sequential order.
    The dense table of a version-4 blob: blob_dense()."""
    magic, ver = struct.unpack_from("<2I", blob, 0)
    assert magic == 0x50515854 and ver in (1, 2, 4)
    if ver == 1:
        _, _, n_prog, n_kmers, n_ops, _, k_off, p_off, o_off = struct.unpack_from("<6I3Q", blob, 0)
        stride = 4
    else:
        _, _, n_prog, n_kmers, n_ops, _, k_off, p_off, o_off, _, _ = struct.unpack_from("<6I5Q", blob, 0)
        stride = 6
    kmers = np.frombuffer(blob, dtype="<u8", count=n_kmers, offset=k_off)
    progs = np.frombuffer(blob, dtype="<u4", count=n_prog * stride, offset=p_off).reshape(n_prog, stride)
    ops = np.frombuffer(blob, dtype="<u4", count=n_ops * 4, offset=o_off).reshape(n_ops, 4)
    out = []
    for row in progs:
        first, cnt, n_slots = int(row[0]), int(row[1]), int(row[2])
        out.append((n_slots, ops[first:first + cnt]))
    return kmers, out


def blob_aux_kmers(blob):
    """Number of trailing k-mer table entries that belong to the auxiliary (d-gram) index."""
    magic, ver = struct.unpack_from("<2I", blob, 0)
    return struct.unpack_from("<6I5Q", blob, 0)[-1] if ver >= 2 else 0


DENSE_OP = 0xFFFFFFFE
DENSE_SLOT_BIT = 0x40000000


def blob_dense(blob):
    """Dense part of a version-4 blob: (params dict(k, bits, alphabet, canonical), table uint32[n, 16] =
    kind, dst, src, r_mask, shape[11], reserved, per-program dense slot counts); None for older versions."""
    magic, ver = struct.unpack_from("<2I", blob, 0)
    if ver != 4:
        return None
    _, _, n_prog, _, _, _, _, p_off, _, _, _, d_off, n_dense, k, bits, alphabet, canonical, _ = struct.unpack_from("<6I5QQ6I", blob, 0)
    table = np.frombuffer(blob, dtype="<u4", count=n_dense * 16, offset=d_off).reshape(n_dense, 16)
    progs = np.frombuffer(blob, dtype="<u4", count=n_prog * 6, offset=p_off).reshape(n_prog, 6)
    return dict(k=k, bits=bits, alphabet=alphabet, canonical=canonical), table, [int(r[5]) for r in progs]


def blob_levels(blob):
    """Level tables of a version-2/4 blob: list of per-program end-index lists."""
    magic, ver = struct.unpack_from("<2I", blob, 0)
    if ver < 2:
        return None
    _, _, n_prog, n_kmers, n_ops, n_lv, k_off, p_off, o_off, l_off, _ = struct.unpack_from("<6I5Q", blob, 0)
    progs = np.frombuffer(blob, dtype="<u4", count=n_prog * 6, offset=p_off).reshape(n_prog, 6)
    lv = np.frombuffer(blob, dtype="<u4", count=n_lv, offset=l_off)
    return [list(int(x) for x in lv[int(r[3]):int(r[3]) + int(r[4])]) for r in progs]


# ---- .ibf index files ------------------------------------------------------------------------
def _index_api():
    L = lib()
    if not hasattr(L, "_index_ready"):
        L.txh_index_parse.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.txh_index_from_ibf.argtypes = [C.c_uint, C.c_int, C.c_uint, C.c_uint, C.c_uint64, C.c_uint64, u64p, C.c_char_p,
                                         C.POINTER(C.c_void_p)]
        L.txh_index_describe.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        L.txh_index_words.restype = C.c_int64
        L.txh_index_words.argtypes = [C.c_void_p, C.c_uint64, u64p, C.c_size_t]
        L.txh_index_maps.restype = C.c_int64
        L.txh_index_maps.argtypes = [C.c_void_p, C.c_uint64, u64p, u64p, C.c_size_t]
        L.txh_index_serialise.restype = C.c_void_p
        L.txh_index_serialise.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
        L.txh_index_free.argtypes = [C.c_void_p]
        L._index_ready = True
    return L


class LayoutParams(C.Structure):
    _fields_ = [("tmax", C.c_uint64), ("fpr", C.c_float), ("relaxed_fpr", C.c_float), ("hash_count", C.c_uint),
                ("alpha", C.c_double)]


class BuildOptions(C.Structure):
    _fields_ = [("k", C.c_uint), ("dna", C.c_int), ("reduction", C.c_uint), ("hash_count", C.c_uint), ("fpr", C.c_float),
                ("flavour", C.c_int), ("tmax", C.c_uint64), ("device", C.c_int), ("rearrange_ratio", C.c_double)]


def default_tmax(user_bins):
    """64 * ceil(ceil(sqrt(B)) / 64): the technical bins of one IBF at most, as the uniform builder chooses them."""
    return 64 * ((int(np.ceil(np.sqrt(float(user_bins)))) + 63) // 64)


def union_window(user_bins, tmax):
    """W = min(B, 4 * ceil(B / t_max)): the longest run of user bins one merged bin may take."""
    return min(user_bins, 4 * ((user_bins + tmax - 1) // tmax))


def layout_order(counts):
    """User bins by estimate descending, ties by id (the order of the union table's rows)."""
    counts = np.asarray(counts, dtype=np.float64)
    return np.lexsort((np.arange(counts.size), -counts)).astype(np.uint64)


REARRANGE_MAX_LEN = 4096  # TXH_REARRANGE_MAX_LEN


def rearrange_intervals(counts, ratio=0.5, max_len=None):
    """Intervals of layout_order(counts) inside which `--rearrange` moves bins (include/txh.h txh_rearrange_intervals): the
    first sorted position of every interval, ascending.  max_len: 1 .. 4096 bins per interval at most (None: 4096)."""
    L = lib()
    L.txh_rearrange_intervals.restype = C.c_int64
    L.txh_rearrange_intervals.argtypes = [C.POINTER(C.c_double), C.c_uint64, C.c_double, C.c_uint64, u64p, C.c_size_t]
    c = np.ascontiguousarray(counts, dtype=np.float64)
    if max_len is not None and int(max_len) < 1:
        raise HostError("an interval holds at least one bin")
    starts = np.zeros(max(1, c.size), dtype=np.uint64)
    n = L.txh_rearrange_intervals(c.ctypes.data_as(C.POINTER(C.c_double)), c.size, float(ratio), int(max_len or 0),
                                  starts.ctypes.data_as(u64p), starts.size)
    if n < 0:
        raise _err()
    return starts[:n]


def rearrange_chain(counts, unions):
    """The nearest-neighbour chain inside one interval (include/txh.h txh_rearrange_chain): counts[n] by position in the
    interval, unions (n, n) pairwise union estimates; returns the positions in their new order (position 0 first)."""
    L = lib()
    L.txh_rearrange_chain.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint64, u64p]
    c = np.ascontiguousarray(counts, dtype=np.float64)
    u = np.ascontiguousarray(unions, dtype=np.float64)
    n = c.size
    if u.size != n * n:
        raise HostError("unions must be n x n")
    chain = np.zeros(n, dtype=np.uint64)
    dp = C.POINTER(C.c_double)
    if L.txh_rearrange_chain(c.ctypes.data_as(dp), u.ctypes.data_as(dp), n, chain.ctypes.data_as(u64p)) != 0:
        raise _err()
    return chain


def hibf_layout(counts, unions, tmax=None, fpr=0.05, relaxed_fpr=0.3, hash_count=3, alpha=1.2, order=None):
    """The size-aware HIBF layout (host/layout.hpp, include/txh.h txh_hibf_layout), a pure function.

    counts: each user bin's estimate, by user bin id; unions: B x W union estimates over runs in layout_order(counts)
    (W = union_window(B, tmax)).  order (optional): lay the bins out in this order instead (a permutation of 0 .. B-1;
    unions then over runs of it; txh_hibf_layout_ordered).  Returns dict(order, tmax, window, ibfs=[dict(bins, bin_size,
    next_ibf_id, tb_to_user_bin)]), the root first and the children in depth-first pre-order."""
    L = lib()
    if not hasattr(L, "_layout_ready"):
        L.txh_hibf_layout_ordered.argtypes = [C.POINTER(C.c_double), C.c_uint64, u64p, C.POINTER(C.c_double), C.c_uint64,
                                              C.POINTER(LayoutParams), C.POINTER(C.c_void_p)]
        L.txh_hibf_layout.argtypes = [C.POINTER(C.c_double), C.c_uint64, C.POINTER(C.c_double), C.c_uint64,
                                      C.POINTER(LayoutParams), C.POINTER(C.c_void_p)]
        L.txh_layout_ibf_count.restype = C.c_int64
        L.txh_layout_ibf_count.argtypes = [C.c_void_p]
        L.txh_layout_ibf.restype = C.c_int64
        L.txh_layout_ibf.argtypes = [C.c_void_p, C.c_uint64, u64p, u64p, u64p, C.c_size_t]
        L.txh_layout_order.restype = C.c_int64
        L.txh_layout_order.argtypes = [C.c_void_p, u64p, C.c_size_t]
        L.txh_layout_free.argtypes = [C.c_void_p]
        L._layout_ready = True
    c = np.ascontiguousarray(counts, dtype=np.float64)
    B = c.size
    tmax = int(tmax) if tmax else default_tmax(B)
    u = np.ascontiguousarray(unions, dtype=np.float64).reshape(-1)
    W = u.size // B if B else 0
    p = LayoutParams(tmax, fpr, relaxed_fpr, hash_count, alpha)
    h = C.c_void_p()
    dp = C.POINTER(C.c_double)
    if order is None:
        rc = L.txh_hibf_layout(c.ctypes.data_as(dp), B, u.ctypes.data_as(dp), W, C.byref(p), C.byref(h))
    else:
        o = np.ascontiguousarray(order, dtype=np.uint64)
        if o.size != B:
            raise HostError("the order must be a permutation of the user bins")
        rc = L.txh_hibf_layout_ordered(c.ctypes.data_as(dp), B, o.ctypes.data_as(u64p), u.ctypes.data_as(dp), W, C.byref(p), C.byref(h))
    if rc != 0:
        raise _err()
    try:
        ibfs = []
        for i in range(L.txh_layout_ibf_count(h)):
            n = L.txh_layout_ibf(h, i, None, None, None, 0)
            size = C.c_uint64()
            nxt = np.zeros(n, dtype=np.uint64)
            tbu = np.zeros(n, dtype=np.uint64)
            L.txh_layout_ibf(h, i, C.byref(size), nxt.ctypes.data_as(u64p), tbu.ctypes.data_as(u64p), n)
            ibfs.append(dict(bins=int(n), bin_size=int(size.value), next_ibf_id=nxt, tb_to_user_bin=tbu))
        order = np.zeros(B, dtype=np.uint64)
        L.txh_layout_order(h, order.ctypes.data_as(u64p), B)
    finally:
        L.txh_layout_free(h)
    return dict(order=order, tmax=tmax, window=W, ibfs=ibfs)


class IndexFile:
    """A parsed / constructed TetRex index image (host/index_file.hpp)."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle)

    @classmethod
    def parse(cls, data):
        L = _index_api()
        h = C.c_void_p()
        if L.txh_index_parse(data, len(data), C.byref(h)) != 0:
            raise _err()
        return cls(h.value)

    @classmethod
    def load(cls, path):
        """read_index_file: the file is mapped, its bit matrices are not copied (what `tetrex query` does)."""
        L = _index_api()
        L.txh_index_load.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        h = C.c_void_p()
        if L.txh_index_load(str(path).encode(), C.byref(h)) != 0:
            raise _err()
        return cls(h.value)

    @classmethod
    def build(cls, paths, k=6, dna=False, reduction=0, layout="sized", tmax=None, fpr=0.05, hash_count=3, device=0, rearrange=None):
        """`tetrex index` without the CLI (txh_index_build of libtetrex_query.so; needs a GPU): layout "sized" (the
        size-aware HIBF), "uniform" (the default HIBF of the CLI) or "ibf" (a flat IBF, -i).  rearrange (sized only):
        None / 0 off, True the default ratio 0.5, or the interval ratio in (0, 1] (`--rearrange [--rearrange-ratio R]`)."""
        from tetrex_amd import capi
        flavours = {"uniform": 0, "sized": 1, "ibf": 2}
        if layout not in flavours:
            raise ValueError("layout must be one of %s" % sorted(flavours))
        Q = capi._query_lib()
        Q.txh_index_build.argtypes = [C.POINTER(C.c_char_p), C.c_size_t, C.POINTER(BuildOptions), C.POINTER(C.c_void_p)]
        arr = (C.c_char_p * len(paths))(*[str(p).encode() for p in paths])
        ratio = 0.5 if rearrange is True else float(rearrange or 0)
        opt = BuildOptions(k, int(dna), reduction, hash_count, fpr, flavours[layout], int(tmax or 0), device, ratio)
        _index_api()  # the handle is freed through libtetrex_host.so
        h = C.c_void_p()
        if Q.txh_index_build(arr, len(paths), C.byref(opt), C.byref(h)) != 0:
            raise HostError(Q.txe_last_error().decode(errors="replace"))
        return cls(h.value)

    @classmethod
    def from_ibf(cls, k, dna, reduction, hash_count, bins, bin_size, words, paths):
        L = _index_api()
        w = np.ascontiguousarray(words, dtype=np.uint64)
        h = C.c_void_p()
        if L.txh_index_from_ibf(k, int(dna), reduction, hash_count, bins, bin_size, w.ctypes.data_as(u64p),
                                "\n".join(paths).encode(), C.byref(h)) != 0:
            raise _err()
        return cls(h.value)

    def describe(self):
        import json
        buf = C.create_string_buffer(1 << 22)
        if _index_api().txh_index_describe(self._h, buf, len(buf)) < 0:
            raise _err()
        return json.loads(buf.value.decode())

    def words(self, ibf_id=0):
        L = _index_api()
        n = L.txh_index_words(self._h, ibf_id, None, 0)
        if n < 0:
            raise _err()
        out = np.zeros(n, dtype=np.uint64)
        L.txh_index_words(self._h, ibf_id, out.ctypes.data_as(u64p), n)
        return out

    def maps(self, ibf_id):
        L = _index_api()
        a = np.zeros(1 << 20, dtype=np.uint64)
        b = np.zeros(1 << 20, dtype=np.uint64)
        n = L.txh_index_maps(self._h, ibf_id, a.ctypes.data_as(u64p), b.ctypes.data_as(u64p), a.size)
        if n < 0:
            raise _err()
        return a[:n].copy(), b[:n].copy()

    def serialise(self):
        size = C.c_size_t()
        p = _index_api().txh_index_serialise(self._h, C.byref(size))
        if not p:
            raise _err()
        return C.string_at(p, size.value)

    def save(self, path):
        with open(path, "wb") as f:
            f.write(self.serialise())

    def __del__(self):
        try:
            if self._h:
                _index_api().txh_index_free(self._h)
                self._h = None
        except Exception:
            pass
