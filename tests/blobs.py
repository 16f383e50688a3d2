"""Hand-built program blobs of versions 2 and 4 (include/txq_program.h) and a generator of well-formed multi-stage
sessions: what a producer other than the C++ frontier compiler may hand to libtxq.so.  The GPU tests put the device beside
helpers.SessionSimulator on these sessions (tests/test_gpu_exec_blobs.py); the CPU tests check the writer against the host
parsers and the generator against the simulator's own well-formedness assertions (tests/test_blobs.py)."""
import struct

import numpy as np

NO_KMER = 0xFFFFFFFF
DENSE_OP = 0xFFFFFFFE
DENSE_BIT = 0x40000000
BLOCK_SHIFT = 22
INDEX_MASK = 0x3FFFFF
TRACKED_BIT = 0x80000000
ZERO, STEP, REDUCE, FILL = 0, 1, 2, 3
TRACKED, NOPROBE = 1, 2
MAGIC = 0x50515854
HEADER_V2, HEADER_V4 = 64, 96
# byte offsets of header fields (txq_blob_header_v2 / _v3), for tests that damage one field
FIELD = dict(magic=0, version=4, n_programs=8, n_kmers=12, n_ops=16, n_levels=20, kmers_offset=24, programs_offset=32, ops_offset=40,
             levels_offset=48, n_aux_kmers=56, dense_offset=64, n_dense=72, k=76, bits=80, alphabet=84, canonical=88)


def dense_slot(block, index=0):
    """slot id of entry `index` of dense block `block`"""
    return DENSE_BIT | (block << BLOCK_SHIFT) | index


def codes_of(mask):
    return [c for c in range(32) if (mask >> c) & 1]


def mask_of(codes):
    m = 0
    for c in codes:
        m |= 1 << int(c)
    return m


def entry_index(geometry, codes):
    """Mixed-radix number of a suffix inside a geometry: geometry = per position (oldest first) the mask of codes that occur
    there, codes = the suffix.  The full geometry [(1 << A) - 1] * (k - 1) gives sum code_j * A^(k-2-j)."""
    idx = 0
    for g, c in zip(geometry, codes):
        cs = codes_of(g)
        idx = idx * len(cs) + cs.index(int(c))
    return idx


def dense_row(kind, dst, src=0, r_mask=0, shape=(), reserved=0):
    """one txq_dense_op as 16 words"""
    shape = [int(x) for x in shape]
    assert len(shape) <= 11
    return [kind, dst, src, r_mask] + shape + [0] * (11 - len(shape)) + [reserved]


def _pad8(out):
    while len(out) % 8:
        out += b"\0"


def write_blob(kmers, programs, dense=None, params=None, n_aux_kmers=0):
    """Serialise a version-2 blob (params is None) or a version-4 blob.
    programs: [(n_slots, n_blocks, tracked, levels)], levels = [[(kmer, dst, a, b), ...], ...]; levels None with a fifth
    element `ops` = a program without a level table (n_levels == 0: executed in op order).
    dense: [dense_row(...)], params: dict(k, bits, alphabet, canonical).
    Layout: header | kmers | programs | ops | levels | dense table, every table 8-byte aligned; the level table holds END
    indices relative to the program's first op."""
    kmers = np.ascontiguousarray(kmers, dtype="<u8")
    v4 = params is not None
    prog_rows, all_ops, all_levels = [], [], []
    for prog in programs:
        n_slots, n_blocks, tracked, levels = prog[:4]
        first_op, first_level = len(all_ops), len(all_levels)
        if levels is None:
            all_ops.extend(prog[4])
            n_ops, n_lv = len(prog[4]), 0
        else:
            n_ops = 0
            for lv in levels:
                all_ops.extend(lv)
                n_ops += len(lv)
                all_levels.append(n_ops)
            n_lv = len(levels)
        prog_rows.append((first_op, n_ops, n_slots, first_level, n_lv, (n_blocks | (TRACKED_BIT if tracked else 0)) if v4 else 0))
    dense = dense or []
    out = bytearray(HEADER_V4 if v4 else HEADER_V2)
    k_off = len(out)
    out += kmers.tobytes()
    _pad8(out)
    p_off = len(out)
    out += np.array(prog_rows, dtype="<u4").reshape(len(prog_rows), 6).tobytes()
    _pad8(out)
    o_off = len(out)
    out += np.array(all_ops, dtype=np.uint64).astype("<u4").reshape(len(all_ops), 4).tobytes()
    _pad8(out)
    l_off = len(out)
    out += np.array(all_levels, dtype="<u4").tobytes()
    _pad8(out)
    struct.pack_into("<6I5Q", out, 0, MAGIC, 4 if v4 else 2, len(programs), kmers.size, len(all_ops), len(all_levels),
                     k_off, p_off, o_off, l_off, n_aux_kmers)
    if v4:
        d_off = len(out)
        out += np.array(dense, dtype=np.uint64).astype("<u4").reshape(len(dense), 16).tobytes()
        struct.pack_into("<Q6I", out, HEADER_V2, d_off, len(dense), params["k"], params["bits"], params["alphabet"], params["canonical"], 0)
    return bytes(out)


def patch_u32(blob, offset, value):
    out = bytearray(blob)
    struct.pack_into("<I", out, offset, value & 0xFFFFFFFF)
    return bytes(out)


def patch_u64(blob, offset, value):
    out = bytearray(blob)
    struct.pack_into("<Q", out, offset, value)
    return bytes(out)


# ---- the generator -----------------------------------------------------------------------------------------------------
N_STAGES = 4


class _Prog:
    """One logical program while it is generated: its levels per stage, the slots and blocks it has claimed so far (what its
    table row says from that stage on: both only grow), and what can be observed of it at the end."""

    def __init__(self, tracked=False, kind="empty"):
        self.tracked, self.kind = tracked, kind
        self.levels = [[] for _ in range(N_STAGES)]   # per stage: [[op, ...], ...]; a dense op is ("D", dense_row)
        self.n_slots, self.n_blocks = 3, 0
        self.slots_at, self.blocks_at = [3] * N_STAGES, [0] * N_STAGES
        self.defined = []      # ordinary slots that hold a value (written at some point), in the order they were first written
        self.entries = []      # dense slot ids of block entries that are defined at the end
        self.must = []         # ... those the first twins observe: entries whose value depends on every predecessor of a step
        self.ask = [[] for _ in range(N_STAGES)]      # per stage: ordinary slots worth a feedback query after it

    def close_stage(self, st):
        for s in range(st, N_STAGES):
            self.slots_at[s], self.blocks_at[s] = self.n_slots, self.n_blocks

    def new_slot(self):
        self.n_slots += 1
        return self.n_slots - 1

    def wrote(self, *slots):
        for s in slots:
            if s >= 3 and not (s & DENSE_BIT) and s not in self.defined:
                self.defined.append(s)

    def has_ops(self, st):
        return any(len(lv) for lv in self.levels[st])


class _Ctx:
    def __init__(self, rng, spec):
        self.rng, self.spec = rng, spec
        self.nk = spec["n_kmers"] + spec.get("n_aux_kmers", 0)  # every stage's table: n_kmers main values, then the auxiliary ones

    def km(self, p_none=0.25):
        """a k-mer operand: an index into the whole table (both halves), or TXQ_NO_KMER"""
        return NO_KMER if self.rng.random() < p_none else int(self.rng.integers(0, self.nk))

    def pick(self, seq):
        return seq[int(self.rng.integers(0, len(seq)))]

    def subset(self, mask, lo=1, proper=False, most=32):
        """random subset of the codes of `mask` with at least `lo` and at most `most` of them (proper: not all of them, where
        it has two or more)"""
        cs = codes_of(mask)
        hi = min(most, len(cs) - (1 if proper and len(cs) > 1 else 0))
        n = int(self.rng.integers(min(lo, hi), hi + 1))
        return mask_of(self.rng.choice(cs, size=n, replace=False))


def _level_of_writes(c, P, readable, n, pool):
    """n independent writes: operands from `readable`, destinations distinct and outside what the level reads"""
    pairs = [(c.pick(readable), c.pick(readable + [0])) for _ in range(n)]
    reads = {s for ab in pairs for s in ab}
    free = [s for s in pool if s not in reads]
    c.rng.shuffle(free)
    lv = [(c.km(), d, a, b) for (a, b), d in zip(pairs, free)]
    return lv


def _small(c, first=0):
    """ordinary small program: levels of independent writes on a region that grows from stage to stage; some stages without
    an op; slots written in stage i read in stage i + 2"""
    P = _Prog(kind='small')
    readable = [1]
    skip = int(c.rng.integers(first + 1, N_STAGES)) if c.rng.random() < 0.6 else -1
    for st in range(first, N_STAGES):
        if st == skip:
            continue
        P.n_slots += int(c.rng.integers(2, 10))
        for _ in range(int(c.rng.integers(1, 6))):
            lv = _level_of_writes(c, P, readable, int(c.rng.integers(1, 10)), list(range(2, P.n_slots)))
            P.levels[st].append(lv)
            for op in lv:
                P.wrote(op[1])
                if op[1] >= 3 and op[1] not in readable:
                    readable.append(op[1])
        src = c.pick(readable)
        P.levels[st].append([(NO_KMER, 2, 2, src) if c.rng.random() < 0.5 else (NO_KMER, 2, src, 2)])
        z = P.new_slot()
        P.levels[st].append([(c.km(0.0), z, 0, 0)])  # a slot that is all zero
        P.wrote(z)
        P.ask[st] = [c.pick(readable), z, 2]
        P.close_stage(st)
    return P


def _fan_in(c, n_acc):
    """a level of independent writes, then a level that is ONLY accumulations: n_acc ops onto RESULT and onto one more
    slot, `dst |= x` written both as dst == a and as dst == b"""
    P = _Prog(kind='fan-in')
    n_src = 24
    srcs = [P.new_slot() for _ in range(n_src)]
    t = P.new_slot()
    P.levels[0].append([(c.km(0.0), s, 1, 0) for s in srcs] + [(NO_KMER, t, 0, 0)])
    P.wrote(*srcs, t)
    for st, target in ((0, 2), (1, t), (3, 2)):
        lv = []
        for i in range(n_acc):
            x = srcs[int(c.rng.integers(0, n_src))]
            lv.append((NO_KMER, target, target, x) if i % 2 else (NO_KMER, target, x, target))
        other = t if target == 2 else 2  # and a few onto the other target, in the same level
        lv += [(NO_KMER, other, other, c.pick(srcs)) for _ in range(7)]
        c.rng.shuffle(lv)
        P.levels[st].append([tuple(int(v) for v in op) for op in lv])
        P.ask[st] = [t, srcs[0]]
        P.close_stage(st)
    return P


def _chain(c, depth=30):
    """a chain `depth` levels deep, one or two ops a level"""
    P = _Prog(kind='chain')
    a, b = P.new_slot(), P.new_slot()
    P.levels[0].append([(c.km(0.0), a, 1, 0), (NO_KMER, b, 0, 0)])
    P.wrote(a, b)
    for l in range(depth):
        n = P.new_slot() if l % 7 == 0 else (a if l % 2 else b)
        src = a if n != a else b
        # alternately AND with a k-mer and OR the other strand in, so that the chain stays alive
        lv = [(c.km(0.3) if l % 3 == 0 else NO_KMER, n, src, a if l % 3 else 0)]
        if l % 5 == 0:
            lv.append((NO_KMER, 2, 2, src))
        P.levels[0].append(lv)
        P.wrote(n)
        if l % 2:
            a = n
        else:
            b = n
    P.levels[0].append([(NO_KMER, 2, a, b)])
    P.ask[0] = [a, b]
    P.close_stage(0)
    P.levels[2].append([(c.km(), 2, a, 2)])
    P.close_stage(2)
    return P


def _big(c, n_ops, depth):
    """a big program without dense ops (n_ops * W reaches the unit path): `depth` levels of independent writes between two
    banks of slots, then accumulations of up to 500 ops a slot onto RESULT and further slots; continued two stages later"""
    P = _Prog(kind='big')
    width = max(4, -(-n_ops // depth))
    bank = [[P.new_slot() for _ in range(width)] for _ in range(2)]
    st = 1
    P.levels[st].append([(c.km(0.0), s, 1, 0) for s in bank[0]])
    for l in range(1, depth):
        src, dst = bank[(l + 1) % 2], bank[l % 2]
        perm = c.rng.permutation(width)
        lv = []
        for i in range(width):
            keep = l % 3 == 0  # every third level ANDs, the others OR a neighbour in: masks stay alive over the whole depth
            lv.append((c.km(0.0) if keep else NO_KMER, dst[i], src[i], 0 if keep else src[int(perm[i])]))
        P.levels[st].append(lv)
    P.wrote(*bank[0], *bank[1])
    last = bank[(depth - 1) % 2]
    targets = [2] + [P.new_slot() for _ in range(max(0, -(-width // 500) - 1))]
    P.levels[st].append([(NO_KMER, t, 0, 0) for t in targets[1:]] or [(NO_KMER, 2, 2, 0)])
    lv = []
    for i, s in enumerate(last):
        t = targets[i // 500]
        lv.append((NO_KMER, t, t, s) if i % 2 else (NO_KMER, t, s, t))
    P.levels[st].append(lv)
    P.wrote(*targets[1:])
    P.ask[st] = [last[0], targets[-1]]
    P.close_stage(st)
    P.levels[3].append([(c.km(), bank[0][i], last[i], bank[0][i]) for i in range(min(width, 16))] if depth % 2 == 0 else
                       [(c.km(), bank[1][i], last[i], bank[1][i]) for i in range(min(width, 16))])
    P.levels[3].append([(NO_KMER, 2, 2, bank[depth % 2][0])])
    P.close_stage(3)
    return P


def _dense_untracked(c):
    """A program with untracked blocks: full and shaped ZERO, FILL over a product shape, STEPs with full shapes, with proper
    subsets at every position, with a single residue and with an empty shape[0], REDUCE into an ordinary slot, into RESULT
    and into a block entry, ordinary ops that scatter into a block and copy out of one.  Blocks grow from 3 to 6."""
    par = c.spec["dense"]
    A, pos = par["alphabet"], par["k"] - 1
    full = (1 << A) - 1
    FULL = [full] * pos
    P = _Prog(kind='untracked')
    D = lambda *a, **k: ("D", dense_row(*a, **k))
    rnd_entry = lambda geom: dense_slot(0, entry_index(geom, [c.pick(codes_of(g)) for g in geom]))
    ent = lambda b, geom: (b << BLOCK_SHIFT) | rnd_entry(geom)
    b0, b1, b2, b3, b4, b5 = (dense_slot(b) for b in range(6))
    s3, s4, s5, s6, s7 = (P.new_slot() for _ in range(5))
    # stage 0
    P.n_blocks = 3
    L = P.levels[0]
    L.append([D(ZERO, b0), D(ZERO, b2), (c.km(0.0), s3, 1, 0), (c.km(0.0), s4, 1, 0), (c.km(0.0), s5, 1, 0)])
    S1 = [c.subset(full, lo=2, proper=True) for _ in range(pos)]
    # (one of the scattered states has the LAST code at the oldest position: the full step's last predecessor matters)
    mid = [c.pick(codes_of(full)) for _ in range(pos - 1)]
    last = dense_slot(0, entry_index(FULL, [A - 1] + mid))
    scatter = sorted({ent(0, FULL) for _ in range(8)} - {last})
    lv = [D(ZERO, b1, r_mask=1, shape=S1), (NO_KMER, last, s3, 0)]
    P.must.append(dense_slot(2, entry_index(FULL, mid + [c.pick(codes_of(full))])))
    for i, e in enumerate(scatter):
        lv.append((c.km(), e, s3, s4) if i % 2 else (NO_KMER, e, e, s5))  # plain writes and accumulations into entries
    L.append(lv)
    F = [c.subset(g, lo=1) for g in S1]
    L.append([D(FILL, b1, src=s3, shape=F), (c.km(), s6, scatter[0], s4)])
    L.append([D(STEP, b2, src=b0, r_mask=full, shape=FULL), (c.km(), s7, s6, 0)])
    R2 = [c.subset(full, lo=1, proper=True) for _ in range(pos)]
    L.append([D(REDUCE, s6, src=b2, shape=FULL), D(REDUCE, 2, src=b2, shape=R2), D(REDUCE, 2, src=b0, shape=FULL), (NO_KMER, 2, 2, s7)])
    P.wrote(s3, s4, s5, s6, s7)
    P.ask[0] = [s6, s7, 2]
    P.close_stage(0)
    # stage 1: two more blocks
    P.n_blocks = 5
    s8, s9 = P.new_slot(), P.new_slot()
    L = P.levels[1]
    # inside what the FILL spread over b1: proper subsets of the alphabet at every position; at most three predecessors, so that
    # a destination entry is no saturated OR in which one predecessor more or less changes no bit
    sub = [c.subset(g, lo=1, most=3 if j == 0 else 32) for j, g in enumerate(F)]
    one = [c.subset(g, lo=1, most=3 if j == 0 else 32) for j, g in enumerate(F)]
    r_sub = c.subset(full, lo=2, proper=True)
    r_one = 1 << c.pick(codes_of(full))
    S4 = [c.subset(full, lo=1) | m for m in one[1:]] + [r_one | c.subset(full, lo=1, proper=True)]
    L.append([D(ZERO, b3), D(ZERO, b4, r_mask=1, shape=S4), (c.km(0.0), s8, s4, 0)])
    L.append([D(STEP, b3, src=b1, r_mask=r_sub, shape=sub)])
    P.must.append(dense_slot(3, entry_index(FULL, [c.pick(codes_of(m)) for m in sub[1:]] + [c.pick(codes_of(r_sub))])))
    P.must.append(dense_slot(4, entry_index(FULL, [c.pick(codes_of(m)) for m in one[1:]] + codes_of(r_one))))
    L.append([D(STEP, b4, src=b1, r_mask=r_one, shape=one), D(STEP, b3, src=b0, r_mask=full, shape=[0] + FULL[1:]),
              (c.km(), s9, s8, s5)])
    e0 = ent(0, FULL)
    L.append([D(REDUCE, e0, src=b3, shape=FULL), D(REDUCE, s8, src=b4, shape=[c.subset(g, lo=1) for g in S4])])
    L.append([(c.km(), s9, ent(3, FULL), e0)])
    L.append([(NO_KMER, 2, s9, 2)])
    P.wrote(s8, s9)
    P.ask[1] = [s8, s9]
    P.close_stage(1)
    # stage 2: what stage 0 left in its slots and blocks is read again
    s10 = P.new_slot()
    P.levels[2].append([(c.km(), s10, s6, ent(2, FULL))])
    P.wrote(s10)
    P.ask[2] = [s10]
    P.close_stage(2)
    # stage 3: blocks of stage 1 are stepped on
    P.n_blocks = 6
    L = P.levels[3]
    L.append([D(ZERO, b5)])
    L.append([D(STEP, b5, src=b3, r_mask=c.subset(full, lo=1), shape=FULL)])
    L.append([D(REDUCE, 2, src=b5, shape=FULL), D(REDUCE, s10, src=b4, shape=S4)])
    P.close_stage(3)
    N = A ** pos
    P.entries = [dense_slot(b, i) for b in (0, 2, 3, 5) for i in c.rng.choice(N, size=min(N, 6), replace=False)]
    P.entries += [dense_slot(1, entry_index(FULL, [c.pick(codes_of(g)) for g in S1])) for _ in range(4)]
    P.entries += [dense_slot(4, entry_index(FULL, [c.pick(codes_of(g)) for g in S4])) for _ in range(4)]
    return P


def _geometry(c, A, pos, must=None, limit=400, most=32):
    """random geometry (per position a non-empty set of at most `most` codes, plus must[j]) of at most `limit` entries"""
    full = (1 << A) - 1
    while True:
        g = [c.subset(full, lo=1, most=most) | (must[j] if must else 0) for j in range(pos)]
        n = int(np.prod([bin(m).count("1") for m in g]))
        if n <= limit:
            return g, n
        if must and int(np.prod([bin(m).count("1") for m in must])) > limit:
            raise AssertionError("no geometry fits")


def _dense_tracked(c):
    """A tracked program: ZEROs with a capacity equal to and above the geometry's product, a block id ZEROed again with another
    geometry and the same capacity, FILL and STEP between blocks of different geometries, NOPROBE steps, REDUCE, ordinary ops
    on entries, a block that stays empty (steps and reduces over an empty live list)."""
    par = c.spec["dense"]
    A, pos = par["alphabet"], par["k"] - 1
    full = (1 << A) - 1
    P = _Prog(tracked=True, kind='tracked')
    T = TRACKED
    D = lambda *a, **k: ("D", dense_row(*a, **k))
    b = [dense_slot(i) for i in range(6)]
    geo = {}   # block -> geometry at the end
    in_geo = lambda blk: dense_slot(blk, entry_index(geo[blk], [c.pick(codes_of(g)) for g in geo[blk]]))
    small = 400 if A ** pos <= 400 else 120
    few = 4 if pos > 1 else 12  # codes per position of the first blocks: what follows them holds these and more, within 400 entries

    def follow(*srcs, r, limit=400):
        """a geometry that takes the steps from the blocks `srcs` with residues r: position j holds what they hold at j + 1"""
        must = [0] * pos
        for s in srcs:
            for j in range(pos - 1):
                must[j] |= geo[s][j + 1]
        must[pos - 1] |= r
        return _geometry(c, A, pos, must=must, limit=limit)

    s3, s4, s5, s6 = (P.new_slot() for _ in range(4))
    # stage 0
    P.n_blocks = 4
    geo[0], n0 = _geometry(c, A, pos, limit=small, most=few)
    geo[2], n2 = _geometry(c, A, pos, limit=small, most=few)
    r01 = c.subset(full, lo=1, most=few)
    geo[1], n1 = follow(0, r=r01, limit=360)
    cap1 = n1 + int(c.rng.integers(1, 40))  # a capacity above the geometry
    r13, r23 = c.subset(full, lo=1), c.subset(full, lo=1)
    geo[3], n3 = follow(1, 2, r=r13 | r23)
    L = P.levels[0]
    L.append([D(ZERO, b[0], src=n0, shape=geo[0], reserved=T), D(ZERO, b[1], src=cap1, shape=geo[1], reserved=T),
              D(ZERO, b[2], src=n2, shape=geo[2], reserved=T), D(ZERO, b[3], src=n3, shape=geo[3], reserved=T),
              (c.km(0.0), s3, 1, 0), (c.km(0.0), s4, 1, 0), (NO_KMER, s5, 0, 0)])
    ents1 = sorted({in_geo(1) for _ in range(5)})
    lv = [D(FILL, b[0], src=s3, shape=geo[0][:1] + [c.subset(g, lo=1) for g in geo[0][1:]], reserved=T)]
    for i, e in enumerate(ents1):
        lv.append((c.km(), e, s3, s4) if i % 2 else (NO_KMER, e, e, s4))
    L.append(lv)
    L.append([D(STEP, b[1], src=b[0], r_mask=r01, shape=geo[0], reserved=T | NOPROBE),
              D(STEP, b[3], src=b[2], r_mask=r23, shape=geo[2], reserved=T), (c.km(), s6, s3, s5)])
    L.append([D(STEP, b[3], src=b[1], r_mask=r13, shape=geo[1], reserved=T)])
    L.append([D(REDUCE, 2, src=b[3], shape=geo[3], reserved=T), D(REDUCE, s4, src=b[2], shape=geo[2], reserved=T),
              D(REDUCE, s4, src=b[1], shape=geo[1], reserved=T), (c.km(), s6, in_geo(3), s5)])
    P.wrote(s3, s4, s5, s6)
    P.ask[0] = [s4, s5, s6]
    P.close_stage(0)
    # stage 1: block 1 again, with another geometry inside the same capacity; one more block
    P.n_blocks = 5
    s7 = P.new_slot()
    geo[1], n1b = _geometry(c, A, pos, limit=cap1)
    geo[1][0] = c.subset(geo[1][0], lo=1, most=3)  # (few predecessors per destination entry: each of them shows in the OR)
    r34, r14 = c.subset(full, lo=1), c.subset(full, lo=1)
    geo[4], n4 = follow(3, 1, r=r34 | r14)
    L = P.levels[1]
    L.append([D(ZERO, b[1], src=cap1, shape=geo[1], reserved=T), D(ZERO, b[4], src=n4, shape=geo[4], reserved=T), (c.km(0.0), s7, s4, 0)])
    e4 = in_geo(4)
    # (the FILL covers every code of the oldest position: each destination entry of the probed step out of block 1 is an OR
    # over all of them, the last one included)
    fill1 = geo[1][:1] + [c.subset(g, lo=1) for g in geo[1][1:]]
    L.append([D(FILL, b[1], src=s4, shape=fill1, reserved=T), (c.km(), e4, s3, s7)])
    L.append([D(STEP, b[4], src=b[3], r_mask=r34, shape=geo[3], reserved=T | (NOPROBE if c.rng.random() < 0.5 else 0))])
    L.append([D(STEP, b[4], src=b[1], r_mask=r14, shape=geo[1], reserved=T)])
    P.must.append(dense_slot(4, entry_index(geo[4], [c.pick(codes_of(m)) for m in fill1[1:]] + [c.pick(codes_of(r14))])))
    L.append([D(REDUCE, 2, src=b[4], shape=geo[4], reserved=T), D(REDUCE, s7, src=b[4], shape=geo[4], reserved=T)])
    P.wrote(s7)
    P.ask[1] = [s7, 2]
    P.close_stage(1)
    # stage 3: blocks and slots of stage 1 are read
    s8 = P.new_slot()
    L = P.levels[3]
    L.append([(c.km(), s8, s7, in_geo(4))])
    L.append([D(REDUCE, s8, src=b[4], shape=geo[4], reserved=T), D(REDUCE, s8, src=b[2], shape=geo[2], reserved=T), (NO_KMER, 2, 2, in_geo(3))])
    P.wrote(s8)
    P.ask[3] = [s8]
    P.close_stage(3)
    P.entries = [in_geo(blk) for blk in (0, 1, 3, 3, 4, 4, 2) for _ in range(2)]
    return P


def _tiny_tracked(c):
    """a tracked program of one stage with eight tiny blocks: hundreds of these put more dense ops into one level than one
    launch of the sparse kernels takes (kMaxSparseGroups = 1024 in txq_exec.hip)"""
    par = c.spec["dense"]
    A, pos = par["alphabet"], par["k"] - 1
    full = (1 << A) - 1
    P = _Prog(tracked=True, kind="tiny tracked")
    D = lambda *a, **k: ("D", dense_row(*a, reserved=TRACKED, **k))
    s3 = P.new_slot()
    P.n_blocks = 8
    geo, size, res = {}, {}, {}
    for i in range(4):
        geo[i], size[i] = _geometry(c, A, pos, most=2)
        res[i] = c.subset(full, lo=1, most=2)
        must = [geo[i][j + 1] for j in range(pos - 1)] + [res[i]]
        geo[4 + i], size[4 + i] = _geometry(c, A, pos, must=must, most=1)
    L = P.levels[0]
    L.append([D(ZERO, dense_slot(i), src=size[i], shape=geo[i]) for i in range(8)] + [(c.km(0.0), s3, 1, 0)])
    L.append([D(FILL, dense_slot(i), src=s3, shape=geo[i]) for i in range(4)])
    L.append([D(STEP, dense_slot(4 + i), src=dense_slot(i), r_mask=res[i], shape=geo[i]) for i in range(4)])
    L.append([D(REDUCE, 2, src=dense_slot(4 + i), shape=geo[4 + i]) for i in range(4)])
    P.wrote(s3)
    P.ask[0] = [s3]
    P.close_stage(0)
    return P


def random_session(rng, spec, meta=None):
    """A well-formed session of N_STAGES stages: [(blob, query_program, query_slot)].
    spec: dict(W = mask words (sizes the big programs), n_kmers = main k-mers per stage, kmer_pool = values to draw them from,
    n_aux_kmers, aux_pool, dense = None or dict(k, bits, alphabet, canonical), dense_mode = "both" | "untracked" | "tracked",
    twins = T, scale = how many of the small kinds; fan_in = accumulations per fan-in program, big = (ops above the unit
    threshold, levels) per big program: smaller sessions for fixtures).  Program ids: logical program i, copy t is program sum(T) ... in order;
    the T copies of a logical program are consecutive programs.  meta: a list that receives, per program, (kind of its logical
    program, number of the logical program, the slot its last level copies into RESULT or None) — for messages."""
    c = _Ctx(rng, spec)
    W, T, scale = spec["W"], spec.get("twins", 4), spec.get("scale", 1)
    logical = []
    if spec.get("many"):  # hundreds of tiny tracked programs, one copy each, and two ordinary ones
        T = 1
        logical = [_tiny_tracked(c) for _ in range(spec["many"])] + [_fan_in(c, 137), _small(c)]
    else:
        for _ in range(5 * scale):
            logical.append(_small(c))
        for n_acc in spec.get("fan_in", (500, 137)):
            logical.append(_fan_in(c, n_acc))
        logical.append(_chain(c, 30))
        logical.append(_Prog())  # no op at all: result zero
        need = -(-32768 // W)
        for extra, depth in spec.get("big", ((8, 32), (300, 5))):
            logical.append(_big(c, need + extra, depth))
        logical.append(_small(c, first=2))  # its first op comes in stage 2
        if spec.get("dense"):
            mode = spec.get("dense_mode", "both")
            for _ in range(2):
                if mode in ("both", "untracked"):
                    logical.append(_dense_untracked(c))
                if mode in ("both", "tracked"):
                    logical.append(_dense_tracked(c))
        logical.append(_Prog())
    # observation twins: copy t of a program ends with RESULT = one of its slots or defined block entries
    programs = []  # (logical program, observed slot or None)
    for P in logical:
        programs.append((P, None))
        cand = list(P.defined[-12:]) + list(P.entries)
        half = [s for s in P.entries]
        for t in range(1, T):
            if not cand:
                programs.append((P, None))
                continue
            pool = half if (t % 2 and half) else cand
            programs.append((P, int(P.must[t - 1] if t <= len(P.must) else pool[int(rng.integers(0, len(pool)))])))
    if meta is not None:
        index_of = {id(P): i for i, P in enumerate(logical)}
        meta.extend((P.kind, index_of[id(P)], obs) for P, obs in programs)
    stages = []
    ran = [False] * len(programs)
    for st in range(N_STAGES):
        table, dense = [], []
        for pi, (P, obs) in enumerate(programs):
            levels = []
            for lv in P.levels[st]:
                out = []
                for op in lv:
                    if op[0] == "D":
                        out.append((DENSE_OP, len(dense), 0, 0))
                        dense.append(op[1])
                    else:
                        out.append(op)
                levels.append(out)
            last = max([s for s in range(N_STAGES) if P.has_ops(s)], default=-1)
            if obs is not None and st == last:
                levels.append([(NO_KMER, 2, obs, 0)])
            ran[pi] = ran[pi] or any(len(lv) for lv in levels)
            table.append((P.slots_at[st], P.blocks_at[st], P.tracked, levels))
        kmers = rng.choice(spec["kmer_pool"], size=spec["n_kmers"], replace=False).astype(np.uint64)
        n_aux = spec.get("n_aux_kmers", 0)
        if n_aux:
            kmers = np.concatenate([kmers, rng.choice(spec["aux_pool"], size=n_aux, replace=False).astype(np.uint64)])
        blob = write_blob(kmers, table, dense=dense, params=spec.get("dense"), n_aux_kmers=n_aux)
        qp, qs = [], []
        for pi, (P, obs) in enumerate(programs):
            if not ran[pi]:
                continue  # (a program is asked about once it has run an op)
            for s in P.ask[st] + ([0] if pi % 3 == 0 else []):
                qp.append(pi)
                qs.append(s)
        stages.append((blob, np.array(qp, dtype=np.uint32), np.array(qs, dtype=np.uint32)))
    return stages


def check_kinds(sim, spec):
    """What a session must have contained, by the simulator's counters (a session that lacks a kind is a generator bug)."""
    if not spec.get("dense"):
        return
    mode = spec.get("dense_mode", "both")
    assert all(n > 0 for n in sim.dense_kinds), sim.dense_kinds
    assert sim.dense_steps > 0
    if mode in ("both", "tracked"):
        assert sim.tracked_ops > 0 and sim.noprobe_steps > 0 and len(sim.block_entries) > 0
    else:
        assert sim.tracked_ops == 0


# ---- the cells: an index (the same in the oracle and as upload descriptors) and the spec of its session -------------------
PEPTIDE3 = dict(k=3, bits=5, alphabet=20, canonical=0)
DNA4 = dict(k=4, bits=2, alphabet=4, canonical=1)
REDUCED3 = dict(k=3, bits=5, alphabet=10, canonical=0)
PEPTIDE2 = dict(k=2, bits=5, alphabet=20, canonical=0)

# flat IBFs of about 2000 rows: bins -> hash count (W = ceil(bins / 64) walks over the executor's width thresholds)
FLAT = {5: 1, 128: 2, 130: 3, 2048: 4, 2112: 5, 2176: 2, 9000: 3}
CELLS = {"flat-%d" % b: dict(index="flat", bins=b, h=h, dense=PEPTIDE3, mode="both", seed=100 + b) for b, h in FLAT.items()}
for _name, _par in (("peptide3", PEPTIDE3), ("dna4", DNA4), ("reduced3", REDUCED3), ("peptide2", PEPTIDE2)):
    for _mode in ("untracked", "tracked"):
        CELLS["%s-%s" % (_name, _mode)] = dict(index="flat", bins=300, h=2, dense=_par, mode=_mode, seed=len(CELLS))
CELLS["aux"] = dict(index="flat", bins=300, h=3, dense=PEPTIDE3, mode="both", aux=True, seed=31)
for _shape in ("16x64", "8x256-mixed", "4x64"):
    for _mode in ("untracked", "tracked"):
        CELLS["tree-%s-%s" % (_shape, _mode)] = dict(index="regular", shape=_shape, dense=PEPTIDE3, mode=_mode, seed=40 + len(CELLS))
CELLS["many-tracked"] = dict(index="flat", bins=130, h=2, dense=PEPTIDE3, mode="tracked", many=280, seed=71)
for _mode in ("untracked", "tracked"):
    CELLS["layout-%s" % _mode] = dict(index="layout", dense=PEPTIDE3, mode=_mode, seed=60 + len(CELLS))


def valid_kmers(par):
    """every packed k-mer value over the alphabet (bits per residue, first residue highest)"""
    v = np.zeros(1, dtype=np.uint64)
    for _ in range(par["k"]):
        v = ((v[:, None] << np.uint64(par["bits"])) | np.arange(par["alphabet"], dtype=np.uint64)[None, :]).reshape(-1)
    return v


def build_cell(O, name):
    """dict(ox = oracle index, upload = ("ibf", bins, rows, h, words) | ("hibf", user_bins, descs), spec, seed, and for the
    cell with auxiliary k-mers: dg = the oracle's second flat IBF, aux_upload)"""
    import helpers
    cell = CELLS[name]
    rng = np.random.default_rng(cell["seed"])
    par = cell["dense"]
    domain = valid_kmers(par)
    out = dict(seed=cell["seed"])
    if cell["index"] == "flat":
        bins, h, m = cell["bins"], cell["h"], 2003
        words = helpers.random_words(bins, m, 0.55 ** (1.0 / h), cell["seed"])  # a k-mer's mask keeps about half of the bins
        out["ox"] = helpers.oracle_ibf_from_words(O, bins, m, h, words, dna=bool(par["canonical"]), k=par["k"])
        out["upload"] = ("ibf", bins, m, h, words)
        user_bins = bins
    elif cell["index"] == "regular":
        shape, _, variant = cell["shape"].partition("-")
        children, per_child = (int(x) for x in shape.split("x"))
        user_bins = children * per_child - (5 if variant == "mixed" else 0)
        n = max(2, domain.size // 4)
        ox, descs, _ = helpers.regular_hibf(O, user_bins, children, n, lambda b: rng.choice(domain, size=n, replace=False), h=2,
                                            k=par["k"], mixed=variant == "mixed")
        out["ox"], out["upload"] = ox, ("hibf", user_bins, descs)
    else:
        user_bins = 150
        n = domain.size // 5

        def plant(values):  # every user bin: a fifth of all k-mers (split bins: runs of this list)
            for b in range(len(values)):
                values[b] = rng.choice(domain, size=n, replace=False)
        ox, descs, _ = helpers.layout_hibf(O, cell["seed"], user_bins, tmax=32, n_values=n, k=par["k"], plant=plant)
        out["ox"], out["upload"] = ox, ("hibf", user_bins, descs)
    spec = dict(W=(user_bins + 63) // 64, n_kmers=48, kmer_pool=domain if domain.size >= 48 else np.arange(4096, dtype=np.uint64),
                dense=par, dense_mode=cell["mode"], twins=4)
    if cell.get("many"):
        spec["many"] = cell["many"]
    if cell.get("aux"):  # the auxiliary index: the same bins, other rows and another hash count
        m2, h2 = 1201, 2
        words2 = helpers.random_words(user_bins, m2, 0.7, cell["seed"] + 1)
        out["dg"] = helpers.oracle_ibf_from_words(O, user_bins, m2, h2, words2)
        out["aux_upload"] = ("ibf", user_bins, m2, h2, words2)
        spec.update(n_aux_kmers=24, aux_pool=np.arange(1 << 16, dtype=np.uint64))
    out["spec"] = spec
    return out


def cell_session(cell, meta=None):
    return random_session(np.random.default_rng(cell["seed"] * 7 + 1), cell["spec"], meta)


def inventory(stages):
    """What the blobs of a session hold, read off their tables: a set of names, one per kind of op or shape found."""
    from tetrex_amd import host
    have = set()
    geometry = {}  # (program, block) -> (shape, capacity) of its last tracked ZERO
    for blob, qp, qs in stages:
        d = host.blob_dense(blob)
        par, table, blocks = d
        A, pos = par["alphabet"], par["k"] - 1
        full = (1 << A) - 1
        levels = host.blob_levels(blob)
        for p, ((n_slots, ops), ends) in enumerate(zip(host.parse_blob(blob)[1], levels)):
            if len(ends) >= 30:
                have.add("30 levels")
            begin = 0
            for end in ends:
                lv = ops[begin:end]
                begin = end
                acc = (lv[:, 0] == NO_KMER) & ((lv[:, 1] == lv[:, 2]) | (lv[:, 1] == lv[:, 3])) if len(lv) else np.zeros(0, bool)
                if len(lv) and acc.all():
                    for dst in np.unique(lv[:, 1]):
                        on = lv[lv[:, 1] == dst]
                        if len(on) >= 500 and (on[:, 2] == dst).any() and (on[:, 3] == dst).any():
                            have.add("500 accumulations onto %s" % ("RESULT" if dst == 2 else "a slot"))
                for o in lv:
                    k, dst, a, b = (int(x) for x in o)
                    if k != DENSE_OP:
                        if dst & DENSE_BIT:
                            have.add("ordinary op writes an entry")
                        if (a | b) & DENSE_BIT:
                            have.add("ordinary op reads an entry")
                        continue
                    row = [int(x) for x in table[dst]]
                    kind, ddst, src, r_mask, shape, res = row[0], row[1], row[2], row[3], row[4:4 + pos], row[15]
                    n = int(np.prod([bin(m).count("1") for m in shape]))
                    t = "tracked " if res & TRACKED else ""
                    if kind == ZERO and t:
                        key = (p, (ddst & ~DENSE_BIT) >> BLOCK_SHIFT)
                        have.add("tracked ZERO, capacity %s its geometry" % ("equal to" if src == n else "above"))
                        if key in geometry and geometry[key][0] != shape and geometry[key][1] == src:
                            have.add("tracked ZERO again, another geometry, same capacity")
                        geometry[key] = (shape, src)
                    elif kind == ZERO:
                        have.add("shaped ZERO" if r_mask else "full ZERO")
                    elif kind == FILL:
                        have.add(t + "FILL")
                    elif kind == REDUCE:
                        have.add(t + "REDUCE into " + ("an entry" if ddst & DENSE_BIT else "RESULT" if ddst == 2 else "a slot"))
                    else:
                        if res & NOPROBE:
                            have.add("NOPROBE STEP")
                        if t:
                            sk, dk = ((x & ~DENSE_BIT) >> BLOCK_SHIFT for x in (src, ddst))
                            if geometry[(p, sk)][0] != geometry[(p, dk)][0]:
                                have.add("tracked STEP between geometries")
                        elif not shape[0]:
                            have.add("STEP with an empty shape[0]")
                        elif all(m == full for m in shape) and r_mask == full:
                            have.add("STEP with full shapes")
                        elif bin(r_mask).count("1") == 1:
                            have.add("STEP with one residue")
                        elif all(m != full for m in shape) and r_mask != full:
                            have.add("STEP with proper subsets")
    return have


UNTRACKED_KINDS = {"full ZERO", "shaped ZERO", "FILL", "STEP with full shapes", "STEP with proper subsets", "STEP with one residue",
                   "STEP with an empty shape[0]", "REDUCE into a slot", "REDUCE into RESULT", "REDUCE into an entry"}
TRACKED_KINDS = {"tracked ZERO, capacity equal to its geometry", "tracked ZERO, capacity above its geometry",
                 "tracked ZERO again, another geometry, same capacity", "tracked FILL", "tracked STEP between geometries", "NOPROBE STEP",
                 "tracked REDUCE into a slot", "tracked REDUCE into RESULT"}
ORDINARY_KINDS = {"30 levels", "500 accumulations onto RESULT", "500 accumulations onto a slot", "ordinary op writes an entry",
                  "ordinary op reads an entry"}


def kinds_wanted(spec):
    mode = spec.get("dense_mode", "both")
    return ORDINARY_KINDS | (UNTRACKED_KINDS if mode != "tracked" else set()) | (TRACKED_KINDS if mode != "untracked" else set())


def host_programs(blob):
    from tetrex_amd import host
    return host.parse_blob(blob)[1]


def host_levels(blob):
    from tetrex_amd import host
    return host.blob_levels(blob)
