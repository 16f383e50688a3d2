"""The path choice and launch arithmetic of the HIBF descent (csrc/txq_hibf_descent_plan.hpp), restated in plain Python, and
the facts about a tree that it takes (what hibf_upload leaves in the Index: csrc/txq_hibf_plan.hpp read_tree, plan_maps,
plan_regular, plan_layout_order), computed from upload descriptors.  tests/test_hibf_descent_plan.py holds this against the header
(tests/native/hibf_descent_plan_dump.cpp); tests/test_gpu_hibf_scale.py asks it, before it runs a case, whether the case's tree,
batch and switches reach the kernel and the loop the case is written for."""
MERGED = 0xFFFFFFFFFFFFFFFF

INTERLEAVED, STATIONARY, SMALL, FUSED, LEVELS = range(5)  # DescentPath

SMALL_THREADS, SMALL_STACK = 256, 32     # kSmallThreads, kSmallStack
FUSED_LDS_BUDGET = 64 << 10              # kFusedLdsBudget
FUSED_WAVES = 256 * 64                   # kFusedWaves
SMALL_BLOCKS = 256 * 8                   # kSmallBlocks
ROOT_BLOCKS = 256 * 32                   # kRootBlocks
LEVEL_BLOCKS = 2048                      # kLevelBlocks
STATIONARY_TILE = 2048                   # kStationaryTile
LAYOUT_LEVEL_TILE = 2048                 # kLayoutLevelTile
CAP_ITEMS = 1 << 24                      # txq_count_plan.hpp kHibfCapItems

KNOBS = dict(levels=0, stationary=1, small=1, lane_hash=0, layout_fused=1, layout_direct=1, steps_per_group=0, tile=0, unroll=1, waves=0, stack_lds=128)
ENV = {"TXQ_HIBF_LEVELS": "levels", "TXQ_HIBF_STATIONARY": "stationary", "TXQ_HIBF_SMALL": "small", "TXQ_HIBF_LANE_HASH": "lane_hash",
       "TXQ_HIBF_LAYOUT_FUSED": "layout_fused", "TXQ_HIBF_LAYOUT_DIRECT": "layout_direct", "TXQ_HIBF_STEPS_PER_GROUP": "steps_per_group",
       "TXQ_HIBF_TILE": "tile", "TXQ_HIBF_UNROLL": "unroll", "TXQ_HIBF_WAVES": "waves", "TXQ_HIBF_STACK_LDS": "stack_lds"}

SHAPE_FIELDS = ("shard_words", "n_ibf", "total_tbs", "max_stride", "max_level_width", "depth", "has_nodes", "n_children", "child_row_words",
                "children_bytes", "children_uniform", "root_stride", "probes_interleaved")
KNOB_FIELDS = ("levels", "stationary", "small", "lane_hash", "steps_per_group", "tile", "unroll", "waves", "stack_lds")
LAYOUT_SHAPE_FIELDS = ("v_words", "n_ibf", "max_stride", "has_vnodes", "has_split", "v_inner_words", "n_groups")
LAYOUT_KNOB_FIELDS = ("layout_fused", "layout_direct", "waves", "stack_lds")
# the numbers of one answer of the dump tool, in its order
DESCENT_FIELDS = ("path",
                  "fused.ok", "fused.stack_lds", "fused.wave_bytes", "fused.waves_per_block", "fused.grid", "fused.G", "fused.w_iters",
                  "stat.ok", "stat.lanes_per_child", "stat.n_steps", "stat.steps_per_group", "stat.n_groups", "stat.groups_per_phase", "stat.phases", "stat.tile",
                  "stat.n_tiles", "stat.grid", "stat.root_blocks", "stat.unroll", "stat.uniform",
                  "small.applies", "small.blocks",
                  "lev.G", "lev.w_iters", "lev.chunk", "lev.cap", "lev.blocks0", "lev.blocks0_last", "lev.blocks_deeper", "lev.alive_blocks")
LAYOUT_FIELDS = ("fused.ok", "fused.stack_lds", "fused.row_lds_words", "fused.wave_bytes", "fused.waves_per_block", "fused.grid", "fused.G", "fused.w_iters",
                 "level.n_tiles", "level.phases", "level.grid", "level.piece")


def knobs(env=None, **kw):
    """The switches as the library reads them (txq_api.hip read_knobs) from a dict of TXQ_HIBF_* variables, or by field name."""
    k = dict(KNOBS)
    for name, value in (env or {}).items():
        if name in ENV:
            k[ENV[name]] = int(value)
    k.update(kw)
    k["steps_per_group"], k["tile"], k["waves"] = max(0, k["steps_per_group"]), max(0, k["tile"]), max(0, k["waves"])
    k["stack_lds"] = max(2, k["stack_lds"])
    k["levels"] = int(k["levels"] == 1)  # (set by "1")
    for f in ("lane_hash", "stationary", "small", "layout_fused", "layout_direct"):  # (the last four: cleared by "0")
        k[f] = int(k[f] != 0)
    return k


# ---- the tree ------------------------------------------------------------------------------------------------------------

def row_stride(words):
    """txq_hibf_plan.hpp row_stride: rows of an even number of words unless there is only one"""
    return 1 if words <= 1 else (words + 1) & ~1


def shard_range(words, r, R):
    base, rem = divmod(words, R)
    lo = base * r + min(r, rem)
    return lo, lo + base + (1 if r < rem else 0)


def levels_of(descs):
    """the IBFs of every level, breadth first from IBF 0 (read_tree)"""
    out, level = [], [0]
    while level:
        out.append(level)
        level = [int(c) for i in level for c, u in zip(descs[i]["next_ibf_id"], descs[i]["tb_to_user"]) if int(u) == MERGED]
    return out


def regular_two_level(user_bins, descs):
    """txq_hibf_plan.hpp regular_two_level: the words per child, or 0"""
    n = len(descs)
    if n < 2 or descs[0]["bins"] != n - 1:
        return 0
    wpr = (descs[1]["bins"] + 63) // 64
    if wpr < 1 or wpr & (wpr - 1) or wpr > 128 or (user_bins + 63) // 64 != wpr * (n - 1):
        return 0
    seen = set()
    for u, c in zip(descs[0]["tb_to_user"], descs[0]["next_ibf_id"]):
        if int(u) != MERGED or int(c) == 0 or int(c) >= n or int(c) in seen:
            return 0
        seen.add(int(c))
    cols = set()
    for d in descs[1:]:
        tbu = [int(u) for u in d["tb_to_user"]]
        if (d["bins"] + 63) // 64 != wpr or tbu[0] == MERGED or tbu[0] % (wpr * 64) or tbu != list(range(tbu[0], tbu[0] + d["bins"])):
            return 0
        col = tbu[0] // (wpr * 64)
        if col >= n - 1 or col in cols:
            return 0
        cols.add(col)
    return wpr


def shape_of(user_bins, descs, shard_rank=0, n_shards=1, interleave_probe=True, interleave=True):
    """DescentShape of an upload of `descs` (tetrex_amd.capi.Index.upload_hibf) as column shard shard_rank of n_shards"""
    mask_words = (user_bins + 63) // 64
    lo, hi = shard_range(mask_words, shard_rank, n_shards)
    sw = hi - lo
    strides = [row_stride((d["bins"] + 63) // 64) for d in descs]  # (every IBF of the tree is kept whole)
    lv = levels_of(descs)
    total = sum(d["bins"] for d in descs)
    moff = sum(((d["bins"] + 63) // 64 + 3) & ~3 for d in descs)
    compact = total < 0xFFFFFFFF and moff < 0xFFFFFFFF and total <= (256 << 20) // 32
    compact = compact and all(d["bin_size"] < (1 << 32) and s < (1 << 20) and d["hash_funs"] < 8 for d, s in zip(descs, strides))
    sh = dict(shard_words=sw, n_ibf=len(descs), total_tbs=total, max_stride=max(strides), max_level_width=max(len(l) for l in lv), depth=len(lv),
              has_nodes=int(compact), n_children=0, child_row_words=0, children_bytes=0, children_uniform=0, root_stride=strides[0], probes_interleaved=0)
    wpr = regular_two_level(user_bins, descs) if compact and len(lv) == 2 and descs[0]["bins"] < (1 << 20) else 0
    if wpr and lo % wpr == 0 and sw % wpr == 0 and sw:  # plan_regular
        by_col = {int(d["tb_to_user"][0]) // (wpr * 64): i + 1 for i, d in enumerate(descs[1:])}
        kids = [descs[by_col[c]] for c in range(lo // wpr, hi // wpr)]
        sh["n_children"], sh["child_row_words"] = len(kids), wpr
        sh["children_bytes"] = sum(d["bin_size"] * row_stride(wpr) * 8 for d in kids)
        sh["children_uniform"] = int(all((d["bin_size"], d["hash_funs"]) == (kids[0]["bin_size"], kids[0]["hash_funs"]) for d in kids))
        # RegularPlan::interleave, upload_regular and Index::probes_interleaved
        kept = sh["children_uniform"] and descs[0]["bins"] <= 64 and sw <= 32 and interleave
        st = row_stride(sw)
        sh["probes_interleaved"] = int(bool(kept and st >= 2 and not st & 1 and interleave_probe))
    return sh


def layout_shape_of(user_bins, descs, n_shards=1):
    """what plan_layout_order leaves for the layout-order kernels: row words, gate words, the groups of every level, split bins; None:
    the index has no layout order (a regular tree, a shard)"""
    sh = shape_of(user_bins, descs)
    lv = levels_of(descs)
    if sh["n_children"] or n_shards != 1 or len(lv) > 4 or any(d["hash_funs"] > 5 for d in descs):
        return None
    bw = [(d["bins"] + 63) // 64 for d in descs]
    exact, padded2 = sum(bw), sum((w + 1) & ~1 for w in bw)
    cwords = 1 if padded2 * 10 > exact * 13 else 2
    padded = [(w + cwords - 1) // cwords * cwords for w in bw]
    words = sum(padded)
    words += words & 1
    groups = []
    for level in lv:
        n_g, run = 0, 0
        for i in level:
            b = descs[i]["bin_size"] * row_stride(bw[i]) * 8
            if n_g == 0 or run + b > (2 << 20):
                n_g, run = n_g + 1, 0
            run += b
        groups.append(n_g)
    inner = sum(p for p, d in zip(padded, descs) if any(int(u) == MERGED for u in d["tb_to_user"]))
    split = False
    for d in descs:
        ubs = [int(u) for u in d["tb_to_user"] if int(u) != MERGED]
        split = split or len(set(ubs)) != len(ubs)
    return dict(v_words=words, n_ibf=len(descs), max_stride=sh["max_stride"], has_vnodes=sh["has_nodes"], has_split=int(split), v_inner_words=inner,
                groups=groups, n_groups=max(groups), chunk_words=cwords)


# ---- the plans -----------------------------------------------------------------------------------------------------------

def fused_stack_lds(stack_lds_knob, stack_cap, w_out):
    in_lds = max(2, stack_lds_knob) & ~1
    if in_lds >= stack_cap or stack_cap - in_lds > 2 * w_out:
        in_lds = (stack_cap + 1) & ~1
    return in_lds


def fused_waves_per_block(wave_bytes):
    best, best_resident = 1, 0
    for w in (4, 2, 1):
        if wave_bytes * w > (64 << 10):
            continue
        block = -(-(wave_bytes * w) // 1280) * 1280
        resident = min((160 << 10) // block * w, 32)
        if resident > best_resident:
            best, best_resident = w, resident
    return best


def fused_lanes(max_stride):
    quads = (max_stride + 3) // 4
    g = 1
    while g < 64 and g < quads:
        g <<= 1
    return g, -(-quads // g)


def _fused_grid(p, kn, n):
    p["waves_per_block"] = fused_waves_per_block(p["wave_bytes"])
    total = min(n, kn["waves"] if kn["waves"] > 0 else FUSED_WAVES)
    p["grid"] = -(-total // p["waves_per_block"])  # (the stride of a wave's k-mer loop is grid * waves_per_block)


def plan_fused(sh, kn, n):
    w_out = sh["shard_words"]
    p = dict(ok=0, stack_lds=fused_stack_lds(kn["stack_lds"], sh["n_ibf"], w_out), row_lds_words=w_out, waves_per_block=0, grid=0, G=1, w_iters=1)
    p["wave_bytes"] = (w_out + p["stack_lds"] // 2) * 8
    p["ok"] = int(bool(w_out and p["wave_bytes"] <= FUSED_LDS_BUDGET and sh["has_nodes"] and not kn["levels"]))
    if p["ok"]:
        _fused_grid(p, kn, n)
        p["G"], p["w_iters"] = fused_lanes(sh["max_stride"])
    return p


def plan_fused_layout(ls, kn, n):
    p = dict(ok=0, stack_lds=0, row_lds_words=0, wave_bytes=0, waves_per_block=0, grid=0, G=1, w_iters=1)
    if not ls["has_vnodes"] or not kn["layout_fused"]:
        return p
    p["stack_lds"] = (ls["n_ibf"] + 1) & ~1 if kn["layout_direct"] else fused_stack_lds(kn["stack_lds"], ls["n_ibf"], ls["v_words"])
    p["row_lds_words"] = 0 if kn["layout_direct"] else ls["v_words"]
    p["wave_bytes"] = (p["row_lds_words"] + p["stack_lds"] // 2) * 8
    if p["wave_bytes"] > FUSED_LDS_BUDGET:
        return p
    _fused_grid(p, kn, n)
    p["G"], p["w_iters"] = fused_lanes(ls["max_stride"])
    p["ok"] = int(not (p["w_iters"] > 1 and ls["has_split"]))
    return p


def plan_stationary(sh, kn, n):
    p = dict(ok=0, lanes_per_child=0, n_steps=0, steps_per_group=0, n_groups=0, groups_per_phase=0, phases=0, tile=0, n_tiles=0, grid=0, root_blocks=0, unroll=4, uniform=0)
    if not sh["n_children"] or sh["child_row_words"] < 2 or sh["shard_words"] <= 16 or not kn["stationary"]:
        return p
    lpc = sh["child_row_words"] // 2
    cps = 64 // lpc
    n_steps = -(-sh["n_children"] // cps)
    per_step = sh["children_bytes"] // n_steps + 1
    spg = max(1, (2 << 20) // per_step)
    if n_steps >= 8 and -(-n_steps // spg) < 8:
        spg = n_steps // 8
    if kn["steps_per_group"]:
        spg = kn["steps_per_group"]
    n_groups = -(-n_steps // spg)
    gpp = min(n_groups, 8)
    phases = -(-n_groups // gpp)
    tile = max(64, kn["tile"]) if kn["tile"] else STATIONARY_TILE
    n_tiles = -(-n // tile)
    p.update(lanes_per_child=lpc, children_per_step=cps, n_steps=n_steps, steps_per_group=spg, n_groups=n_groups, groups_per_phase=gpp, phases=phases, tile=tile, n_tiles=n_tiles)
    if not (phases * n_tiles * gpp < (1 << 31) and n_tiles < (1 << 31)):
        return p
    p["ok"], p["grid"], p["root_blocks"] = 1, phases * n_tiles * gpp, min(-(-n // 256), ROOT_BLOCKS)
    p["uniform"] = int(bool(sh["children_uniform"] and not kn["lane_hash"]))
    u = kn["unroll"]
    p["unroll"] = u if u in (1, 2, 8) or (u == 3 and p["uniform"]) else 4
    return p


def small_applies(sh, kn):
    return int(bool(sh["max_stride"] <= 4 and sh["n_ibf"] <= SMALL_STACK and sh["total_tbs"] < 0xFFFF and sh["shard_words"] <= 16 and kn["small"]))


def small_blocks(n):
    return min(-(-n // SMALL_THREADS), SMALL_BLOCKS)


def level_blocks(g, lvl, m):
    groups = LEVEL_BLOCKS * 256 // g if lvl else m
    return max(1, min(-(-(groups * g) // 256), LEVEL_BLOCKS))


def plan_levels(sh, n):
    chunk = min(max(1, CAP_ITEMS // sh["max_level_width"]), n)
    g = 1
    while g < 64 and g < sh["max_stride"]:
        g <<= 1
    last = n % chunk or chunk
    return dict(G=g, w_iters=-(-sh["max_stride"] // g), chunk=chunk, cap=chunk * sh["max_level_width"], blocks0=level_blocks(g, 0, chunk),
                blocks0_last=level_blocks(g, 0, last), blocks_deeper=level_blocks(g, 1, 0), alive_blocks=min(-(-(-(-n // 64) * 64) // 256), LEVEL_BLOCKS))


def descent_path(sh, kn, n):
    if sh["probes_interleaved"]:
        return INTERLEAVED
    if not plan_fused(sh, kn, n)["ok"]:
        return LEVELS
    if plan_stationary(sh, kn, n)["ok"]:
        return STATIONARY
    if small_applies(sh, kn):
        return SMALL
    return FUSED


def layout_level(ls, n):
    n_tiles = -(-n // LAYOUT_LEVEL_TILE)
    phases = (ls["n_groups"] + 7) // 8
    grid = phases * n_tiles * 8
    piece = max(4 << 20, ((96 << 20) // (max(ls["v_inner_words"], 1) * 8)) // LAYOUT_LEVEL_TILE * LAYOUT_LEVEL_TILE)
    return dict(n_tiles=n_tiles, phases=phases, grid=0 if grid >= (1 << 31) else grid, piece=piece)


# ---- one line of the dump tool ---------------------------------------------------------------------------------------------

def descent_command(sh, kn, n):
    return "descent " + " ".join(str(int(sh[f])) for f in SHAPE_FIELDS) + "  " + " ".join(str(int(kn[f])) for f in KNOB_FIELDS) + "  %d" % n


def descent_numbers(sh, kn, n):
    """what the tool answers to descent_command(sh, kn, n)"""
    f, c, l = plan_fused(sh, kn, n), plan_stationary(sh, kn, n), plan_levels(sh, n)
    return [descent_path(sh, kn, n),
            f["ok"], f["stack_lds"], f["wave_bytes"], f["waves_per_block"], f["grid"], f["G"], f["w_iters"],
            c["ok"], c["lanes_per_child"], c["n_steps"], c["steps_per_group"], c["n_groups"], c["groups_per_phase"], c["phases"], c["tile"], c["n_tiles"], c["grid"],
            c["root_blocks"], c["unroll"], c["uniform"],
            small_applies(sh, kn), small_blocks(n),
            l["G"], l["w_iters"], l["chunk"], l["cap"], l["blocks0"], l["blocks0_last"], l["blocks_deeper"], l["alive_blocks"]]


def layout_command(ls, kn, n):
    return "layout " + " ".join(str(int(ls[f])) for f in LAYOUT_SHAPE_FIELDS) + "  " + " ".join(str(int(kn[f])) for f in LAYOUT_KNOB_FIELDS) + "  %d" % n


def layout_numbers(ls, kn, n):
    f, v = plan_fused_layout(ls, kn, n), layout_level(ls, n)
    return [f["ok"], f["stack_lds"], f["row_lds_words"], f["wave_bytes"], f["waves_per_block"], f["grid"], f["G"], f["w_iters"],
            v["n_tiles"], v["phases"], v["grid"], v["piece"]]
