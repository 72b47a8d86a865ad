"""Python mirror of the run-time instantiation choice of every dense forward / dX / dW launcher (no GPU needed).

Each launcher of librgcn_mi355x.so picks a template instantiation from the widths, the plan geometry (tile, chunk,
chunk_rows, layout, tile count), the flags and whether the gathered matrices fit a buffer descriptor.  The functions
below restate those rules, one per launcher, and return the instantiation tuple the launch runs or ("err", status).
``reachable()`` enumerates what each launcher can run over widths 1..128, every tile and chunk ``check_plan`` accepts,
both addressing modes and every flag combination.  tests/test_kernel_variants.py pins the constants to the C sources
and checks that tests/test_gpu_kernel_variants.py has a case for every reachable tuple.

Tuples:
  ("tile", KP, NP, NBUF, BUF, CH, merged)      rgcn_tile_kernel<KP, NP, NBUF, BUF, CH>, merged = layout-3 plan
  ("tile3p", ST, layout, multi)                rgcn_tile3p_kernel<ST>; multi = a workgroup walks more than one tile
  ("tpw", t)                                   rgcn_tile_kernel launched with t tiles per workgroup
  ("dw", KP, NP, NBUF, BUF, upb)               rgcn_dw_kernel<KP, NP, NBUF, BUF>, upb units per workgroup
  ("dw_wide", KP, NP, NBUF, BUF, CONS, upb)    rgcn_dw_wide_kernel<KP, NP, NBUF, BUF, CONS>
  ("dw_direct", upb)                           rgcn_dw_direct_kernel
  ("dw_root_only", chunk, rows)                RGCN_FLAG_DW_ROOT_ONLY walk of a plan whose chunks hold `rows` rows
  ("dw_tiles", SPLIT, PAIRS)                   rgcn_dw_tile_kernel<SPLIT, PAIRS>
  ("ep", KP, NP) / ("ep3",)                    rgcn_ep_transform_kernel<KP, NP> / rgcn_ep_transform3_kernel
  ("segsum", G)                                rgcn_ep_segment_sum_kernel<G>
"""
from __future__ import annotations

from functools import lru_cache

# ---- constants the rules use (tests/test_kernel_variants.py reads each of them back from the C sources) ---------------
LDS_BYTES = 160 * 1024          # rgcn_common.h kLdsBytes
ACC_PAD = 4                     # rgcn_tile_common.h kAccStride<NP> = NP + ACC_PAD
TILE_PRODUCERS = 4              # rgcn_tile_fp32_kernel.h kTileProducers
TILE_RING_PAD = 2               # launch_tile: a ring slot row holds KP + 2 floats (row index + weight)
TPW_CUS = 256                   # tiles_per_workgroup: kCUs
TPW_MAX = 16                    # ... t = 1..16
TPW_STARTUP = 0.04              # ... cost = rounds * (t + 0.04)
TPW_SLACK = 1.002               # ... ties within 0.2 % go to the larger count
P3_MULTI_MIN_TILES = 16 * 256   # launch_tile3p: one tile per workgroup below this many tiles
P3_ST7_ROWS = 112               # launch_tile3p: chunk_rows <= 112 -> ST = 7, else 8
P3_CH = 128                     # rgcn_tile3p.hip kP3CH
DW_CHUNK = 64                   # rgcn_common.h kChunk
DW_BLOCKS = 512                 # rgcn_dw_relmajor.hip kDwBlocks
DW_RING_BLOCKS = 256            # ... kDwRingBlocks
DW_DIRECT_MIN_UNITS = 16 * 1024  # ... kDwDirectMinUnits
DW_WIDE_CONSUMERS = 4           # ... kWideConsumers
DW_WIDE_MAX_AREA = 64 * 128     # launch_dw: kWide = KP % 64 == 0 && NP % 64 == 0 && KP * NP <= 64 * 128
DW_WIDE_TWO_TEAM_AREA = 64 * 64  # ... CONS = KP * NP <= 64 * 64 ? kWideConsumers : 4
DW_UPB = 4                      # rgcn_bwd_dw: units per workgroup (every plan layout)
DW_TILE_T = 320                 # rgcn_dw_tile.hip kDwTileT
DW_TILE_MAX_REL = 32            # ... kDwTileMaxRel
SEGSUM_G = ((4, 4), (8, 8), (16, 16))   # rgcn_ep_segment_sum: G = 4 if ld4 <= 4, 8 if <= 8, 16 if <= 16, else 32
SEGSUM_G_MAX = 32

OK, ERR_WIDTH, ERR_PLAN, ERR_LDS, ERR_ADDRESS = 0, -2, -4, -5, -10
FLAG_POINTER_GATHER, FLAG_DW_RING, FLAG_DW_DIRECT, FLAG_EXACT_FP32, FLAG_DW_ROOT_ONLY, FLAG_SPLIT_PRODUCERS = 1, 2, 4, 8, 16, 32
TILE_FLAGS = FLAG_SPLIT_PRODUCERS | FLAG_EXACT_FP32
ALL_FLAGS = (FLAG_POINTER_GATHER, FLAG_DW_RING, FLAG_DW_DIRECT, FLAG_EXACT_FP32, FLAG_DW_ROOT_ONLY, FLAG_SPLIT_PRODUCERS)

WIDTHS = range(1, 129)
TILES = range(16, 32768 + 1, 16)
# (chunk, chunk_rows, layout) of every plan header check_plan accepts that rgcn_plan_build makes (chunk_rows 0 means "the
# chunk"; 112-row chunks in layouts 0 / 3 only, layouts 2 and 5 with 64-slot chunks only)
PLAN_FORMS = [(c, cr, lay) for c in (64, 128) for cr in (0, c, 112) for lay in (0, 1, 2, 3, 5)
              if not (cr == 112 and (c != 128 or lay not in (0, 3))) and not (lay in (1, 3) and c != 128)
              and not (lay in (2, 5) and c != 64)]


def err(status):
    return ("err", status)


def padded_width(w):
    if w < 1 or w > 128:
        return 0
    return 16 if w <= 16 else 32 if w <= 32 else 64 if w <= 64 else 128


def tiles_per_workgroup(n_tiles):
    best, best_cost = 1, 1e30
    for t in range(1, TPW_MAX + 1):
        wgs = (n_tiles + t - 1) // t
        rounds = (wgs + TPW_CUS - 1) // TPW_CUS
        cost = rounds * (t + TPW_STARTUP)
        if cost <= best_cost * TPW_SLACK:
            best_cost = min(cost, best_cost)
            best = t
    return best


def tile_lds_bytes(KP, NP, tile, chunk, nbuf):
    return 4 * ((tile + 1) * (NP + ACC_PAD) + nbuf * chunk * (KP + TILE_RING_PAD))


@lru_cache(maxsize=None)
def launch_tile(KP, NP, tile, chunk, merged, buf):
    """rgcn_tile_fp32_kernel.h launch_tile: the deepest ring that fits beside the accumulator"""
    fits = lambda nbuf: tile_lds_bytes(KP, NP, tile, chunk, nbuf) <= LDS_BYTES
    if chunk == 128:
        if KP <= 64:
            if fits(3) and not merged:
                return ("tile", KP, NP, 3, buf, 128, merged)
            if fits(2):
                return ("tile", KP, NP, 2, buf, 128, merged)
        return err(ERR_LDS)
    if TILE_PRODUCERS >= 3 and KP < 128 and fits(4):
        return ("tile", KP, NP, 4, buf, 64, merged)
    if KP < 128 and fits(3):
        return ("tile", KP, NP, 3, buf, 64, merged)
    if fits(2):
        return ("tile", KP, NP, 2, buf, 64, merged)
    return err(ERR_LDS)


def p3_lds_bytes(tile, st):
    return 4 * (tile + 1) * (64 + ACC_PAD) + 2 * (3 * 16 * st * 128) + 2 * P3_CH * 8


def p3_st(chunk_rows):
    return 7 if 0 < chunk_rows <= P3_ST7_ROWS else 8


def launch_tile3p(tile, chunk_rows, layout, buf, n_tiles):
    if not buf:
        return err(ERR_PLAN)
    st = p3_st(chunk_rows)
    if p3_lds_bytes(tile, st) > LDS_BYTES:
        return err(ERR_LDS)
    tpw = 1 if n_tiles < P3_MULTI_MIN_TILES else tiles_per_workgroup(n_tiles)
    return ("tile3p", st, layout, tpw > 1)


def run_tile(din, dout, tile, chunk, chunk_rows, layout, flags, buffer_addressable, n_tiles):
    """rgcn_fwd / rgcn_bwd_dx (run_tile in rgcn_tile_fp32.hip): din = gathered width, dout = stored width"""
    if layout in (2, 5):
        return err(ERR_PLAN)
    KP, NP = padded_width(din), padded_width(dout)
    if KP == 0 or NP == 0:
        return err(ERR_WIDTH)
    buf = bool(buffer_addressable) and not (flags & FLAG_POINTER_GATHER)
    if (flags & FLAG_SPLIT_PRODUCERS) and not (flags & FLAG_EXACT_FP32) and KP == 64 and NP == 64 and chunk == 128 and buf:
        r = launch_tile3p(tile, chunk_rows, layout, buf, n_tiles)
        if r != err(ERR_LDS) or layout == 3:
            return r
    if layout == 3 and not (KP == 64 and NP == 64 and chunk == 128 and buf):
        return err(ERR_PLAN)
    return launch_tile(KP, NP, tile, chunk, layout == 3, buf)


def tile_tpw(din, dout, tile, chunk, chunk_rows, layout, flags, buffer_addressable, n_tiles):
    """tiles per workgroup of the launch run_tile makes (None: no rgcn_tile_kernel launch)"""
    r = run_tile(din, dout, tile, chunk, chunk_rows, layout, flags, buffer_addressable, n_tiles)
    return ("tpw", tiles_per_workgroup(n_tiles)) if r[0] == "tile" else None


def dw_nbuf(KP, NP):
    return 2 if KP == 128 or NP == 128 else 4


def launch_dw(KP, NP, buf, upb):
    nbuf = dw_nbuf(KP, NP)
    wide = KP % 64 == 0 and NP % 64 == 0 and KP * NP <= DW_WIDE_MAX_AREA
    lds = 4 * (nbuf * DW_CHUNK * (KP + NP + 1) + (2 * (2 * nbuf - 1) * DW_CHUNK if wide else 0))
    if lds > LDS_BYTES:
        return err(ERR_LDS)
    if wide:
        cons = DW_WIDE_CONSUMERS if KP * NP <= DW_WIDE_TWO_TEAM_AREA else 4
        return ("dw_wide", KP, NP, nbuf, buf, cons, upb)
    return ("dw", KP, NP, nbuf, buf, upb)


def bwd_dw(din, dout, tile, chunk, chunk_rows, layout, flags, buffer_addressable, n_tiles, n_units=1):
    """rgcn_bwd_dw: which relation-major kernel the launch runs"""
    if layout in (3, 5):
        return err(ERR_PLAN)
    if (flags & FLAG_DW_ROOT_ONLY) and layout == 2:
        return err(ERR_PLAN)
    KP, NP = padded_width(din), padded_width(dout)
    if KP == 0 or NP == 0:
        return err(ERR_WIDTH)
    buf = bool(buffer_addressable) and not (flags & FLAG_POINTER_GATHER)
    upb = DW_UPB
    can_direct = KP == 64 and NP == 64 and buf
    want_direct = can_direct and not (flags & FLAG_DW_RING) and (bool(flags & FLAG_DW_DIRECT) or n_units >= DW_DIRECT_MIN_UNITS)
    if want_direct:
        return ("dw_direct", upb)
    return launch_dw(KP, NP, buf, upb)


def root_units(n_owned, n_tiles, tile, chunk, chunk_rows):
    """rgcn_bwd_dw's closed form for the number of root units that close rel_order (RGCN_FLAG_DW_ROOT_ONLY)"""
    cap = (chunk_rows if chunk_rows > 0 else chunk) // 16

    def units_of(rows):
        nt = (rows + 15) // 16
        if cap * 16 == chunk:
            return (nt + 3) // 4
        return nt // cap * ((cap + 3) // 4) + (nt % cap + 3) // 4
    last_rows = n_owned - (n_tiles - 1) * tile
    return (n_tiles - 1) * units_of(tile) + units_of(last_rows)


def dw_root_only(din, dout, tile, chunk, chunk_rows, layout, flags, buffer_addressable, n_tiles):
    if layout in (2, 3, 5):
        return err(ERR_PLAN)
    if padded_width(din) == 0 or padded_width(dout) == 0:
        return err(ERR_WIDTH)
    return ("dw_root_only", chunk, chunk_rows if chunk_rows > 0 else chunk)


def bwd_dw_tiles(din, dout, tile, chunk, chunk_rows, layout, flags, buffer_addressable, n_tiles, num_relations=1):
    """rgcn_bwd_dw_tiles"""
    if padded_width(din) != 64 or padded_width(dout) != 64:
        return err(ERR_WIDTH)
    if tile != DW_TILE_T or chunk != 64 or layout not in (0, 5) or num_relations > DW_TILE_MAX_REL:
        return err(ERR_PLAN)
    if not buffer_addressable or (flags & FLAG_POINTER_GATHER):
        return err(ERR_ADDRESS)
    return ("dw_tiles", bool(flags & FLAG_SPLIT_PRODUCERS), layout == 5)


def ep_transform(din, dout, tile, chunk, chunk_rows, layout, flags, buffer_addressable, n_tiles):
    """rgcn_ep_transform (the plan geometry does not enter: edge units are relation-major 64-row blocks)"""
    KP, NP = padded_width(din), padded_width(dout)
    if KP == 0 or NP == 0:
        return err(ERR_WIDTH)
    buf = bool(buffer_addressable) and not (flags & FLAG_POINTER_GATHER)
    if KP == 64 and NP == 64 and buf and (flags & FLAG_SPLIT_PRODUCERS) and not (flags & FLAG_EXACT_FP32):
        return ("ep3",)
    return ("ep", KP, NP)


def segsum_g(width):
    ld4 = (width + 3) // 4
    for lim, g in SEGSUM_G:
        if ld4 <= lim:
            return g
    return SEGSUM_G_MAX


def ep_segment_sum(din, dout, tile, chunk, chunk_rows, layout, flags, buffer_addressable, n_tiles):
    """rgcn_ep_segment_sum over rows of width dout"""
    if padded_width(dout) == 0:
        return err(ERR_WIDTH)
    return ("segsum", segsum_g(dout))


def _flag_sets():
    out = []
    for m in range(1 << len(ALL_FLAGS)):
        f = 0
        for i, b in enumerate(ALL_FLAGS):
            if m >> i & 1:
                f |= b
        out.append(f)
    return out


@lru_cache(maxsize=None)
def reachable():
    """{launcher: set of instantiation tuples} over the whole argument space"""
    classes = sorted({padded_width(w) for w in WIDTHS})
    reps = {c: max(w for w in WIDTHS if padded_width(w) == c) for c in classes}   # the rules see widths through padded_width
    flag_sets = [f for f in _flag_sets() if not (f & FLAG_POINTER_GATHER)]         # pointer gather == not addressable
    out = {k: set() for k in ("tile", "tile3p", "tpw", "dw", "dw_root_only", "dw_tiles", "ep", "segsum")}
    # the tile-kernel rules depend on the tile through the LDS budget only; the tile count only through the tiles per workgroup
    tile_counts = sorted({1, P3_MULTI_MIN_TILES - 1, P3_MULTI_MIN_TILES, P3_MULTI_MIN_TILES + 1})
    for chunk, cr, lay in PLAN_FORMS:
        for KP in classes:
            for NP in classes:
                din, dout = reps[KP], reps[NP]
                for buf in (True, False):
                    # run_tile reads no flag bit but these two (and the pointer-gather bit, folded into buf); the tile count
                    # only in launch_tile3p (64 x 64)
                    for f in {f & TILE_FLAGS for f in flag_sets}:
                        for nt in (tile_counts if KP == 64 and NP == 64 else [1]):
                            for tile in TILES:
                                r = run_tile(din, dout, tile, chunk, cr, lay, f, buf, nt)
                                out["tile3p" if r[0] == "tile3p" else "tile"].add(r)
                                if r[0] == "err":       # ERR_LDS: the LDS bytes grow with the tile; any other error ignores it
                                    break
                    for f in flag_sets:
                        out["dw"].add(bwd_dw(din, dout, 16, chunk, cr, lay, f, buf, 1, 1))
                        out["dw"].add(bwd_dw(din, dout, 16, chunk, cr, lay, f, buf, 1, DW_DIRECT_MIN_UNITS))
                        out["dw_root_only"].add(dw_root_only(din, dout, 16, chunk, cr, lay, f, buf, 1))
                        out["dw_tiles"].add(bwd_dw_tiles(din, dout, DW_TILE_T, chunk, cr, lay, f, buf, 1))
                        out["ep"].add(ep_transform(din, dout, 16, chunk, cr, lay, f, buf, 1))
                        out["segsum"].add(ep_segment_sum(din, dout, 16, chunk, cr, lay, f, buf, 1))
    for w in WIDTHS:
        out["segsum"].add(ep_segment_sum(w, w, 16, 64, 0, 0, 0, True, 1))
    # tiles per workgroup: every tile count up to the largest plan (n_tiles * tile <= 2^31)
    n = 1
    while n <= 1 << 20:
        out["tpw"].add(("tpw", tiles_per_workgroup(n)))
        n += 1 if n < 70000 else 997
    return {k: {x for x in v if x[0] != "err"} for k, v in out.items()}
