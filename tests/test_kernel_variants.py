"""The launcher mirror of tests/kernel_variants.py against the C sources, and the case table of
tests/test_gpu_kernel_variants.py against the mirror's reachable set (no GPU needed)."""
import os
import re

import pytest

from tests import kernel_variants as K
from tests import test_gpu_kernel_variants as G

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scaling_rgcn_training_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"\s+", " ", f.read())        # one line, single spaces: expressions match across line breaks


def _one(name, pattern):
    m = re.findall(pattern, _src(name))
    assert len(m) == 1, f"{name}: {pattern!r} matched {len(m)} times -- the launcher changed; update tests/kernel_variants.py"
    return m[0]


def _num(expr):
    assert re.fullmatch(r"[0-9 *+()]+", expr), expr
    return eval(expr)       # a product of integer literals, as the sources write their constants


def test_mirror_constants_match_sources():
    assert _num(_one("rgcn_common.h", r"constexpr int kLdsBytes = ([^;]+);")) == K.LDS_BYTES
    assert _num(_one("rgcn_common.h", r"constexpr int kChunk = ([^;]+);")) == K.DW_CHUNK
    assert int(_one("rgcn_tile_common.h", r"constexpr int kAccStride = NP \+ (\d+);")) == K.ACC_PAD
    assert int(_one("rgcn_tile_fp32_kernel.h", r"constexpr int kTileProducers = (\d+);")) == K.TILE_PRODUCERS
    # launch_tile: LDS bytes and the ring-depth ladder
    assert int(_one("rgcn_tile_fp32_kernel.h", r"kAccStride<NP> \+ \(size_t\)nbuf \* chunk \* \(KP \+ (\d+)\)\);")) == K.TILE_RING_PAD
    ladder = re.findall(r"launch_tile_nbuf<KP, NP, (\d), (\d+)>", _src("rgcn_tile_fp32_kernel.h"))
    assert ladder == [("3", "128"), ("2", "128"), ("4", "64"), ("3", "64"), ("2", "64")]
    assert _one("rgcn_tile_fp32_kernel.h", r"if \(bytes\(3\) <= cap && (!a\.merged)\)") == "!a.merged"
    assert _one("rgcn_tile_fp32_kernel.h", r"if constexpr \(KP <= (\d+)\) \{ //") == "64"
    assert _one("rgcn_tile_fp32_kernel.h", r"if \(KP < (\d+) && bytes\(4\) <= cap\)") == "128"
    # tiles_per_workgroup
    tpw = _one("rgcn_kernels_shared.h", r"static int tiles_per_workgroup\(int n_tiles\) \{(.*?)return best; \}")
    assert re.search(r"kCUs = (\d+);", tpw).group(1) == str(K.TPW_CUS)
    assert re.search(r"for \(int t = 1; t <= (\d+); \+\+t\)", tpw).group(1) == str(K.TPW_MAX)
    assert float(re.search(r"rounds \* \(t \+ ([0-9.]+)\)", tpw).group(1)) == K.TPW_STARTUP
    assert float(re.search(r"best_cost \* ([0-9.]+)\)", tpw).group(1)) == K.TPW_SLACK
    # ring depths of the relation-major dW kernels (and the tile kernel's nominal one)
    assert _one("rgcn_kernels_shared.h", r"constexpr int tile_nbuf\(\) \{ return (KP == 128 \? 2 : 4); \}") == "KP == 128 ? 2 : 4"
    assert _one("rgcn_kernels_shared.h", r"constexpr int dw_nbuf\(\) \{ return \((KP == 128 \|\| NP == 128)\) \? 2 : 4; \}")
    assert all(K.dw_nbuf(kp, np_) == (2 if 128 in (kp, np_) else 4) for kp in (16, 32, 64, 128) for np_ in (16, 32, 64, 128))
    # rgcn_tile3p: ST rule, multi-tile threshold, LDS bytes
    st = _one("rgcn_tile3p.hip", r"const int st = chunk_rows > 0 && chunk_rows <= (\d+) \? 7 : 8;")
    assert int(st) == K.P3_ST7_ROWS
    assert _num(_one("rgcn_tile3p.hip", r"if \(n_tiles < ([0-9 *]+)\) b\.tiles_per_wg = 1;")) == K.P3_MULTI_MIN_TILES
    assert int(_one("rgcn_tile3p.hip", r"constexpr int kP3CH = (\d+);")) == K.P3_CH
    assert _one("rgcn_tile3p.hip", r"constexpr int kP3LDO = kAccStride<(\d+)>;") == "64"
    p3 = _one("rgcn_tile3p.hip", r"static size_t p3_lds_bytes\(int tile, int st\) \{ return ([^;]+); \}")
    assert p3 == "sizeof(float) * (size_t)(tile + 1) * kP3LDO + 2 * (size_t)(3 * 16 * st * 128) + 2 * kP3CH * 8", p3
    # relation-major dW: wide rule, consumer count, LDS, direct threshold, units per workgroup
    dw = "rgcn_dw_relmajor.hip"
    assert _num(_one(dw, r"constexpr int kDwBlocks = (\d+);")) == K.DW_BLOCKS
    assert _num(_one(dw, r"constexpr int kDwRingBlocks = (\d+);")) == K.DW_RING_BLOCKS
    assert _num(_one(dw, r"constexpr int kDwDirectMinUnits = ([0-9 *]+);")) == K.DW_DIRECT_MIN_UNITS
    assert _num(_one(dw, r"constexpr int kWideConsumers = (\d+);")) == K.DW_WIDE_CONSUMERS
    assert _num(_one(dw, r"constexpr bool kWide = KP % 64 == 0 && NP % 64 == 0 && KP \* NP <= ([0-9 *]+);")) == K.DW_WIDE_MAX_AREA
    assert _num(_one(dw, r"constexpr int CONS = KP \* NP <= ([0-9 *]+) \? kWideConsumers : 4;")) == K.DW_WIDE_TWO_TEAM_AREA
    assert _one(dw, r"const size_t lds = sizeof\(float\) \* \(([^;]+)\);") == \
        "(size_t)NBUF * kChunk * (KP + NP + 1) + (kWide ? 2 * (2 * NBUF - 1) * kChunk : 0)"
    assert int(_one(dw, r"const int upb = (\d+);")) == K.DW_UPB
    assert _one(dw, r"const bool can_direct = ([^;]+);") == "KP == 64 && NP == 64 && xb != 0 && gb != 0"
    # tile-major dW geometry
    assert int(_one("rgcn_dw_tile.hip", r"constexpr int kDwTileT = (\d+);")) == K.DW_TILE_T
    assert int(_one("rgcn_dw_tile.hip", r"constexpr int kDwTileMaxRel = (\d+);")) == K.DW_TILE_MAX_REL
    # edge-parallel segment sum: G thresholds (the rule every row-group launch shares, rgcn_launch.h)
    g = _one("rgcn_launch.h", r"inline int lanes_per_row\(int width4\) \{ return width4 <= (\d+) \? (\d+) : \(width4 <= (\d+) \? (\d+) : \(width4 <= (\d+) \? (\d+) : (\d+)\)\); \}")
    assert re.search(r"rgcn_ep_segment_sum\(.*?return launch_row_groups\(ld4, n_out,", _src("rgcn_ep.hip"), re.S)
    assert tuple(map(int, g)) == tuple(v for pair in K.SEGSUM_G for v in pair) + (K.SEGSUM_G_MAX,)


# the branch conditions each mirror function restates, as they stand in the C sources (whitespace normalised)
BRANCHES = {
    "rgcn_tile_fp32.hip": [      # run_tile
        "if (plan->layout == 2) return RGCN_ERR_PLAN;",
        "if (plan->layout == 5) return RGCN_ERR_PLAN;",
        "if ((flags & RGCN_FLAG_SPLIT_PRODUCERS) && !(flags & RGCN_FLAG_EXACT_FP32) && KP == 64 && NP == 64 && plan->chunk == 128 && "
        "a.x_bytes != 0) {",
        "const int st3 = launch_tile3p(b, plan->n_tiles, plan->chunk_rows, stream); if (st3 != RGCN_ERR_LDS || plan->layout == 3) return st3;",
        "if (plan->layout == 3 && !(KP == 64 && NP == 64 && plan->chunk == 128 && a.x_bytes != 0)) return RGCN_ERR_PLAN;",
        "a.merged = plan->layout == 3 ? 1 : 0;",
        "a.tiles_per_wg = tiles_per_workgroup(plan->n_tiles);",
        "a.x_bytes = buffer_bytes(plan->n_nodes, ldx, flags);",
    ],
    "rgcn_tile3p.hip": [         # launch_tile3p
        "if (a.x_bytes == 0) return RGCN_ERR_PLAN;",
        "if (lds > (size_t)kLdsBytes) return RGCN_ERR_LDS;",
        "if (st == 7) return launch_tile3p_as<7>(b, nwg, lds, (hipStream_t)stream); return launch_tile3p_as<8>(b, nwg, lds, (hipStream_t)stream);",
    ],
    "rgcn_ep.hip": [             # rgcn_ep_transform
        "if (KP == 64 && NP == 64 && a.x_bytes != 0 && (flags & RGCN_FLAG_SPLIT_PRODUCERS) && !(flags & RGCN_FLAG_EXACT_FP32)) {",
        "a.x_bytes = buffer_bytes(units->n_nodes, ldx, flags);",
        "const int ld4 = (width + 3) / 4;",
    ],
    "rgcn_dw_tile.hip": [        # rgcn_bwd_dw_tiles
        "if (padded_width(din) != 64 || padded_width(dout) != 64) return RGCN_ERR_WIDTH; if (plan->tile != kDwTileT || plan->chunk != 64 || "
        "(plan->layout != 0 && plan->layout != 5) || plan->num_relations > kDwTileMaxRel) return RGCN_ERR_PLAN;",
        "if (a.x_bytes == 0 || a.g_bytes == 0) return RGCN_ERR_ADDRESS;",
        "const bool split = (flags & RGCN_FLAG_SPLIT_PRODUCERS) != 0;",
        "a.slot_src2 = plan->layout == 5 ? plan->slot_src2 : nullptr;",
    ],
    "rgcn_dw_relmajor.hip": [    # rgcn_bwd_dw, the root-only closed form included
        "if (plan->layout == 3) return RGCN_ERR_PLAN;",
        "if (plan->layout == 5) return RGCN_ERR_PLAN;",
        "if (flags & RGCN_FLAG_DW_ROOT_ONLY) { if (plan->layout == 2) return RGCN_ERR_PLAN;",
        "const long cap = (plan->chunk_rows > 0 ? plan->chunk_rows : plan->chunk) / 16;",
        "const long nt = (rows + 15) / 16; if (cap * 16 == plan->chunk) return (nt + 3) / 4; return nt / cap * ((cap + 3) / 4) + (nt % cap + 3) / 4;",
        "const long last_rows = (long)plan->n_owned - (long)(plan->n_tiles - 1) * plan->tile;",
        "const long root_units = (long)(plan->n_tiles - 1) * units_of(plan->tile) + units_of(last_rows);",
        "const unsigned xb = buffer_bytes(plan->n_nodes, ldx, flags), gb = buffer_bytes(plan->n_owned, ldg, flags);",
        "const bool want_direct = can_direct && !(flags & RGCN_FLAG_DW_RING) && ((flags & RGCN_FLAG_DW_DIRECT) || n_units >= kDwDirectMinUnits);",
        "const bool buf = a.x_bytes && a.g_bytes;",
    ],
    "rgcn_kernels_shared.h": [   # buffer_bytes: the pointer-gather flag turns addressing off
        "if (flags & RGCN_FLAG_POINTER_GATHER) return 0u;",
    ],
}


@pytest.mark.parametrize("name", sorted(BRANCHES))
def test_mirror_branches_match_sources(name):
    src = _src(name)
    missing = [b for b in BRANCHES[name] if b not in src]
    assert not missing, f"{name}: the launcher changed; update tests/kernel_variants.py -- not found: {missing}"


def test_mirror_padded_width_matches_source():
    body = _one("rgcn_common.h", r"inline int padded_width\(int w\) \{ (.*?) \}")
    assert body == "if (w < 1 || w > 128) return 0; return w <= 16 ? 16 : (w <= 32 ? 32 : (w <= 64 ? 64 : 128));"
    assert [K.padded_width(w) for w in (0, 1, 16, 17, 32, 33, 64, 65, 128, 129)] == [0, 16, 16, 32, 32, 64, 64, 128, 128, 0]


def test_mirror_check_plan_forms():
    """the plan headers the mirror enumerates are those check_plan takes and the builder makes"""
    src = _src("rgcn_kernels_shared.h")
    assert "(p->chunk != 64 && p->chunk != 128)" in src
    assert "if ((p->layout == 1 || p->layout == 3) && p->chunk != 128) return RGCN_ERR_PLAN;" in src
    assert "!(p->chunk_rows == 112 && p->chunk == 128)" in src
    assert "(tile % 16) != 0 || p->tile > 32768" in src.replace("p->tile % 16", "tile % 16")
    plan = _src("rgcn_plan.hip")
    assert "if (layout != 0 && layout != 3) return RGCN_ERR_PLAN;" in plan        # 112-row chunks: layouts 0 / 3
    assert {(c, cr if cr else c, lay) for c, cr, lay in K.PLAN_FORMS} == {
        (64, 64, 0), (64, 64, 2), (64, 64, 5), (128, 128, 0), (128, 128, 1), (128, 128, 3), (128, 112, 0), (128, 112, 3)}


def test_mirror_rules_spot_checks():
    """a few launches worked out by hand from the sources"""
    # 64 x 64, chunk 64: 4 slots up to the tile where (tile + 1) * 68 + 4 * 64 * 66 floats pass 40960
    assert K.run_tile(64, 64, 352, 64, 64, 0, 0, True, 8) == ("tile", 64, 64, 4, True, 64, False)
    assert K.run_tile(64, 64, 368, 64, 64, 0, 0, True, 7) == ("tile", 64, 64, 3, True, 64, False)
    assert K.run_tile(100, 13, 16, 64, 64, 0, 0, True, 1) == ("tile", 128, 16, 2, True, 64, False)
    assert K.run_tile(100, 13, 16, 128, 128, 0, 0, True, 1) == K.err(K.ERR_LDS)
    assert K.run_tile(64, 64, 224, 128, 128, 0, K.FLAG_SPLIT_PRODUCERS, True, 12) == ("tile3p", 8, 0, False)
    assert K.run_tile(64, 64, 240, 128, 128, 0, K.FLAG_SPLIT_PRODUCERS, True, 12)[0] == "tile"      # falls through
    assert K.run_tile(64, 64, 240, 128, 128, 3, K.FLAG_SPLIT_PRODUCERS, True, 12) == K.err(K.ERR_LDS)
    assert K.run_tile(64, 64, 272, 128, 112, 3, K.FLAG_SPLIT_PRODUCERS, True, 12) == ("tile3p", 7, 3, False)
    assert K.run_tile(64, 64, 224, 128, 128, 3, K.FLAG_SPLIT_PRODUCERS | K.FLAG_POINTER_GATHER, True, 1) == K.err(K.ERR_PLAN)
    assert K.run_tile(64, 64, 16, 64, 64, 2, 0, True, 1) == K.err(K.ERR_PLAN)
    assert [K.tiles_per_workgroup(n) for n in (1, 256, 257, 4096, 4097, 4353, 28410)] == [1, 1, 2, 16, 1, 9, 16]
    assert K.bwd_dw(64, 64, 64, 64, 64, 0, 0, True, 1, K.DW_DIRECT_MIN_UNITS) == ("dw_direct", 4)
    assert K.bwd_dw(64, 64, 64, 64, 64, 0, K.FLAG_DW_RING, True, 1, K.DW_DIRECT_MIN_UNITS) == ("dw_wide", 64, 64, 4, True, 4, 4)
    assert K.bwd_dw(128, 128, 64, 64, 64, 2, 0, False, 1) == ("dw", 128, 128, 2, False, 4)
    assert K.bwd_dw(64, 64, 64, 64, 64, 2, K.FLAG_DW_ROOT_ONLY, True, 1) == K.err(K.ERR_PLAN)
    assert K.bwd_dw_tiles(64, 64, 320, 64, 64, 5, 0, False, 1) == K.err(K.ERR_ADDRESS)
    assert [K.segsum_g(w) for w in (1, 16, 17, 32, 33, 64, 65, 128)] == [4, 4, 8, 8, 16, 16, 32, 32]
    assert K.root_units(257, 3, 128, 128, 112) == 2 * (2 + 1) + 1


def test_reachable_set_sizes():
    r = K.reachable()
    sizes = {k: len(v) for k, v in r.items()}
    print("reachable tuples per launcher:", sizes)
    assert sizes == {"tile": 127, "tile3p": 10, "tpw": 16, "dw": 33, "dw_root_only": 3, "dw_tiles": 4, "ep": 17, "segsum": 4}


def test_gpu_cases_close_the_reachable_set():
    """every reachable tuple is the target of a case of tests/test_gpu_kernel_variants.py, and every target is reachable"""
    reach = set().union(*K.reachable().values())
    targeted = {}
    for case in G.CASES:
        for t in G.case_targets(case):
            assert t[0] != "err", (G.case_id(case), t)
            assert t in reach, (G.case_id(case), t)
            targeted.setdefault(t, []).append(G.case_id(case))
    unreached = sorted(reach - set(targeted), key=str)
    assert not unreached, f"{len(unreached)} reachable instantiations without a case: {unreached[:20]}"


def test_gpu_case_table_shapes():
    """the root-only cases cover every last-tile row count for every chunk form; the multi-tile cases leave short walks"""
    roots = {(c[5], c[1] - 2 * c[4]) for c in G.CASES if c[0] == "root"}
    assert roots == {(ch, m) for ch in (64, 128, 112) for m in G.ROOT_M}
    assert all(c[4] == 128 and 0 < c[1] - 2 * c[4] <= c[4] for c in G.CASES if c[0] == "root")
    seen = set()
    for c in G.CASES:
        if c[0] == "ring" and c[4] == 16:
            nt = -(-c[1] // 16)
            t = K.tiles_per_workgroup(nt) if c[7] != K.FLAG_SPLIT_PRODUCERS or nt >= K.P3_MULTI_MIN_TILES else 1
            assert t > 1 and nt % t != 0 and c[1] % 16 != 0, G.case_id(c)
            seen.add(t)
    assert seen >= set(range(2, 17))
    assert len(G.CASES) == len({G.case_id(c) for c in G.CASES})


@pytest.mark.parametrize("n", [257, 2500, 69643])
def test_gpu_case_graphs(n):
    """dead relation, duplicate triples, self loops, one hub, and windows of 16 k - 8 distinct destinations inside one tile"""
    ei, et = G.make_graph(n)
    assert int(ei.max()) < n and int(et.max()) < G.NUM_REL - 1
    assert bool((ei[0] == ei[1]).any())
    trip = ei[0] * (n * G.NUM_REL) + ei[1] * G.NUM_REL + et
    assert trip.unique().numel() < trip.numel()
    assert int(ei[1].bincount().max()) >= 300
    starts = G.window_starts(n)
    assert len(starts) == min(8, len(starts)) and starts
    if n >= 2500:
        assert len(starts) == 8
