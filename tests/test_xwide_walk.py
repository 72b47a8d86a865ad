"""tests/xwide_walk.py against csrc/rgcn_xwide.hip (its mirrored constants and host rules), and the case tables of
tests/test_gpu_xwide_edges.py against the emulator on the torch builder's plans: every GPU case has the structure it is named
for.  No GPU needed (test_gpu_plan_build.py holds the device builder equal to the torch one)."""
import ctypes
import os
import re

import pytest

from tests import test_gpu_xwide_edges as G
from tests import xwide_walk as A

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scaling_rgcn_training_amd", "csrc")


def _src():
    with open(os.path.join(CSRC, "rgcn_xwide.hip")) as f:
        return re.sub(r"\s+", " ", f.read())


def _one(pattern):
    m = re.findall(pattern, _src())
    assert len(m) == 1, f"rgcn_xwide.hip: {pattern!r} matched {len(m)} times -- the source changed; update tests/xwide_walk.py"
    return m[0]


def test_mirror_constants_match_the_source():
    assert int(_one(r"constexpr int kXwKS = (\d+);")) == A.KS
    assert int(_one(r"constexpr int kXwDwB = (\d+);")) == A.DW_B
    assert int(_one(r"constexpr int kXwDwWorkgroups = (\d+);")) == A.DW_WORKGROUPS
    assert int(_one(r"constexpr int kXwBiasRows = (\d+);")) == A.BIAS_ROWS
    assert int(_one(r"constexpr int kXwMaxRT = (\d+);")) == 8
    assert _one(r"int xw_nb\(int n\) \{ return ([^;]+); \}") == "n <= 64 ? 64 : 128"
    assert [A.xw_nb(n) for n in (1, 64, 65, 512)] == [64, 64, 128, 128]
    assert _one(r"int dw_shape\(int din, int dout\) \{ return ([^;]+); \}") == "din <= 64 && dout > 64 ? 1 : (dout <= 64 && din > 64 ? 2 : 0)"
    assert len(re.findall(r"const int bm = shape == 1 \? 64 : \(shape == 2 \? 256 : kXwDwB\), bn = shape == 1 \? 256 : \(shape == 2 \? 64 : kXwDwB\);",
                          _src())) == 2
    assert _one(r"const int want = ([^;]+);") == "kXwDwWorkgroups / blocks"
    assert _one(r"return std::max\(1, std::min\(p->n_units, want\)\);") is not None
    assert _one(r"piece_start\(long p, long n_units, long pieces\) \{ return ([^;]+); \}") == "p * n_units / pieces"
    assert _one(r"int bias_blocks\(const rgcn_plan_t\* p\) \{ return ([^;]+); \}") == "std::min(1024, (p->n_owned + kXwBiasRows - 1) / kXwBiasRows)"
    assert _one(r"w\.bias = ([^;]+);") == "align256((size_t)dw_pieces(p, din, dout) * 2 * din * dout * 4)"
    assert _one(r"w\.total = ([^;]+);") == "w.bias + align256((size_t)bias_blocks(p) * dout * 4)"
    assert _one(r"a\.upc = ([^;]+);") == "plan->chunk / 64"
    assert [(A.dw_shape(a, b), A.dw_block(a, b), A.dw_blocks(a, b)) for a, b in ((64, 64), (64, 65), (65, 64), (512, 512), (16, 512), (300, 300))] == \
        [(0, (128, 128), 1), (1, (64, 256), 1), (2, (256, 64), 1), (0, (128, 128), 16), (1, (64, 256), 2), (0, (128, 128), 9)]


@pytest.mark.parametrize("key,din,dout", [c[:3] for c in G.DW_CASES] + [(G.FAT[64, 128], a, b) for a, b in G.WIDTH_CASES])
def test_workspace_bytes_match_the_library(key, din, dout):
    """both align256 terms of the emulator against the library's own answer on a plan of these sizes (a host-side query)"""
    from scaling_rgcn_training_amd import _lib
    p = G.cpu_plans(key).fwd
    dummy = (ctypes.c_int32 * 16)()
    d = ctypes.addressof(dummy)
    ps = _lib.RgcnPlanStruct(p.n_nodes, p.n_owned, p.num_relations, p.tile, p.n_tiles, p.n_chunks, p.chunk, p.n_units, 0, p.chunk_rows,
                             d, d, d, d, d, d, d, d, d, d, None)
    need = _lib.load().rgcn_xwide_bwd_dw_workspace_bytes(ctypes.byref(ps), din, dout)
    assert need == A.workspace_bytes(p.n_units, p.n_owned, din, dout) > 0
    if 8 * din * dout >= 256:
        assert A.pieces_from_workspace(need, p.n_owned, din, dout) == A.dw_pieces(p.n_units, din, dout)


@pytest.mark.parametrize("key,din,dout,paths", G.DW_CASES, ids=lambda v: v[0] + "-%d-%d" % v[1:3] if isinstance(v, tuple) else None)
def test_dw_cases_take_the_store_paths_they_are_named_for(key, din, dout, paths):
    G.assert_dw_case(G.cpu_plans(key), key, din, dout, paths)


def test_dw_cases_cover_the_kernel():
    G.dw_coverage([(key, A.piece_paths(G.cpu_plans(key).fwd, din, dout)) for key, din, dout, _ in G.DW_CASES])
    assert all(c[:3] in [d[:3] for d in G.DW_CASES] for c in G.NULL_CASES)


def test_the_many_graph_is_what_it_is_named_for():
    ei, et, n, r = G.graph("MANY")
    assert (n, r, et.numel()) == (256, 150, 1500) and not {70, 71, r - 1} & set(et.tolist())
    assert int((ei[0] == ei[1]).sum()) >= 20                                              # self loops
    triples = set()
    dup = sum((t in triples) or triples.add(t) or False for t in zip(ei[0].tolist(), ei[1].tolist(), et.tolist()))
    assert dup >= 30                                                                      # repeated triples
    p = G.cpu_plans(G.MANY).fwd
    assert (p.tile, p.chunk, p.n_tiles) == (192, 64, 2) and p.n_owned % p.tile != 0
    # at 512 x 512: 32 pieces, most relations stored from the middle of a piece
    s = A.piece_paths(p, 512, 512)
    paths = list(s["stores"].values())
    assert s["pieces"] == 32 and paths.count("direct_middle") > 2 * (paths.count("slab0") + paths.count("slab1"))


@pytest.mark.parametrize("geom", list(G.FAT), ids=lambda g: "%d-%d" % g)
def test_fat_geometries(geom):
    p = G.cpu_plans(G.FAT[geom])
    assert (p.fwd.tile, p.fwd.chunk, p.bwd.tile, p.bwd.chunk) == geom * 2
    G.assert_rt_case(p, geom)


def test_fat_covers_row_tile_counts_1_to_8_and_the_hub():
    ei, et, n, r = G.graph("FAT")
    assert (n, r) == (500, 3) and int(((ei[1] == 5) & (et == 1)).sum()) >= G.HUB
    seen = set()
    for geom in G.FAT:
        p = G.cpu_plans(G.FAT[geom])
        seen |= set(A.tile_walk(p.fwd, 1)["rt"]) | set(A.tile_walk(p.bwd, 1)["rt"])
    assert seen == set(range(1, 9))
    assert {g[0] for g in G.FAT} == {16, 32, 64, 192} and {g[1] for g in G.FAT} == {64, 128}
    assert all((FAT_geom, a, b) in G.RT_CASES for FAT_geom in G.FAT for a, b in ((129, 65), (36, 257)))


@pytest.mark.parametrize("din,dout", list(G.WIDTH_CASES), ids=lambda v: str(v))
def test_width_cases(din, dout):
    assert G.width_walk(din, dout) == G.WIDTH_CASES[(din, dout)]


def test_width_cases_cover_the_edges():
    fwd_dx = [w for pair in G.WIDTH_CASES.values() for w in pair]
    assert {1, 2, 5, 8} <= {ks for ns, ks, *_ in fwd_dx if ns >= 1}
    assert any(ns >= 2 and ks == 1 for ns, ks, *_ in fwd_dx)                       # one k-step in a second slice
    assert {(nb, ncb, live) for _, _, nb, ncb, live in fwd_dx} >= {(64, 1, 1), (64, 1, 4), (128, 1, 3), (128, 2, 1), (128, 3, 1),
                                                                   (128, 4, 1), (128, 4, 4)}
    assert A.dw_shape(40, 48) == 0 and {A.dw_shape(a, b) for a, b in G.WIDTH_CASES} == {0, 1, 2}


def test_part_and_tiny_plans():
    p = G.cpu_plans(G.PART)
    assert (p.fwd.node_begin, p.fwd.n_owned, p.bwd.node_begin, p.bwd.n_owned, p.fwd.n_nodes) == (192, 308, 192, 308, 500)
    assert A.tile_walk(p.fwd, 1)["last_rows"] == 116 and A.tile_walk(p.fwd, 1)["tiles"] == 2
    for key, units in ((G.TINY40, 4), (G.TINY1, 2)):
        q = G.cpu_plans(key).fwd
        assert q.n_units == units and q.n_tiles == 1 and q.n_owned < q.tile
    assert [c[:3] for c in G.CONTRACT_CASES] == [(k, a, b) for k in (G.FAT[192, 128], G.PART) for a, b in ((129, 65), (36, 257))]


def test_the_layers_own_plan_stores_from_the_middle_of_a_piece():
    """RGCNConv(300, 300, 150, wide=True) on MANY's 256 nodes: rgcn_xwide_geometry answers tile 16, chunk 64"""
    from scaling_rgcn_training_amd import _lib, plan as P
    assert _lib.xwide_geometry(256, 300, 300) == G.LAYER_GEOMETRY
    ei, et, n, r = G.graph("MANY")
    p = P.build_graph_plans_torch(ei, et, n, r, G.LAYER_GEOMETRY[0], chunk=G.LAYER_GEOMETRY[1])
    s = A.piece_paths(p.fwd, 300, 300)
    assert "direct_middle" in s["paths"] and set(s["empty"]) == {70, 71, r - 1}
