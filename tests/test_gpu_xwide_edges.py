"""The wide-layer kernels (csrc/rgcn_xwide.hip, rgcn_xwide_*) at the sizes where their structure changes, through the raw entry
points on sentinel-guarded operands: every store path of xw_dw_kernel / xw_dw_reduce (direct first / middle / last, slab 0 / 1,
relations spanning three and more pieces from either slab slot, relations without units), 128-slot chunks (row-tile counts 5..8
in the forward / dX walk, two units per chunk in the d_W walk), tiles 16 / 32 / 64 / 192 with a ragged last tile, the width
edges of the 32-column K-slice and the 64 / 128-column blocks, NULL outputs, the workspace at exactly its queried size and the
memory contract of include/rgcn_mi355x.h (strides, pad columns, relu_of, a plan over a node sub-range).

Every case asserts, through tests/xwide_walk.py on the device plan, the structure it is named for (tests/test_xwide_walk.py
asserts the same on the torch builder's plans, without a GPU), runs forward, dX and d_W on one (din, dout), compares with the
float64 segment oracle under oracle/tolerance.py's defaults and demands bit-equal results from a second run.
Needs an MI355X: ``pytest -m gpu``."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import rgcn_oracle as O
from oracle.tolerance import abs_condition, assert_close, cpu32_reference
from tests import xwide_walk as A
from tests.test_gpu_abi_contract import G_OUT, SENT, Flat, Guarded, Workspace, r4

pytestmark = pytest.mark.gpu

OK, ERR_WORKSPACE = 0, -6
NAN_BITS = 0x7FC00000
PART_LO = 192
HUB = 700


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    _lib().load()
    yield torch.device("cuda:0")
    oracle.cache_clear()          # (MANY at 512 x 512 holds four [150, 512, 512] float64 tensors)
    dev_plans.cache_clear()


def _lib():
    from scaling_rgcn_training_amd import _lib as L
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- the graphs -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def graph(name):
    """(edge_index, edge_type, nodes, relations)"""
    if name == "MANY":      # 150 thin relations: about ten edges each, two (tile 192, relation) groups of one unit
        n, r = 256, 150
        ei, et = O.synthetic_graph(n, 1500, r, seed=21)
        et[(et == 70) | (et == 71)] = 69          # two empty relations in the middle of the range
        et[et == r - 1] = r - 2                   # and the last one
        ei[:, 10:40], et[10:40] = ei[:, 50:80], et[50:80]      # duplicate triples
        ei[1, 200:220] = ei[0, 200:220]           # self loops
    elif name == "FAT":     # three fat relations and a hub: groups of many chunks
        n, r = 500, 3
        ei, et = O.synthetic_graph(n, 6000, r, seed=22)
        g = torch.Generator().manual_seed(23)
        hub = torch.stack([torch.randint(0, n, (HUB,), generator=g), torch.full((HUB,), 5)])
        ei, et = torch.cat([ei, hub], 1), torch.cat([et, torch.ones(HUB, dtype=torch.int64)])
    elif name == "TINY40":
        n, r = 40, 3
        ei, et = O.synthetic_graph(n, 60, r, seed=24)
    elif name == "TINY1":   # one node, one self loop; relation 1 without edges
        n, r = 1, 2
        ei, et = torch.zeros(2, 1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
    else:
        raise KeyError(name)
    return ei.contiguous(), et.contiguous(), n, r


def rng(key):
    name, _, _, part = key
    n = graph(name)[2]
    return (PART_LO, n) if part else (0, n)


@functools.lru_cache(None)
def cpu_plans(key):
    """key = (graph, tile, chunk, part): part = the plans of the owned rows [192, n) only"""
    from scaling_rgcn_training_amd import plan as P
    name, tile, chunk, _ = key
    ei, et, n, r = graph(name)
    return P.build_graph_plans_torch(ei, et, n, r, tile, fwd_range=rng(key), bwd_range=rng(key), chunk=chunk, split=False)


@functools.lru_cache(None)
def dev_plans(key):
    from scaling_rgcn_training_amd import plan as P
    name, tile, chunk, _ = key
    ei, et, n, r = graph(name)
    d = torch.device("cuda:0")
    return P.build_graph_plans_device(ei.to(d), et.to(d), n, r, tile, fwd_range=rng(key), bwd_range=rng(key), chunk=chunk,
                                      split=False)


MANY = ("MANY", 192, 64, False)
FAT = {(t, c): ("FAT", t, c, False) for t, c in ((192, 128), (64, 128), (32, 64), (16, 128))}
PART = ("FAT", 192, 128, True)
TINY40 = ("TINY40", 192, 128, False)
TINY1 = ("TINY1", 16, 64, False)


# ---- the structure every case is named for (asserted on the torch plans by test_xwide_walk.py, on the device plans here) -----------
# d_W store paths: key, din, dout -> the paths that occur
F, M, L_, S0, S1 = A.PATHS
DW_CASES = [
    (MANY, 300, 300, {F, M, L_, S0, S1}),
    (MANY, 512, 512, {F, M, L_, S0, S1}),
    (MANY, 16, 512, {F, L_, S0, S1}),
    (MANY, 512, 16, {F, L_, S0, S1}),
    (MANY, 40, 48, {L_, S0}),
    (FAT[192, 128], 300, 300, {S0, S1}),
    (FAT[192, 128], 33, 65, {S0}),
    (TINY40, 300, 300, {L_}),
    (TINY40, 129, 129, {L_}),
    (TINY1, 300, 300, {L_}),
    (TINY1, 129, 129, {L_}),
]
NULL_CASES = [(MANY, 300, 300), (FAT[192, 128], 33, 65)]
# row tiles per chunk (chunk_cnt / 16: the MFMA walk's switch) that occur in FAT's forward and transposed plan at every geometry
RT = {(192, 128): ({2, 3, 4, 6, 7, 8}, {1, 3, 4, 5, 6, 7, 8}), (64, 128): ({1, 2, 3, 4, 5, 6, 7, 8}, {1, 2, 3, 4, 5, 7, 8}),
      (32, 64): ({1, 2, 3, 4}, {1, 2, 3, 4}), (16, 128): ({1, 2, 3, 4, 5, 6, 8}, {1, 2, 4, 5, 6})}
RT_CASES = [(g, a, b) for g in FAT for a, b in ((129, 65), (36, 257))]
# width edges on FAT (tile 64, chunk 128): (din, dout) -> forward (K-slices, last k-steps, NB, column blocks, live waves of the last
# block), dX the same with the sides swapped
WIDTH_CASES = {
    (1, 1): ((1, 1, 64, 1, 1), (1, 1, 64, 1, 1)),
    (31, 15): ((1, 8, 64, 1, 1), (1, 4, 64, 1, 2)),
    (32, 16): ((1, 8, 64, 1, 1), (1, 4, 64, 1, 2)),
    (33, 17): ((2, 1, 64, 1, 2), (1, 5, 64, 1, 3)),
    (36, 63): ((2, 1, 64, 1, 4), (2, 8, 64, 1, 3)),
    (37, 64): ((2, 2, 64, 1, 4), (2, 8, 64, 1, 3)),
    (64, 65): ((2, 8, 128, 1, 3), (3, 1, 64, 1, 4)),
    (65, 127): ((3, 1, 128, 1, 4), (4, 8, 128, 1, 3)),
    (128, 129): ((4, 8, 128, 2, 1), (5, 1, 128, 1, 4)),
    (129, 128): ((5, 1, 128, 1, 4), (4, 8, 128, 2, 1)),
    (257, 33): ((9, 1, 64, 1, 3), (2, 1, 128, 3, 1)),
    (385, 5): ((13, 1, 64, 1, 1), (1, 2, 128, 4, 1)),
    (511, 512): ((16, 8, 128, 4, 4), (16, 8, 128, 4, 4)),
    (512, 511): ((16, 8, 128, 4, 4), (16, 8, 128, 4, 4)),
}
CONTRACT_CASES = [(k, a, b) for k in (FAT[192, 128], PART) for a, b in ((129, 65), (36, 257))]
# through the layer: RGCNConv(300, 300, 150, wide=True) on MANY's edges picks tile 16 for 256 nodes
LAYER_GEOMETRY = (16, 64)


def assert_dw_case(plans, key, din, dout, paths):
    s = A.piece_paths(plans.fwd, din, dout)
    assert s["paths"] == set(paths), (key, din, dout, sorted(s["paths"]))
    nu = plans.fwd.n_units
    assert s["pieces"] == min(nu, A.DW_WORKGROUPS // A.dw_blocks(din, dout))
    name = key[0]
    r = graph(name)[3]
    if name == "MANY":
        assert set(s["empty"]) == {70, 71, r - 1}
    if name == "TINY1":
        assert s["empty"] == [1]
    if name.startswith("TINY"):
        assert s["pieces"] == nu and plans.fwd.n_owned < plans.fwd.tile and plans.fwd.n_tiles == 1
    if (din, dout) == (40, 48):     # shape 0 with both sides at most 64: one 128 x 128 block, pieces capped by the units or 512
        assert A.dw_shape(din, dout) == 0 and A.dw_blocks(din, dout) == 1 and s["pieces"] == min(nu, 512)
    return s


def dw_coverage(all_s):
    """over the d_W cases together: all five paths; a relation that starts in slab slot 1 and one that starts in slot 0, each
    spanning at least three pieces; a relation of exactly one unit; the root relation stored directly and through the slabs"""
    paths, spans, one_unit, root = set(), set(), False, set()
    for key, s in all_s:
        paths |= s["paths"]
        spans |= {slot for n, slot in s["span"].values() if n >= 3}
        one_unit |= 1 in s["units"].values()
        rr = graph(key[0])[3]
        root |= {s["stores"][k][:-1].split("_")[0] for k in s["stores"] if k[1] == rr}
    assert paths == set(A.PATHS), paths
    assert spans == {0, 1}, spans
    assert one_unit and root == {"direct", "slab"}, (one_unit, root)


def assert_rt_case(plans, geom):
    tile, chunk = geom
    f, b = A.tile_walk(plans.fwd, 1), A.tile_walk(plans.bwd, 1)
    assert (set(f["rt"]), set(b["rt"])) == RT[geom], (geom, sorted(f["rt"]), sorted(b["rt"]))
    assert 0 < f["last_rows"] < tile and 0 < b["last_rows"] < tile          # a ragged last tile
    assert f["tiles"] == b["tiles"] == -(-500 // tile) > 1
    if chunk == 128:
        assert max(f["rt"]) > 4 and max(b["rt"]) > 4
        assert A.short_second_halves(plans.fwd) > 0       # upc == 2 units whose second half holds fewer than 64 used slots
        assert_hub(plans)
    else:
        assert max(f["rt"]) <= 4 and max(b["rt"]) <= 4 and A.short_second_halves(plans.fwd) == 0


def assert_hub(plans):
    """node 5 gathers 700 edges of relation 1: its (tile 0, relation 1) group spans at least three 128-slot chunks"""
    assert A.tile_walk(plans.fwd, 1)["groups"][(0, 1)] >= 3


def width_walk(din, dout):
    return (A.k_slices(din) + A.col_blocks(dout), A.k_slices(dout) + A.col_blocks(din))


# ---- float64 references, once per (graph, widths) ---------------------------------------------------------------------------------
@functools.lru_cache(None)
def oracle(name, din, dout, part=False):
    ei, et, n, r = graph(name)
    w, root, _ = O.synthetic_params(r, din, dout, seed=din * 7 + dout)
    g = torch.Generator().manual_seed(din * 131 + dout)
    bias = torch.randn(dout, generator=g) * 0.1
    x = torch.randn(n, din, generator=g)
    dg = torch.randn(n, dout, generator=g)

    def ev(dgv):
        a = [t.numpy() for t in (x, ei, et, w, root, bias, dgv)]
        ref, gr = O.rgcn_conv_segments(*a)
        c_out, c = abs_condition(*a)
        o32, g32 = cpu32_reference(*a)
        return ref, gr, c_out, c, o32, g32

    ref, gr, c_out, c, o32, g32 = ev(dg)
    if part:        # out and dX: the owned rows of the full result; the weight gradients: from the edges into the owned rows
        own = slice(PART_LO, n)
        dgm = dg.clone()
        dgm[:PART_LO] = 0
        _, gm, _, cm, _, g32m = ev(dgm)
        gr, c, g32 = dict(gm, x=gr["x"][own]), dict(cm, x=c["x"][own]), dict(g32m, x=g32["x"][own])
        ref, c_out, o32 = ref[own], c_out[own], o32[own]
    return dict(x=x, dg=dg, w=w, root=root, bias=bias, ref=ref, gr=gr, c_out=c_out, c=c, o32=o32, g32=g32)


def _act(z, act):
    return np.maximum(z, 0) if act == 1 else (1 / (1 + np.exp(-z)) if act == 2 else z)


def _ld(w, k, padded):
    """row stride of operand k: round4(w), or a multiple of 4 beyond it that no other operand of the call has"""
    return r4(w) + (4 * k if padded else 0)


def _filled(values, dev):
    f = Flat(values.numel(), dev)
    f.t.copy_(values.reshape(-1))
    return f, f.buf.clone()


def run_layer(dev, key, din, dout, padded=False, want=(True, True, True), act=0, relu=None, parts=("fwd", "dx", "dw"),
              ws_short=0):
    """rgcn_xwide_fwd / _bwd_dx / _bwd_dw on guarded operands -> the results (out, dx: float64 arrays of the written rows;
    weight, root, bias: tensors).  Asserts the statuses, the footprints, the untouched inputs and the workspace's tail."""
    L = _lib()
    lib = L.load()
    name, tile, chunk, part = key
    _, _, n, r = graph(name)
    gp = dev_plans(key)
    o = oracle(name, din, dout, part)
    lo = rng(key)[0]
    own = n - lo
    fp, bp = L.plan_struct(gp.fwd), L.plan_struct(gp.bwd)
    assert (fp.n_owned, bp.n_owned, fp.tile, fp.chunk, fp.layout) == (own, own, tile, chunk, 0)
    tag = f"[{name} {tile}/{chunk}{' part' if part else ''} {din}x{dout}{' padded' if padded else ''}]"
    res = {}
    x = Guarded(n, _ld(din, 1, padded), dev).fill(o["x"])
    op = torch.cat([o["w"], o["root"][None]])
    if "fwd" in parts:
        wf, wsnap = _filled(op, dev)
        bias, bsnap = _filled(o["bias"], dev)
        out = Guarded(own, _ld(dout, 2, padded), dev, g1=G_OUT)
        st = lib.rgcn_xwide_fwd(C.byref(fp), x.ptr, x.ld, din, wf.ptr, bias.ptr, out.ptr, out.ld, dout, act, _stream())
        torch.cuda.synchronize()
        assert st == OK, (tag, st)
        x.unchanged("rgcn_xwide_fwd x " + tag)
        assert torch.equal(wf.buf, wsnap) and torch.equal(bias.buf, bsnap), f"{tag}: rgcn_xwide_fwd wrote an input"
        res["out"] = out.out(dout, "rgcn_xwide_fwd " + tag)
        res["out_t"] = out.mat[:, :dout].clone()
    if "dx" in parts:
        g = Guarded(n, _ld(dout, 3, padded), dev).fill(o["dg"])
        wt, wsnap = _filled(op.transpose(1, 2).contiguous(), dev)
        dx = Guarded(own, _ld(din, 4, padded), dev, g1=G_OUT)
        rel = None if relu is None else Guarded(own, _ld(din, 5, padded), dev).fill(relu)
        st = lib.rgcn_xwide_bwd_dx(C.byref(bp), g.ptr, g.ld, dout, wt.ptr, dx.ptr, dx.ld, din, None if rel is None else rel.ptr,
                                   0 if rel is None else rel.ld, _stream())
        torch.cuda.synchronize()
        assert st == OK, (tag, st)
        g.unchanged("rgcn_xwide_bwd_dx g " + tag)
        if rel is not None:
            rel.unchanged("rgcn_xwide_bwd_dx relu_of " + tag)
        assert torch.equal(wt.buf, wsnap), f"{tag}: rgcn_xwide_bwd_dx wrote its weights"
        res["dx"] = dx.out(din, "rgcn_xwide_bwd_dx " + tag)
    if "dw" in parts:
        go = Guarded(own, _ld(dout, 6, padded), dev).fill(o["dg"][lo:])
        outs = [Flat(k, dev) for k in (r * din * dout, din * dout, dout)]
        need = lib.rgcn_xwide_bwd_dw_workspace_bytes(C.byref(fp), din, dout)
        assert need == A.workspace_bytes(gp.fwd.n_units, own, din, dout) and need % 256 == 0
        ws = Workspace(need, dev)
        ws.buf[:need].view(torch.int32).fill_(NAN_BITS)      # a slab read without having been written poisons the result
        st = lib.rgcn_xwide_bwd_dw(C.byref(fp), x.ptr, x.ld, din, go.ptr, go.ld, dout, ws.ptr, need - ws_short,
                                   *[f.ptr if w_ else None for f, w_ in zip(outs, want)], _stream())
        torch.cuda.synchronize()
        x.unchanged("rgcn_xwide_bwd_dw x " + tag)
        go.unchanged("rgcn_xwide_bwd_dw g " + tag)
        ws.check("rgcn_xwide_bwd_dw workspace " + tag)
        res["need"] = need
        if ws_short:
            assert st == ERR_WORKSPACE, (tag, st)
            assert all(bool((f.buf == SENT).all()) for f in outs), f"{tag}: a refused call wrote an output"
            assert bool((ws.buf[:need].view(torch.int32) == NAN_BITS).all()), f"{tag}: a refused call wrote its workspace"
            return res
        assert st == OK, (tag, st)
        for f, w_, nm, shape in zip(outs, want, ("weight", "root", "bias"), ((r, din, dout), (din, dout), (dout,))):
            if w_:
                res[nm] = f.out(f"d_{nm} {tag}").view(shape)
            else:
                assert bool((f.buf == SENT).all()), f"{tag}: d_{nm} was not passed and was written"
    return res


def check(res, key, din, dout, act=0, mask=None):
    """every result against float64 under oracle/tolerance.py's defaults (a NaN -- a sentinel that was read -- fails)"""
    name, tile, chunk, part = key
    o = oracle(name, din, dout, part)
    tag = f"{name} {tile}/{chunk}{' part' if part else ''} {din}x{dout}"
    if "out" in res:
        assert_close(res["out"], _act(o["ref"], act), o["c_out"], f"xwide edges out {tag}", cpu32=_act(o["o32"].astype(np.float32), act))
    if "dx" in res:
        ref, cond, c32 = o["gr"]["x"], o["c"]["x"], o["g32"]["x"]
        if mask is not None:
            ref, cond, c32 = ref * mask, cond * mask, c32 * mask
        assert_close(res["dx"], ref, cond, f"xwide edges d_x {tag}", cpu32=c32)
    for nm in ("weight", "root", "bias"):
        if nm in res:
            assert_close(res[nm].double().cpu().numpy(), o["gr"][nm], o["c"][nm], f"xwide edges d_{nm} {tag}", cpu32=o["g32"][nm])


def same_bits(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k].view(np.int64), b[k].view(np.int64)), f"{tag}: {k} differs between two runs"
        elif isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{tag}: {k} differs between two runs"


def run_twice_and_check(dev, key, din, dout, **kw):
    res = run_layer(dev, key, din, dout, **kw)
    check(res, key, din, dout)
    same_bits(res, run_layer(dev, key, din, dout, **kw), f"{key} {din}x{dout}")
    return res


# ---- 1. d_W store paths -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,din,dout,paths", DW_CASES, ids=lambda v: v[0] + "-%d-%d" % v[1:3] if isinstance(v, tuple) else None)
def test_dw_store_paths(dev, key, din, dout, paths):
    gp = dev_plans(key)
    s = assert_dw_case(gp, key, din, dout, paths)
    res = run_twice_and_check(dev, key, din, dout)
    assert A.pieces_from_workspace(res["need"], gp.fwd.n_owned, din, dout) == s["pieces"]
    r = graph(key[0])[3]
    for e in s["empty"]:
        assert e < r and bool((res["weight"][e].view(torch.int32) == 0).all()), f"relation {e} has no edges: d_weight must be +0.0"


def test_dw_store_paths_cover_the_kernel(dev):
    """over the cases above, on the device plans (the same assertion on the torch plans: test_xwide_walk.py)"""
    dw_coverage([(key, A.piece_paths(dev_plans(key).fwd, din, dout)) for key, din, dout, _ in DW_CASES])


# ---- 2. NULL outputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,din,dout", NULL_CASES, ids=lambda v: v[0] if isinstance(v, tuple) else str(v))
def test_null_outputs(dev, key, din, dout):
    """(d_weight, d_root, d_bias) present or NULL in all seven combinations: every present output bit-equal to the all-present
    run's (checked against float64), every absent one an untouched sentinel buffer that is not passed"""
    assert_dw_case(dev_plans(key), key, din, dout, dict((c[:3], c[3]) for c in DW_CASES)[(key, din, dout)])
    full = run_layer(dev, key, din, dout, parts=("dw",))
    check(full, key, din, dout)
    for bits in range(1, 7):
        want = tuple(bool(bits >> i & 1) for i in range(3))
        res = run_layer(dev, key, din, dout, parts=("dw",), want=want)
        for nm, w_ in zip(("weight", "root", "bias"), want):
            assert (nm in res) == w_
            if w_:
                assert torch.equal(res[nm].view(torch.int32), full[nm].view(torch.int32)), (want, nm)


# ---- 3. workspace -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,din,dout", NULL_CASES + [(FAT[16, 128], 129, 65)], ids=lambda v: v[0] if isinstance(v, tuple) else str(v))
def test_workspace_exact_and_short(dev, key, din, dout):
    """every call of this file has a workspace of exactly the queried bytes, NaN-filled, with a sentinel tail (run_layer); one
    byte less is refused with RGCN_ERR_WORKSPACE before anything is written"""
    res = run_layer(dev, key, din, dout, parts=("dw",), ws_short=1)
    assert set(res) == {"need"}
    check(run_layer(dev, key, din, dout, parts=("dw",)), key, din, dout)


# ---- 4. row-tile counts and tiles -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,din,dout", RT_CASES, ids=lambda v: "%d-%d" % v if isinstance(v, tuple) else str(v))
def test_row_tile_counts_and_tiles(dev, geom, din, dout):
    gp = dev_plans(FAT[geom])
    assert_rt_case(gp, geom)
    run_twice_and_check(dev, FAT[geom], din, dout)


def test_row_tile_counts_cover_1_to_8(dev):
    """over FAT's four geometries, forward and transposed plans: every row-tile count of the MFMA walk's switch"""
    seen = set()
    for geom in FAT:
        gp = dev_plans(FAT[geom])
        seen |= set(A.tile_walk(gp.fwd, 1)["rt"]) | set(A.tile_walk(gp.bwd, 1)["rt"])
    assert seen == set(range(1, 9)), seen


# ---- 5. width edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("din,dout", list(WIDTH_CASES), ids=lambda v: str(v))
def test_width_edges(dev, din, dout):
    """the K-slice count, the last slice's k-steps, the column blocks and the live waves of the last block, forward and dX; the
    d_weight / d_root buffers are exactly [R, din, dout] / [din, dout] floats between sentinels"""
    assert width_walk(din, dout) == WIDTH_CASES[(din, dout)]
    key = FAT[64, 128]
    assert_rt_case(dev_plans(key), (64, 128))
    run_twice_and_check(dev, key, din, dout)


# ---- 6. the memory contract -------------------------------------------------------------------------------------------------------------
def relu_mask(key, din):
    """relu_of: both signs and exact zeros (+0.0 and -0.0 mask like a negative value)"""
    lo, hi = rng(key)
    g = torch.Generator().manual_seed(din + lo)
    m = torch.randn(hi - lo, din, generator=g)
    m[torch.rand(hi - lo, din, generator=g) < 0.2] = 0.0
    m[torch.rand(hi - lo, din, generator=g) < 0.05] = -0.0
    assert bool((m > 0).any()) and bool((m < 0).any()) and bool((m == 0).any())
    return m


@pytest.mark.parametrize("key,din,dout", CONTRACT_CASES, ids=lambda v: ("part" if v[3] else "whole") if isinstance(v, tuple) else str(v))
def test_memory_contract(dev, key, din, dout):
    """every matrix between guard rows at a row stride of its own beyond round4(width): inputs unchanged, sentinels intact, pad
    columns +0.0, values within tolerance (so no sentinel was read); dX under relu_of = the unmasked dX with the mask applied, to
    the bit; the fused ReLU / sigmoid store against torch on the plain result"""
    gp = dev_plans(key)
    assert gp.fwd.n_owned == (308 if key[3] else 500) and gp.fwd.node_begin == (PART_LO if key[3] else 0)
    plain = run_twice_and_check(dev, key, din, dout, padded=True)
    mask = relu_mask(key, din)
    masked = run_layer(dev, key, din, dout, padded=True, relu=mask, parts=("dx",))
    keep = (mask > 0).numpy()
    check(masked, key, din, dout, mask=keep)
    assert np.array_equal(np.where(keep, plain["dx"], 0.0).view(np.int64), masked["dx"].view(np.int64))      # masked: +0.0
    z = plain["out_t"]
    for act in (1, 2):
        got = run_layer(dev, key, din, dout, padded=True, act=act, parts=("fwd",))
        check(got, key, din, dout, act=act)
        if act == 1:
            assert torch.equal(got["out_t"], torch.relu(z))
        else:
            torch.testing.assert_close(got["out_t"], torch.sigmoid(z), rtol=1e-6, atol=1e-7)


# ---- 7. through the layer -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "basis"])
def test_through_the_layer(dev, mode):
    """RGCNConv(300, 300, 150, wide=True) on MANY's edges: the layer's own plan (tile 16) stores relations directly from the
    middle of a piece"""
    from scaling_rgcn_training_amd.plan import _CACHE, cached_graph_plans
    from tests.test_gpu_xwide import _check, _layer, _run
    ei, et, n, r = graph("MANY")
    eid, etd = ei.to(dev), et.to(dev)
    conv = _layer(300, 300, r, mode, "mean", True, seed=7).to(dev)
    assert conv.xwide and _lib().xwide_geometry(n, 300, 300) == LAYER_GEOMETRY
    gen = torch.Generator().manual_seed(17)
    x, g = torch.randn(n, 300, generator=gen), torch.randn(n, 300, generator=gen)
    out, dx, grads = _run(conv, x, eid, etd, g, dev)
    cached = len(_CACHE)
    plans = cached_graph_plans(eid, etd, n, r, LAYER_GEOMETRY[0], "mean", chunk=LAYER_GEOMETRY[1], extra_key=("xwide",))
    assert len(_CACHE) == cached, "not the plan the layer walked"
    s = A.piece_paths(plans.fwd, 300, 300)
    assert "direct_middle" in s["paths"] and set(s["empty"]) == {70, 71, r - 1}
    _check(conv, x, ei, et, g, out, dx, grads, "mean", f"layer on MANY {mode}")
    if mode == "full":
        assert all(bool((grads["weight"][e] == 0).all()) for e in s["empty"])
    out2, dx2, grads2 = _run(conv, x, eid, etd, g, dev)
    assert torch.equal(out, out2) and torch.equal(dx, dx2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
