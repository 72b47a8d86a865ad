"""Every template instantiation the dense forward / dX / dW launchers can pick, run once against the float64 oracle.

tests/kernel_variants.py restates each launcher's run-time choice; tests/test_kernel_variants.py (no GPU) checks that
CASES below targets every tuple of its reachable set and that every case's target is reachable.  Here each case builds
its plans on the device, asserts from the plan itself that the launch reaches the instantiation it targets (the plan's
tile / chunk / layout / tile count under the mirror, the row-tile counts of its chunks, the tiles per workgroup, formed
pairs), then runs the raw ABI wrappers with outputs pre-filled with NaN and compares against ``O.rgcn_conv_segments`` under
both bounds of oracle/tolerance.py.  Every graph has a dead relation, duplicate triples, self loops and one hub.
The row-tile-count (nrt) span is asserted on the single-tile-per-workgroup rgcn_tile3p_kernel cases of layouts 0 and 3 (tiles
224 / 272).  The multi-tile rgcn_tile3p_kernel cases run at tile 16, so their chunks hold one row tile each: a multi-tile walk
of that kernel with several row tiles per chunk would take ~1M nodes (4,096+ tiles of 224) and is not a case here.

Case rows: (kind, n_nodes, din, dout, tile, chunk, layout, flags)
  ring  forward (activation none / relu / sigmoid in rotation), dX (with / without the fused ReLU mask) and relation-major
        d_weight / d_root / d_bias on a tile plan (chunk 112 = 128-slot chunks of at most 112 rows; layout 3: no dW)
  ep    the edge-parallel path: rgcn_ep_transform + rgcn_ep_segment_sum both ways, dW on the dense layout-2 units
  root  RGCN_FLAG_DW_ROOT_ONLY on a tile plan with n_nodes = 2 * tile + m, against fp64 and against the full walk
  dwt   rgcn_bwd_dw_tiles on a layout-0 / layout-5 plan (tile 320, 64-slot chunks)
"""
import numpy as np
import pytest
import torch

from oracle import rgcn_oracle as O
from oracle.tolerance import abs_condition, assert_close, cpu32_reference
from tests import kernel_variants as K

pytestmark = pytest.mark.gpu

PTR, SPLIT, DIRECT = K.FLAG_POINTER_GATHER, K.FLAG_SPLIT_PRODUCERS, K.FLAG_DW_DIRECT
NUM_REL = 6            # relations 0..3 random, 4 the windows' (full chunks of 1..8 row tiles), 5 dead
ROOT_M = (1, 15, 16, 17, 111, 112, 113, 128)       # rows of the last tile of the root-only plans (tile 128)
# tiles per workgroup k = 2..16 of rgcn_tile_kernel at tile 16: the first tile count of each band that leaves the last
# workgroup a short walk, less 5 rows (a short last tile)
TPW_NODES = (4107, 8219, 12299, 16411, 20491, 24587, 28683, 32779, 36875, 40971, 45067, 49163, 53259, 57371, 61451)
P3_MULTI_NODES = 69643     # 4353 tiles of 16: rgcn_tile3p_kernel walks 9 tiles per workgroup, the last workgroup 6

CASES = [
    # ---- rgcn_tile_kernel: every (KP, NP, NBUF, BUF, CH) at the largest tile that gives that ring depth and
    # leaves the dX launch of the same plan a ring that fits (where none does -- 128-slot chunks with a side of 128 -- the dX
    # launch must answer RGCN_ERR_LDS)
    ("ring", 2500, 100, 100, 176, 64, 0, PTR),
    ("ring", 2500, 100, 100, 176, 64, 0, 0),
    ("ring", 2500, 100, 13, 288, 64, 0, PTR),
    ("ring", 2500, 100, 13, 288, 64, 0, 0),
    ("ring", 2500, 100, 32, 272, 64, 0, PTR),
    ("ring", 2500, 100, 32, 272, 64, 0, 0),
    ("ring", 2500, 100, 64, 240, 64, 0, PTR),
    ("ring", 2500, 100, 64, 240, 64, 0, 0),
    ("ring", 2500, 13, 100, 272, 128, 0, PTR),
    ("ring", 2500, 13, 100, 272, 128, 0, 0),
    ("ring", 2500, 13, 100, 256, 128, 0, PTR),
    ("ring", 2500, 13, 100, 256, 128, 0, 0),
    ("ring", 2500, 13, 100, 272, 64, 0, PTR),
    ("ring", 2500, 13, 100, 272, 64, 0, 0),
    ("ring", 2500, 13, 13, 1808, 128, 0, PTR),
    ("ring", 2500, 13, 13, 1920, 64, 0, PTR),
    ("ring", 2500, 13, 13, 1808, 128, 0, 0),
    ("ring", 2500, 13, 13, 1920, 64, 0, 0),
    ("ring", 2500, 13, 13, 1696, 128, 0, PTR),
    ("ring", 2500, 13, 13, 1872, 64, 0, PTR),
    ("ring", 2500, 13, 13, 1696, 128, 0, 0),
    ("ring", 2500, 13, 13, 1872, 64, 0, 0),
    ("ring", 2500, 13, 13, 1808, 64, 0, PTR),
    ("ring", 2500, 13, 13, 1808, 64, 0, 0),
    ("ring", 2500, 13, 32, 1008, 128, 0, PTR),
    ("ring", 2500, 13, 32, 1072, 64, 0, PTR),
    ("ring", 2500, 13, 32, 1008, 128, 0, 0),
    ("ring", 2500, 13, 32, 1072, 64, 0, 0),
    ("ring", 2500, 13, 32, 944, 128, 0, PTR),
    ("ring", 2500, 13, 32, 1040, 64, 0, PTR),
    ("ring", 2500, 13, 32, 944, 128, 0, 0),
    ("ring", 2500, 13, 32, 1040, 64, 0, 0),
    ("ring", 2500, 13, 32, 1008, 64, 0, PTR),
    ("ring", 2500, 13, 32, 1008, 64, 0, 0),
    ("ring", 2500, 13, 64, 528, 128, 0, PTR),
    ("ring", 2500, 13, 64, 560, 64, 0, PTR),
    ("ring", 2500, 13, 64, 528, 128, 0, 0),
    ("ring", 2500, 13, 64, 560, 64, 0, 0),
    ("ring", 2500, 13, 64, 496, 128, 0, PTR),
    ("ring", 2500, 13, 64, 544, 64, 0, PTR),
    ("ring", 2500, 13, 64, 496, 128, 0, 0),
    ("ring", 2500, 13, 64, 544, 64, 0, 0),
    ("ring", 2500, 13, 64, 528, 64, 0, PTR),
    ("ring", 2500, 13, 64, 528, 64, 0, 0),
    ("ring", 2500, 32, 100, 240, 128, 0, PTR),
    ("ring", 2500, 32, 100, 240, 128, 0, 0),
    ("ring", 2500, 32, 100, 208, 128, 0, PTR),
    ("ring", 2500, 32, 100, 256, 64, 0, PTR),
    ("ring", 2500, 32, 100, 208, 128, 0, 0),
    ("ring", 2500, 32, 100, 256, 64, 0, 0),
    ("ring", 2500, 32, 100, 240, 64, 0, PTR),
    ("ring", 2500, 32, 100, 240, 64, 0, 0),
    ("ring", 2500, 32, 13, 1600, 128, 0, PTR),
    ("ring", 2500, 32, 13, 1824, 64, 0, PTR),
    ("ring", 2500, 32, 13, 1600, 128, 0, 0),
    ("ring", 2500, 32, 13, 1824, 64, 0, 0),
    ("ring", 2500, 32, 13, 1712, 64, 0, PTR),
    ("ring", 2500, 32, 13, 1712, 64, 0, 0),
    ("ring", 2500, 32, 32, 880, 128, 0, PTR),
    ("ring", 2500, 32, 32, 1008, 64, 0, PTR),
    ("ring", 2500, 32, 32, 880, 128, 0, 0),
    ("ring", 2500, 32, 32, 1008, 64, 0, 0),
    ("ring", 2500, 32, 32, 768, 128, 0, PTR),
    ("ring", 2500, 32, 32, 944, 64, 0, PTR),
    ("ring", 2500, 32, 32, 768, 128, 0, 0),
    ("ring", 2500, 32, 32, 944, 64, 0, 0),
    ("ring", 2500, 32, 32, 880, 64, 0, PTR),
    ("ring", 2500, 32, 32, 880, 64, 0, 0),
    ("ring", 2500, 32, 64, 464, 128, 0, PTR),
    ("ring", 2500, 32, 64, 528, 64, 0, PTR),
    ("ring", 2500, 32, 64, 464, 128, 0, 0),
    ("ring", 2500, 32, 64, 528, 64, 0, 0),
    ("ring", 2500, 32, 64, 400, 128, 0, PTR),
    ("ring", 2500, 32, 64, 496, 64, 0, PTR),
    ("ring", 2500, 32, 64, 400, 128, 0, 0),
    ("ring", 2500, 32, 64, 496, 64, 0, 0),
    ("ring", 2500, 32, 64, 464, 64, 0, PTR),
    ("ring", 2500, 32, 64, 464, 64, 0, 0),
    ("ring", 2500, 64, 100, 176, 128, 0, PTR),
    ("ring", 2500, 64, 100, 176, 128, 0, 0),
    ("ring", 2500, 64, 100, 112, 128, 0, PTR),
    ("ring", 2500, 64, 100, 208, 64, 0, PTR),
    ("ring", 2500, 64, 100, 112, 128, 0, 0),
    ("ring", 2500, 64, 100, 208, 64, 0, 0),
    ("ring", 2500, 64, 100, 176, 64, 0, PTR),
    ("ring", 2500, 64, 100, 176, 64, 0, 0),
    ("ring", 2500, 64, 13, 1200, 128, 0, PTR),
    ("ring", 2500, 64, 13, 1616, 64, 0, PTR),
    ("ring", 2500, 64, 13, 1200, 128, 0, 0),
    ("ring", 2500, 64, 13, 1616, 64, 0, 0),
    ("ring", 2500, 64, 13, 1408, 64, 0, PTR),
    ("ring", 2500, 64, 13, 1408, 64, 0, 0),
    ("ring", 2500, 64, 32, 896, 64, 0, PTR),
    ("ring", 2500, 64, 32, 896, 64, 0, 0),
    ("ring", 2500, 64, 32, 784, 64, 0, PTR),
    ("ring", 2500, 64, 32, 784, 64, 0, 0),
    ("ring", 2500, 64, 64, 352, 128, 0, PTR),
    ("ring", 2500, 64, 64, 464, 64, 0, PTR),
    ("ring", 2500, 64, 64, 352, 128, 0, 0),
    ("ring", 2500, 64, 64, 352, 128, 3, 0),
    ("ring", 2500, 64, 64, 464, 64, 0, 0),
    ("ring", 2500, 64, 64, 224, 128, 0, PTR),
    ("ring", 2500, 64, 64, 400, 64, 0, PTR),
    ("ring", 2500, 64, 64, 224, 128, 0, 0),
    ("ring", 2500, 64, 64, 400, 64, 0, 0),
    ("ring", 2500, 64, 64, 352, 64, 0, PTR),
    ("ring", 2500, 64, 64, 352, 64, 0, 0),
    # ---- rgcn_tile3p_kernel: ST 8 (chunk 128, tile <= 224) on layouts 0 / 1 / 3, ST 7 (chunk 112, tile <= 272) on 0 / 3 ----
    ("ring", 2500, 64, 64, 224, 128, 0, SPLIT),
    ("ring", 2500, 64, 64, 224, 128, 1, SPLIT),
    ("ring", 2500, 64, 64, 224, 128, 3, SPLIT),
    ("ring", 2500, 64, 64, 272, 112, 0, SPLIT),
    ("ring", 2500, 64, 64, 272, 112, 3, SPLIT),
    ("ring", P3_MULTI_NODES, 64, 64, 16, 128, 0, SPLIT),
    ("ring", P3_MULTI_NODES, 64, 64, 16, 128, 1, SPLIT),
    ("ring", P3_MULTI_NODES, 64, 64, 16, 128, 3, SPLIT),
    ("ring", P3_MULTI_NODES, 64, 64, 16, 112, 0, SPLIT),
    ("ring", P3_MULTI_NODES, 64, 64, 16, 112, 3, SPLIT),
    # ---- direct-gather d_weight on a tile plan --------------------------------------------------------------------------
    ("ring", 2500, 64, 64, 352, 64, 0, DIRECT),
    # ---- rgcn_tile_kernel walking 2..16 tiles per workgroup --------------------------------------------------------------
    *[("ring", n, 13, 13, 16, 64, 0, 0) for n in TPW_NODES],
    # ---- edge-parallel path at every width pair, both addressing modes; bf16 x 3 transform; direct dW on dense units ---
    *[("ep", 2500, din, dout, 0, 64, 2, f) for din in (13, 32, 64, 100) for dout in (13, 32, 64, 100) for f in (0, PTR)],
    ("ep", 2500, 64, 64, 0, 64, 2, SPLIT),
    ("ep", 2500, 64, 64, 0, 64, 2, DIRECT),
    # ---- root-only walks: chunk 64 / 128 / 112, every last-tile row count of ROOT_M -------------------------------------
    *[("root", 256 + m, din, dout, 128, ch, 0, 0) for ch, (din, dout) in ((64, (64, 64)), (128, (13, 100)), (112, (100, 32)))
      for m in ROOT_M],
    # ---- tile-major d_weight: exact / split operands, one row per slot / pairs on one slot -------------------------------
    *[("dwt", 3000, 64, 64, 320, 64, lay, f) for lay in (0, 5) for f in (0, SPLIT)],
]


def _chunk_form(chunk):
    """(chunk, chunk_rows) of the plan header a builder ``chunk`` argument makes"""
    return (128, 112) if chunk == 112 else (chunk, chunk)


def _dw_flags(flags):
    return flags if flags & K.FLAG_DW_DIRECT else flags | K.FLAG_DW_RING


def case_targets(case):
    """The instantiation tuples a case runs, under the mirror (from the case row alone: no plan needed)."""
    kind, n, din, dout, tile, chunk, layout, flags = case
    ch, cr = _chunk_form(chunk)
    nt = -(-n // tile) if tile else 1
    if kind == "ring":
        out = [K.run_tile(din, dout, tile, ch, cr, layout, flags, True, nt), K.run_tile(dout, din, tile, ch, cr, layout, flags, True, nt),
               K.tile_tpw(din, dout, tile, ch, cr, layout, flags, True, nt), K.tile_tpw(dout, din, tile, ch, cr, layout, flags, True, nt)]
        if layout != 3:
            out.append(K.bwd_dw(din, dout, tile, ch, cr, layout, _dw_flags(flags), True, nt))
        return [t for t in out if t is not None and t[0] != "err"]
    if kind == "ep":
        return [K.ep_transform(din, dout, 0, 64, 64, 2, flags, True, 1), K.ep_transform(dout, din, 0, 64, 64, 2, flags, True, 1),
                K.ep_segment_sum(din, dout, 0, 64, 64, 2, flags, True, 1), K.ep_segment_sum(dout, din, 0, 64, 64, 2, flags, True, 1),
                K.bwd_dw(din, dout, 0, 64, 64, 2, _dw_flags(flags), True, 1)]
    if kind == "root":
        return [K.dw_root_only(din, dout, tile, ch, cr, layout, flags | K.FLAG_DW_ROOT_ONLY, True, nt)]
    if kind == "dwt":
        return [K.bwd_dw_tiles(din, dout, tile, ch, cr, layout, flags, True, nt, NUM_REL)]
    raise ValueError(kind)


def case_id(case):
    kind, n, din, dout, tile, chunk, layout, flags = case
    return f"{kind}-n{n}-{din}x{dout}-t{tile}-c{chunk}-l{layout}-f{flags}"


# ---------------------------------------------------------------------------------------------------------------------
def window_starts(n, tiles=(224, 272), count=8, span=128):
    """starts of the windows of relation 4: each lies inside one tile of every size in ``tiles``"""
    out, s = [], 0
    while s + span <= n and len(out) < count:
        if all(s // t == (s + span - 1) // t for t in tiles):
            out.append(s)
            s += span
        else:
            s += 16
    return out


def make_graph(n):
    """Random edges over relations 0..3 (2 per node), relation 5 dead; window k = 1..8 of relation 4 sends 16 k - 8 edges
    into 16 k - 8 distinct nodes of one tile (a group that fills k row tiles, uncompactable by layout 3); self loops,
    duplicate triples and one hub (300 edges in, 100 out)."""
    g = torch.Generator().manual_seed(n)
    e = 2 * n
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, n, (e,), generator=g)
    et = torch.randint(0, 4, (e,), generator=g)
    src[:20] = dst[:20]                                   # self loops
    src[40:80], dst[40:80], et[40:80] = src[100:140], dst[100:140], et[100:140]     # duplicate triples
    hub = n // 3
    dst[200:500] = hub
    src[500:600] = hub
    ws, wd = [], []
    for k, s in enumerate(window_starts(n), start=1):
        m = 16 * k - 8
        wd.append(torch.arange(s, s + m))
        ws.append(torch.randint(0, n, (m,), generator=g))
    if ws:
        src, dst = torch.cat([src] + ws), torch.cat([dst] + wd)
        et = torch.cat([et, torch.full((sum(len(w) for w in ws),), 4, dtype=torch.int64)])
    return torch.stack([src, dst]), et


_ORACLE = {}


def oracle(n, din, dout):
    """graph, inputs, float64 reference, condition numbers and fp32 CPU loop, shared by every case on (n, din, dout)"""
    key = (n, din, dout)
    if key not in _ORACLE:
        ei, et = make_graph(n)
        w, root, _ = O.synthetic_params(NUM_REL, din, dout, seed=din * 131 + dout)
        g = torch.Generator().manual_seed(7919 * n + 31 * din + dout)
        bias = torch.randn(dout, generator=g) * 0.1
        x = torch.randn(n, din, generator=g)
        dg = torch.randn(n, dout, generator=g)
        mask = torch.randn(n, din, generator=g)
        ref, gr = O.rgcn_conv_segments(x.numpy(), ei.numpy(), et.numpy(), w.numpy(), root.numpy(), bias.numpy(), dg.numpy())
        c_out, c = abs_condition(x, ei, et, w, root, bias, dg)
        o32, g32 = cpu32_reference(x, ei, et, w, root, bias, dg)
        _ORACLE.clear()          # cases are ordered by key: keep one entry (the large graphs are tens of MB)
        _ORACLE[key] = dict(ei=ei, et=et, w=w, root=root, bias=bias, x=x, dg=dg, mask=mask, ref=ref, gr=gr, c_out=c_out, c=c,
                            o32=o32, g32=g32)
    return _ORACLE[key]


def _act(a, act):
    a = np.asarray(a, dtype=np.float64)
    return a if act == 0 else (np.maximum(a, 0.0) if act == 1 else 1.0 / (1.0 + np.exp(-a)))


def _check_out(out, o, act, tag):
    assert_close(out, _act(o["ref"], act), o["c_out"], "out" + tag, cpu32=_act(o["o32"], act))


def _check_dx(dx, o, masked, tag):
    m = (o["mask"].numpy() > 0) if masked else 1.0
    assert_close(dx, o["gr"]["x"] * m, o["c"]["x"], "d_x" + tag, cpu32=o["g32"]["x"] * m)


def _check_dw(dw, dr, db, o, tag):
    if dw is not None:
        assert_close(dw, o["gr"]["weight"], o["c"]["weight"], "d_weight" + tag, cpu32=o["g32"]["weight"])
    assert_close(dr, o["gr"]["root"], o["c"]["root"], "d_root" + tag, cpu32=o["g32"]["root"])
    assert_close(db, o["gr"]["bias"], o["c"]["bias"], "d_bias" + tag, cpu32=o["g32"]["bias"])


def _nrt_set(plan, cap):
    cnt = plan.chunk_cnt.cpu().numpy()
    return set(np.minimum(cap, (cnt + 15) // 16).tolist())


def _plan_targets(plan, din, dout, flags, dw=True):
    """the mirror's answer for the plan the builder actually made (tile, chunk, chunk_rows, layout, tile count)"""
    a = (plan.tile, plan.chunk, plan.chunk_rows, plan.layout, flags, True, plan.n_tiles)
    out = [K.run_tile(din, dout, *a), K.tile_tpw(din, dout, *a)]
    if dw:
        out.append(K.bwd_dw(din, dout, plan.tile, plan.chunk, plan.chunk_rows, plan.layout, _dw_flags(flags), True, plan.n_tiles,
                            plan.n_units))
    return out


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from scaling_rgcn_training_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _inputs(dev, o, din, dout):
    from scaling_rgcn_training_amd import _lib
    from scaling_rgcn_training_amd.conv import _rows16
    xd, gd = _rows16(o["x"].to(dev), din), _rows16(o["dg"].to(dev), dout)
    wd, rd, bd = o["w"].to(dev).contiguous(), o["root"].to(dev).contiguous(), o["bias"].to(dev).contiguous()
    return xd, gd, _lib.pack_weights(wd, rd, False), _lib.pack_weights(wd, rd, True), bd


def _run_ring(dev, case, idx):
    from scaling_rgcn_training_amd import _lib, plan as P
    from scaling_rgcn_training_amd.conv import _rows16, _round4
    kind, n, din, dout, tile, chunk, layout, flags = case
    o = oracle(n, din, dout)
    act, masked = idx % 3, idx % 2 == 1
    tag = f" [{case_id(case)} act{act} mask{int(masked)}]"
    plans = P.build_graph_plans_device(o["ei"].to(dev), o["et"].to(dev), n, NUM_REL, tile, chunk=chunk, split=layout)
    want = case_targets(case)
    # non-vacuity: the plans the builder made reach what the case row targets
    ch, cr = _chunk_form(chunk)
    for pl in (plans.fwd, plans.bwd):
        assert (pl.tile, pl.chunk, pl.chunk_rows, pl.layout, pl.n_tiles) == (tile, ch, cr, layout, -(-n // tile)), tag
    got = _plan_targets(plans.fwd, din, dout, flags, dw=layout != 3) + _plan_targets(plans.bwd, dout, din, flags, dw=False)
    assert got[0][0] != "err", (tag, got)
    assert set(t for t in got if t is not None and t[0] != "err") == set(want), (tag, got, want)
    dx_err = got[-2] if got[-2][0] == "err" else None
    for t in want:
        if t[0] == "tpw" and t[1] > 1:      # a multi-tile walk whose last workgroup walks fewer tiles
            assert plans.fwd.n_tiles % t[1] != 0, tag
        if t[0] == "tile3p":
            if t[3]:
                tpw = K.tiles_per_workgroup(plans.fwd.n_tiles)
                assert tpw > 1 and plans.fwd.n_tiles % tpw != 0, tag
            elif layout in (0, 3):     # every row-tile count the kernel's switch has a case for
                assert _nrt_set(plans.fwd, t[1]) >= set(range(1, t[1] + 1)), (tag, _nrt_set(plans.fwd, t[1]))
    xd, gd, pw, pwt, bd = _inputs(dev, o, din, dout)
    out = torch.full((n, _round4(dout)), float("nan"), device=dev)
    _lib.fwd(_lib.plan_struct(plans.fwd), xd, din, pw, bd, out, dout, act, flags)
    dx = torch.full((n, _round4(din)), float("nan"), device=dev)
    mask = _rows16(o["mask"].to(dev), din) if masked else None
    if dx_err is None:
        _lib.bwd_dx(_lib.plan_struct(plans.bwd), gd, dout, pwt, dx, din, mask, flags)
    else:           # the transposed direction has no ring that fits: refused, nothing written
        with pytest.raises(_lib.RgcnLibraryError) as ei:
            _lib.bwd_dx(_lib.plan_struct(plans.bwd), gd, dout, pwt, dx, din, mask, flags)
        assert ei.value.status == dx_err[1], tag
    res = None
    if layout != 3:
        dw = torch.full((NUM_REL, din, dout), float("nan"), device=dev)
        dr = torch.full((din, dout), float("nan"), device=dev)
        db = torch.full((dout,), float("nan"), device=dev)
        _lib.bwd_dw(_lib.plan_struct(plans.fwd), xd, din, gd, dout, dw, dr, db, _dw_flags(flags))
        res = dw, dr, db
    torch.cuda.synchronize()
    _check_out(out[:, :dout].cpu().numpy(), o, act, tag)
    if dx_err is None:
        _check_dx(dx[:, :din].cpu().numpy(), o, masked, tag)
    else:
        assert bool(dx.isnan().all()), tag
    if res is not None:
        _check_dw(*(t.cpu().numpy() for t in res), o, tag)
        assert torch.all(res[0][NUM_REL - 1] == 0), tag         # the dead relation


def _run_ep(dev, case, idx):
    from scaling_rgcn_training_amd import _lib, eplan as E, plan as P
    from scaling_rgcn_training_amd.conv import _rows16, _round4
    kind, n, din, dout, tile, chunk, layout, flags = case
    o = oracle(n, din, dout)
    act, masked = idx % 3, idx % 2 == 1
    tag = f" [{case_id(case)} act{act} mask{int(masked)}]"
    eid, etd = o["ei"].to(dev), o["et"].to(dev)
    wgt = P.edge_weights(eid[0], eid[1], etd, NUM_REL)
    fwd = E.build_edge_plan(eid[0], eid[1], etd, wgt, n, NUM_REL, heavy=0)
    bwd = E.build_edge_plan(eid[1], eid[0], etd, wgt, n, NUM_REL, heavy=0)
    tp = fwd.as_tile_plan()
    assert tp.layout == 2 and tp.chunk == 64 and fwd.heavy is None and bwd.heavy is None, tag
    xd, gd, pw, pwt, bd = _inputs(dev, o, din, dout)
    out = torch.full((n, _round4(dout)), float("nan"), device=dev)
    _lib.ep_layer(fwd, xd, din, pw, bd, out, dout, act, None, flags)
    dx = torch.full((n, _round4(din)), float("nan"), device=dev)
    _lib.ep_layer(bwd, gd, dout, pwt, None, dx, din, 0, _rows16(o["mask"].to(dev), din) if masked else None, flags)
    dw = torch.full((NUM_REL, din, dout), float("nan"), device=dev)
    dr = torch.full((din, dout), float("nan"), device=dev)
    db = torch.full((dout,), float("nan"), device=dev)
    _lib.bwd_dw(_lib.plan_struct(tp), xd, din, gd, dout, dw, dr, db, _dw_flags(flags))
    torch.cuda.synchronize()
    _check_out(out[:, :dout].cpu().numpy(), o, act, tag)
    _check_dx(dx[:, :din].cpu().numpy(), o, masked, tag)
    _check_dw(dw.cpu().numpy(), dr.cpu().numpy(), db.cpu().numpy(), o, tag)


def _run_root(dev, case, idx):
    from scaling_rgcn_training_amd import _lib, plan as P
    kind, n, din, dout, tile, chunk, layout, flags = case
    o = oracle(n, din, dout)
    tag = f" [{case_id(case)}]"
    plans = P.build_graph_plans_device(o["ei"].to(dev), o["et"].to(dev), n, NUM_REL, tile, chunk=chunk)
    pl = plans.fwd
    ch, cr = _chunk_form(chunk)
    assert (pl.tile, pl.chunk, pl.chunk_rows, pl.layout, pl.n_tiles) == (tile, ch, cr, 0, 3), tag
    # the closed form rgcn_bwd_dw uses for the root units' count against the units of the root relation in the plan
    upc = pl.chunk // 64
    rel_of_unit = pl.chunk_rel[pl.rel_order.long() // upc]
    n_root = int((rel_of_unit == pl.num_relations).sum())
    assert n_root == K.root_units(pl.n_owned, pl.n_tiles, pl.tile, pl.chunk, pl.chunk_rows), tag
    assert bool((rel_of_unit[pl.n_units - n_root:] == pl.num_relations).all()), tag       # they close rel_order
    xd, gd, _, _, _ = _inputs(dev, o, din, dout)
    dr = torch.full((din, dout), float("nan"), device=dev)
    db = torch.full((dout,), float("nan"), device=dev)
    _lib.bwd_dw(_lib.plan_struct(pl), xd, din, gd, dout, None, dr, db, K.FLAG_DW_ROOT_ONLY | K.FLAG_DW_RING)
    dw0 = torch.full((NUM_REL, din, dout), float("nan"), device=dev)
    dr0, db0 = torch.full_like(dr, float("nan")), torch.full_like(db, float("nan"))
    _lib.bwd_dw(_lib.plan_struct(pl), xd, din, gd, dout, dw0, dr0, db0, K.FLAG_DW_RING)
    torch.cuda.synchronize()
    dr, db, dr0, db0 = (t.cpu().numpy() for t in (dr, db, dr0, db0))
    _check_dw(None, dr, db, o, " (root-only)" + tag)
    _check_dw(dw0.cpu().numpy(), dr0, db0, o, " (full walk)" + tag)
    # (the two walks cut the units over different workgroup counts: equal up to fp32 re-association)
    assert_close(dr, dr0, o["c"]["root"], "root-only vs full walk d_root" + tag)
    assert_close(db, db0, o["c"]["bias"], "root-only vs full walk d_bias" + tag)


def _run_dwt(dev, case, idx):
    from scaling_rgcn_training_amd import _lib, plan as P
    kind, n, din, dout, tile, chunk, layout, flags = case
    o = oracle(n, din, dout)
    tag = f" [{case_id(case)}]"
    if layout == 5:
        plans = P.build_graph_plans_device(o["ei"].to(dev), o["et"].to(dev), n, NUM_REL, 128, dw_tiles=True)
        pl, walk = plans.dw, plans.dw_walk
        src2 = pl.slot_src2.cpu()
        assert bool((src2 != pl.n_nodes).any()), tag      # pairs were formed
    else:
        plans = P.build_graph_plans_device(o["ei"].to(dev), o["et"].to(dev), n, NUM_REL, tile, chunk=chunk)
        pl = plans.fwd
        walk = _lib.dw_tiles_walk(_lib.plan_struct(pl), dev)
    assert (pl.tile, pl.chunk, pl.layout) == (tile, chunk, layout), tag
    assert K.bwd_dw_tiles(din, dout, pl.tile, pl.chunk, pl.chunk_rows, pl.layout, flags, True, pl.n_tiles, NUM_REL) == case_targets(case)[0]
    xd, gd, _, _, _ = _inputs(dev, o, din, dout)
    dw = torch.full((NUM_REL, din, dout), float("nan"), device=dev)
    _lib.bwd_dw_tiles(_lib.plan_struct(pl), walk, xd, din, gd, dout, dw, flags)
    torch.cuda.synchronize()
    assert_close(dw.cpu().numpy(), o["gr"]["weight"], o["c"]["weight"], "d_weight (tile-major)" + tag, cpu32=o["g32"]["weight"])
    assert torch.all(dw[NUM_REL - 1] == 0), tag


_RUN = {"ring": _run_ring, "ep": _run_ep, "root": _run_root, "dwt": _run_dwt}
# cases sharing (n, din, dout) run back to back, so each oracle is computed once
_ORDER = sorted(range(len(CASES)), key=lambda i: (CASES[i][1], CASES[i][2], CASES[i][3], i))


@pytest.mark.parametrize("idx", _ORDER, ids=[case_id(CASES[i]) for i in _ORDER])
def test_kernel_variant(dev, idx):
    case = CASES[idx]
    _RUN[case[0]](dev, case, idx)
