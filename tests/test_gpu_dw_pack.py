"""The packed tile-major weight-gradient plan on the GPU: dw_pack_kernel (csrc/rgcn_plan.hip) against its torch twin plan.dw_pack at
shapes whose walker ranges span tiles, and rgcn_bwd_dw_tiles -- all four forms of rgcn_dw_tile_kernel -- walking units that hold
rows of two tiles, against the float64 oracle."""
import copy

import numpy as np
import pytest
import torch

from oracle import rgcn_oracle as O
from oracle.tolerance import abs_condition, assert_close, cpu32_reference
from tests import dw_pack_checks as C
from tests.test_gpu_plan_build import _compare

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
R = 32

# name: (nodes, edges, skew, dead last relation, owned range of the forward plan, of the transposed plan)
CASES = {
    "uniform": (41_600, 416_000, False, False, None, None),                       # 130 tiles, two per walker range
    "skew": (41_600, 416_000, True, False, None, None),                           # hubs: groups the pairs pass leaves alone
    "sparse": (41_600, 60_000, False, False, None, None),                         # relations absent from tiles: units closed early
    "range": (41_500, 416_000, False, True, (6_400, 41_500), (0, 35_200)),        # node_begin > 0, a partial last tile, a relation without edges
}
_cache = {}


def _graph(name, unique=False):
    n, e, skew, dead, fr, br = CASES[name]
    ei, et = O.synthetic_graph(n, e, R, seed=n + e, skew=skew)
    if dead:
        et = et.clamp(max=R - 2)
    if unique:      # one edge per (destination, relation): a plan without pairs
        key = (ei[1] * R + et).numpy()
        keep = torch.from_numpy(np.sort(np.unique(key, return_index=True)[1]))
        ei, et = ei[:, keep].contiguous(), et[keep].contiguous()
    else:
        ei[:, 10:40] = ei[:, 50:80]                # duplicate triples: merged slots inside runs
        et[10:40] = et[50:80]
    return n, ei, et, fr, br


def _case(name, unique=False):
    """device plans (bit-identical to the twin's: _compare), operands and the float64 / fp32 CPU references, once per case"""
    if (name, unique) in _cache:
        return _cache[name, unique]
    from scaling_rgcn_training_amd import _lib
    t_dw, walkers, _ = _lib.dw_tiles_geometry()
    from scaling_rgcn_training_amd import plan as P
    assert (t_dw, walkers) == (320, P.DW_WALKERS)
    n, ei, et, fr, br = _graph(name, unique)
    plans = _compare(ei.to(DEV), et.to(DEV), n, R, t_dw, 64, fr=fr, br=br, split=5)
    w, root, bias = O.synthetic_params(R, 64, 64, seed=2)
    g = torch.Generator().manual_seed(23)
    x = torch.randn(n, 64, generator=g)
    dg = torch.randn(n, 64, generator=g)
    b, e_ = fr if fr is not None else (0, n)
    dg_own = torch.zeros_like(dg)
    dg_own[b:e_] = dg[b:e_]                       # d_weight of the owned destinations = the full sum with the other gradient rows zero
    _, gr = O.rgcn_conv_segments(x.numpy(), ei.numpy(), et.numpy(), w.numpy(), root.numpy(), bias.numpy(), dg_own.numpy())
    _, c = abs_condition(x, ei, et, w, root, bias, dg_own)
    _, g32 = cpu32_reference(x, ei, et, w, root, bias, dg_own)
    _cache[name, unique] = dict(n=n, plans=plans, x=x.to(DEV), g=dg[b:e_].contiguous().to(DEV), ref=gr["weight"], cond=c["weight"],
                                cpu32=g32["weight"], dead=CASES[name][3])
    return _cache[name, unique]


@pytest.mark.parametrize("name", list(CASES))
def test_device_pack_matches_twin(name):
    """every array of the packed plan bit-identical to the twin's (both owned ranges), the invariants on the device's arrays"""
    o = _case(name)
    for p in (o["plans"].fwd, o["plans"].bwd):
        assert p.layout == 5
        straddling = C.check_units(p)
        assert straddling > 0, "no unit straddles: the case tests nothing"
    if name == "sparse":
        assert sum(s[2] for s in C.stream_stats(o["plans"].fwd)) > 0, "no unit was closed early: the case tests nothing"


def test_straddling_halves_carry_pair_heads():
    p = _case("uniform")["plans"].fwd
    flags = p.chunk_flags.cpu().numpy()
    s2 = p.slot_src2.cpu().numpy().reshape(-1, 2, 4)
    h0 = np.nonzero((flags >> 28 & 1).astype(bool) & (s2[:, 0] < p.n_nodes).any(axis=1))[0]
    h1 = np.nonzero((flags >> 29 & 1).astype(bool) & (s2[:, 1] < p.n_nodes).any(axis=1))[0]
    assert len(h0) > 0 and len(h1) > 0
    u = int(h0[0])
    assert (s2[u, 0][s2[u, 0] != p.n_nodes] < p.n_nodes).all() and (s2[u, 0] < p.n_nodes).any()


def _run(o, plan, flags):
    from scaling_rgcn_training_amd import _lib
    ps = _lib.plan_struct(plan)
    walk = _lib.dw_tiles_walk(ps, DEV)
    dw = torch.full((R, 64, 64), float("nan"), device=DEV)
    _lib.bwd_dw_tiles(ps, walk, o["x"], 64, o["g"], 64, dw, flags)
    torch.cuda.synchronize()
    return dw


@pytest.mark.parametrize("split", [False, True], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("pairs", [True, False], ids=["pairs", "nopairs"])
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_walks_packed_plan(name, pairs, split):
    """rgcn_dw_tile_kernel<split, pairs> on units of two tiles.  The forms without pairs walk the packed plan of the same graph cut
    down to one edge per (destination, relation) -- no pair forms, slot_src2 is all padding -- handed over as a layout-0 plan."""
    from scaling_rgcn_training_amd import _lib
    o = _case(name, unique=not pairs)
    plan = o["plans"].fwd
    if not pairs:
        assert int((plan.slot_src2 < plan.n_nodes).sum()) == 0
        plan = copy.copy(plan)
        plan.layout = 0
    flags = _lib.FLAG_SPLIT_PRODUCERS if split else 0
    dw = _run(o, plan, flags)
    assert_close(dw.cpu().numpy(), o["ref"], o["cond"], f"d_weight (packed plan) [{name} pairs={pairs} split={split}]", cpu32=o["cpu32"])
    if o["dead"]:
        assert torch.all(dw[R - 1] == 0)
    assert torch.equal(dw, _run(o, plan, flags)), "two runs differ"


def test_layer_step_on_packed_plan_replays_in_a_graph(monkeypatch):
    """forward + backward of the module on the tile-major path (forced at this size) captured and replayed: bit-identical"""
    from scaling_rgcn_training_amd import conv as M
    monkeypatch.setattr(M, "DW_TILES_MIN_EDGES", 1)
    monkeypatch.setattr(M, "_SIDE_STREAM_MIN_ROWS", 1)
    n, ei, et, _, _ = _graph("uniform")
    ei, et = ei.to(DEV), et.to(DEV)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n, 64, generator=g).to(DEV).requires_grad_(True)
    dg = torch.randn(n, 64, generator=g).to(DEV)
    conv = M.RGCNConv(64, 64, R).to(DEV)

    def step():
        x.grad = None
        conv.zero_grad(set_to_none=True)
        out = conv(x, ei, et)
        out.backward(dg)
        return out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    plans = conv._plans(x, ei, et)
    assert plans.dw is not None and C.check_units(plans.dw) > 0
    ref = [t.detach().clone() for t in (step(), x.grad, conv.weight.grad, conv.root.grad, conv.bias.grad)]
    x.grad = None
    conv.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = conv(x, ei, et)
        out.backward(dg)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for a, b, nm in zip((out, x.grad, conv.weight.grad, conv.root.grad, conv.bias.grad), ref, ("out", "d_x", "d_weight", "d_root", "d_bias")):
        assert torch.equal(a, b), nm
