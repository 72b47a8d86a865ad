"""The bipartite RGCNConv's constructor options on every route a bipartite call can take, through the module, against the float64
reference of tests/bipartite_reference.py: weight mode x aggr x root / bias x trainable set over the routes of
tests/bipartite_options.py (a pairwise cover; tests/test_bipartite_options.py proves it on the CPU), at N_src != N_dst in both
orders.  Every case asserts the route it took -- from ``conv._route`` and from the plans the call ran on -- so a case that drifts
to other kernels fails instead of passing on them.  Output, d_x_src, d_x_dst, d_root, d_bias and the gradients of the layer's own
weight parameters (bases + comp, blocks) under both bounds of oracle/tolerance.py; never compared with another kernel."""
import inspect

import pytest
import torch

from tests import bipartite_options as L
from tests.bipartite_reference import check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from scaling_rgcn_training_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _run(conv, xs, xd, eid, etd, g, grad_src, grad_dst):
    for p in conv.parameters():
        p.grad = None
    xs, xd = xs.clone().requires_grad_(grad_src), xd.clone().requires_grad_(grad_dst)
    out = conv((xs, xd), eid, etd)
    out.backward(g)
    torch.cuda.synchronize()
    res = {"out": out.detach().cpu(), "x_src": None if xs.grad is None else xs.grad.cpu(), "x_dst": None if xd.grad is None else xd.grad.cpu()}
    res.update({k: p.grad.detach().cpu().clone() for k, p in conv.named_parameters() if p.grad is not None})
    return res


def _spy_on_flags(monkeypatch):
    """the ``flags`` argument of every forward, dX and relation-major d_weight call that reaches the binding: {entry: {flags}}"""
    from scaling_rgcn_training_amd import _lib
    seen = {}
    for name in ("fwd", "bwd_dx", "bwd_dw", "ep_layer"):
        fn = getattr(_lib, name)
        sig = inspect.signature(fn)

        def spy(*a, _fn=fn, _sig=sig, _name=name, **k):
            bound = _sig.bind(*a, **k)
            bound.apply_defaults()
            seen.setdefault(_name, set()).add(int(bound.arguments["flags"]))
            return _fn(*a, **k)

        monkeypatch.setattr(_lib, name, spy)
    return seen


@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_bipartite_options_against_fp64(dev, monkeypatch, case):
    from scaling_rgcn_training_amd import _lib
    from scaling_rgcn_training_amd.plan import clear_plan_cache
    c, tag = case, L.case_id(case)
    ei, et = L.make_graph(c)
    assert int((et == c.r - 1).sum()) == 0, "the last relation has no edge"
    eid, etd = ei.to(dev), et.to(dev)
    conv = L.make_layer(c).to(dev)
    gen = torch.Generator().manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)      # noqa: E731
    xs, xd, g = rnd(c.n_src, c.in_src), rnd(c.n_dst, c.in_dst), rnd(c.n_dst, c.dout)
    grad_src, grad_dst = c.frozen != "x_src", c.frozen != "x_dst"
    seen = _spy_on_flags(monkeypatch)
    try:
        got = _run(conv, xs, xd, eid, etd, g, grad_src, grad_dst)
        # ---- the route the layer took
        n = max(c.n_src, c.n_dst)
        route = conv._route(n, int(et.shape[0]), True, plain=True)
        L.assert_route(c, route)
        plans = conv._bipartite_plans(eid, etd, c.n_src, c.n_dst, route)      # (the cached plans of the call above)
        ep = L.ep_of(c)
        print(f"\n{tag}: tile {route.tile} chunk {route.chunk} split {route.split_producers} paths {route.paths} flags {conv.kernel_flags}")
        assert ((plans.ep_fwd is not None), (plans.ep_bwd is not None)) == ep, tag
        assert ((plans.fwd is None), (plans.bwd is None)) == ep, tag
        assert plans.dw is None and plans.dw_walk is None, "never a tile-major d_weight plan"
        for pl, rows in ((plans.fwd, c.n_dst), (plans.bwd, c.n_src)):
            if pl is not None:
                assert pl.layout == 0 and pl.chunk == c.chunk and (pl.chunk_rows or pl.chunk) == c.chunk, (tag, pl.layout, pl.chunk)
                assert (pl.n_nodes, pl.node_begin, pl.node_end) == (n, 0, rows), (tag, pl.n_nodes, pl.node_begin, pl.node_end)
                assert pl.n_tiles == -(-rows // route.tile) > 2 and rows % route.tile, "several tiles, the last one partial"
        for pl, rows in ((plans.ep_fwd, c.n_dst), (plans.ep_bwd, c.n_src)):
            if pl is not None:
                assert (pl.n_nodes, pl.n_owned) == (n, rows), (tag, pl.n_nodes, pl.n_owned)
                assert pl.heavy is not None and pl.heavy.n_seg > 0, "a hub on either side: heavy segments"
        # the flags that reached the kernels: the layer's own plus the bf16 x 3 bit of the route, at every launch site
        want = L.ROUTES[c.route].flags | (_lib.FLAG_SPLIT_PRODUCERS if c.split else 0)
        needs_dw = any(getattr(conv, k) is not None and getattr(conv, k).requires_grad for k in ("weight", "comp", "bias"))
        sites = {"ep_layer" if ep[0] else "fwd"} | ({"ep_layer" if ep[1] else "bwd_dx"} if grad_src else set()) | ({"bwd_dw"} if needs_dw else set())
        assert set(seen) == sites and all(v == {want} for v in seen.values()), (tag, seen, want)
        # ---- shapes, the float64 reference, frozen / absent parameters
        assert tuple(got["out"].shape) == (c.n_dst, c.dout)
        assert (got["x_src"] is None) == (not grad_src) and (got["x_src"] is None or tuple(got["x_src"].shape) == (c.n_src, c.in_src))
        assert (got["x_dst"] is None) == (not (grad_dst and c.root)) and (got["x_dst"] is None or tuple(got["x_dst"].shape) == (c.n_dst, c.in_dst))
        for name in ("weight", "comp", "root", "bias"):
            p = getattr(conv, name)
            if p is None or not p.requires_grad:
                assert name not in got and (p is None or p.grad is None), f"{tag}: {name} is frozen or absent and has a gradient"
            else:
                assert name in got and got[name].shape == p.shape, f"{tag}: {name} trains and has no gradient"
        check(conv, xs, xd, ei, et, g, got, c.aggr, tag)
        if c.mode == "full" and "weight" in got:
            assert torch.all(got["weight"][c.r - 1] == 0), "the relation without edges"
        # ---- bit-reproducible
        again = _run(conv, xs, xd, eid, etd, g, grad_src, grad_dst)
        assert got.keys() == again.keys()
        for k, v in got.items():
            assert (v is None and again[k] is None) or torch.equal(v, again[k]), (tag, k)
    finally:
        clear_plan_cache()
