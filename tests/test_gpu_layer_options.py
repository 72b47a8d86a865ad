"""RGCNConv's constructor options on every route of the base kernel family (float features, mean / sum, at most 128 columns per
side), through the module, against the float64 oracle: weight mode x aggr x root / bias x trainable set over the routes of
tests/layer_options.py (a pairwise cover; tests/test_layer_options.py proves it on the CPU).  Every case asserts the route it
took -- from ``conv._route`` and from the plans -- so a case that drifts to other kernels fails instead of passing on them.
Output, d_x, d_root, d_bias and the gradients of the layer's own weight parameters (bases + comp, blocks) under both bounds of
oracle/tolerance.py; never compared with another kernel of the library."""
import pytest
import torch

from tests import layer_options as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from scaling_rgcn_training_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _run(conv, x, eid, etd, g, dev, x_grad):
    for p in conv.parameters():
        p.grad = None
    xd = x.to(dev).requires_grad_(x_grad)
    out = conv(xd, eid, etd)
    out.backward(g.to(dev))
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu().clone() for k, p in conv.named_parameters() if p.grad is not None}
    return xd, out.detach().cpu(), None if xd.grad is None else xd.grad.detach().cpu(), grads


@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_layer_options_against_fp64(dev, monkeypatch, case):
    from scaling_rgcn_training_amd import conv as conv_mod
    from scaling_rgcn_training_amd.plan import clear_plan_cache
    c, rt, tag = case, L.ROUTES[case.route], L.case_id(case)
    ei, et = L.make_graph(c)
    assert int((et == c.r - 1).sum()) == 0, "the last relation has no edge"
    eid, etd = ei.to(dev), et.to(dev)
    conv = L.make_layer(c, monkeypatch).to(dev)
    gen = torch.Generator().manual_seed(7)
    x, g = torch.randn(c.n, c.din, generator=gen), torch.randn(c.n, c.dout, generator=gen)
    x_grad = c.frozen != "x"
    try:
        xd, out, dx, grads = _run(conv, x, eid, etd, g, dev, x_grad)
        # ---- the route the layer took
        route = conv._route(c.n, int(et.shape[0]), True)
        L.assert_route(c, route)
        plans = conv._plans(xd, eid, etd, route)
        ep = tuple(reversed(rt.ep)) if c.swap else rt.ep
        assert ((plans.ep_fwd is not None), (plans.ep_bwd is not None)) == ep, tag
        assert ((plans.fwd is None), (plans.bwd is None)) == ep, tag
        for pl in (plans.fwd, plans.bwd):
            if pl is not None:
                assert pl.layout == rt.layout and pl.chunk == (64 if c.chunk == 64 else 128), (tag, pl.layout, pl.chunk)
                assert (pl.chunk_rows or pl.chunk) == c.chunk, (tag, pl.chunk_rows)
        assert (plans.dw is not None) == rt.dw and (plans.dw_walk is not None) == rt.dw, tag
        if rt.dw:
            assert plans.dw.layout == 5, "the pair plan of the tile-major d_weight kernel"
        if ep[0]:
            assert plans.ep_fwd.heavy is not None and plans.ep_fwd.heavy.n_seg > 0, "a hub graph: heavy segments in the forward"
        if rt.side_rows is not None:
            assert c.n >= conv_mod._SIDE_STREAM_MIN_ROWS and x_grad and (conv.root is not None or conv.bias is not None)
        # ---- shapes, the float64 reference, frozen / absent parameters
        assert out.shape == (c.n, c.dout) and (dx is None) == (not x_grad) and (dx is None or dx.shape == (c.n, c.din))
        assert all(grads[k].shape == getattr(conv, k).shape for k in grads)
        L.check_layer(conv, x, ei, et, g, out, dx, grads, tag)
        if c.mode == "full" and "weight" in grads:
            assert torch.all(grads["weight"][c.r - 1] == 0), "the relation without edges"
        # ---- bit-reproducible
        _, out2, dx2, grads2 = _run(conv, x, eid, etd, g, dev, x_grad)
        assert torch.equal(out, out2) and (dx is None or torch.equal(dx, dx2))
        assert grads.keys() == grads2.keys() and all(torch.equal(grads[k], grads2[k]) for k in grads), tag
    finally:
        clear_plan_cache()
