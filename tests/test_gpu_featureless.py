"""Featureless RGCNConv on the GPU (csrc/rgcn_featureless.hip): x = None or int64 node indices, full or basis weights, mean or
sum, root / bias on or off -- against the fp64 oracle of the equivalent dense layer with x = one_hot(x, in_channels) (identity
for x = None); basis gradients pushed from that dense d_W through ``effective_weight`` by fp64 autograd."""
import numpy as np
import pytest
import torch

from oracle import rgcn_oracle as O
from oracle.tolerance import assert_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from scaling_rgcn_training_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _graph(n, e, r, seed):
    """random edges with duplicate triples, relation r - 1 without edges, the last 20 nodes without in-edges"""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, n - 20, (e,), generator=g)
    typ = torch.randint(0, r - 1, (e,), generator=g)
    ei = torch.cat([torch.stack([src, dst]), torch.stack([src[:150], dst[:150]])], 1)
    et = torch.cat([typ, typ[:150]])
    return ei, et


def _reference(xoh, ei, et, params, num_rel, in_rows, dout, g, aggr, absolute=False):
    """fp64 (out, grads) of the dense layer on x = xoh; with ``absolute``: on absolute values (the condition of the sums)"""
    f = (lambda t: None if t is None else t.detach().double().abs()) if absolute else (
        lambda t: None if t is None else t.detach().double())
    w, comp, root, bias = (f(p) for p in params)
    gg = g.double().abs() if absolute else g.double()
    if comp is not None:
        w = w.clone().requires_grad_(True)
        comp = comp.clone().requires_grad_(True)
    wfull = O.effective_weight(w, comp, num_rel, None, in_rows, dout)
    wn = wfull.detach().numpy()
    rn = None if root is None else root.numpy()
    out = O.rgcn_conv_dense(xoh, ei.numpy(), et.numpy(), wn, rn, None if bias is None else bias.numpy(), aggr=aggr)
    gr = O.rgcn_conv_grads_dense(xoh, ei.numpy(), et.numpy(), wn, rn, gg.numpy(), aggr=aggr)
    grads = {"bias": gr["bias"], "root": gr.get("root")}
    if comp is None:
        grads["weight"] = gr["weight"]
    else:
        dv, dc = torch.autograd.grad(wfull, (w, comp), torch.from_numpy(gr["weight"]))
        grads["weight"], grads["comp"] = dv.numpy(), dc.numpy()
    return out, grads


def _run(conv, x, ei, et, g):
    for p in conv.parameters():
        p.grad = None
    out = conv(x, ei, et)
    out.backward(g)
    torch.cuda.synchronize()
    return out.detach().cpu(), {k: p.grad.detach().cpu().clone() for k, p in conv.named_parameters()}


CASES = [(idx, mode, aggr, rb) for idx in (False, True) for mode in ("full", "basis") for aggr in ("mean", "sum")
         for rb in (True, False)]
WIDTH = {("full", "mean"): 16, ("full", "sum"): 12, ("basis", "mean"): 40, ("basis", "sum"): 7}


@pytest.mark.parametrize("indexed,mode,aggr,root_bias", CASES)
def test_featureless_against_fp64(dev, indexed, mode, aggr, root_bias):
    from scaling_rgcn_training_amd.conv import RGCNConv
    n, r = 300, 6
    in_rows = 120 if indexed else n
    dout = WIDTH[(mode, aggr)]
    ei, et = _graph(n, 2500, r, seed=7)
    torch.manual_seed(11)
    conv = RGCNConv(in_rows, dout, r, num_bases=3 if mode == "basis" else None, aggr=aggr, root_weight=root_bias,
                    bias=root_bias, featureless=True).to(dev)
    if root_bias:
        with torch.no_grad():
            conv.bias.uniform_(-1, 1)
    x = None
    if indexed:
        x = torch.randint(0, in_rows - 10, (n,), generator=torch.Generator().manual_seed(5))   # repeats; 10 rows unused
        assert x.unique().numel() < n
    g = torch.randn(n, dout, generator=torch.Generator().manual_seed(9))
    xd = None if x is None else x.to(dev)
    eid, etd = ei.to(dev), et.to(dev)
    out, grads = _run(conv, xd, eid, etd, g.to(dev))
    assert out.shape == (n, dout)
    xoh = np.eye(in_rows) if x is None else torch.nn.functional.one_hot(x, in_rows).double().numpy()
    params = (conv.weight, conv.comp, conv.root, conv.bias)
    p_cpu = tuple(None if p is None else p.cpu() for p in params)
    ref, rg = _reference(xoh, ei, et, p_cpu, r, in_rows, dout, g, aggr)
    c_out, cg = _reference(xoh, ei, et, p_cpu, r, in_rows, dout, g, aggr, absolute=True)
    tag = f"{'idx' if indexed else 'none'}/{mode}/{aggr}/{root_bias}"
    assert_close(out.numpy(), ref, c_out, f"featureless out {tag}")
    assert_close(grads["weight"].numpy(), rg["weight"], cg["weight"], f"featureless d_weight {tag}")
    if mode == "basis":
        assert_close(grads["comp"].numpy(), rg["comp"], cg["comp"], f"featureless d_comp {tag}")
    if root_bias:
        assert_close(grads["root"].numpy(), rg["root"], cg["root"], f"featureless d_root {tag}")
        assert_close(grads["bias"].numpy(), rg["bias"], cg["bias"], f"featureless d_bias {tag}")
    # a relation without edges and table rows no node gathers: exact zeros in the dense gradient
    if mode == "full":
        assert torch.all(grads["weight"][r - 1] == 0)
    # the backward is bit-reproducible
    out2, grads2 = _run(conv, xd, eid, etd, g.to(dev))
    assert torch.equal(out, out2)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k


def test_featureless_widest_layer(dev):
    """out = 128 (32 lanes per slot, two slots per pass), x = None, full weights"""
    from scaling_rgcn_training_amd.conv import RGCNConv
    n, r, dout = 200, 4, 128
    ei, et = _graph(n, 1500, r, seed=3)
    torch.manual_seed(2)
    conv = RGCNConv(n, dout, r, featureless=True).to(dev)
    g = torch.randn(n, dout, generator=torch.Generator().manual_seed(1))
    out, grads = _run(conv, None, ei.to(dev), et.to(dev), g.to(dev))
    p_cpu = (conv.weight.cpu(), None, conv.root.cpu(), conv.bias.cpu())
    ref, rg = _reference(np.eye(n), ei, et, p_cpu, r, n, dout, g, "mean")
    c_out, cg = _reference(np.eye(n), ei, et, p_cpu, r, n, dout, g, "mean", absolute=True)
    assert_close(out.numpy(), ref, c_out, "featureless out 128")
    for k in ("weight", "root", "bias"):
        assert_close(grads[k].numpy(), rg[k], cg[k], f"featureless d_{k} 128")


def test_out_of_range_node_index_raises(dev):
    from scaling_rgcn_training_amd.conv import RGCNConv
    conv = RGCNConv(50, 8, 3, featureless=True).to(dev)
    ei = torch.tensor([[0, 1], [1, 2]], device=dev)
    et = torch.tensor([0, 1], device=dev)
    with pytest.raises(ValueError):
        conv(torch.tensor([0, 50, 3], device=dev), ei, et)
    with pytest.raises(ValueError):
        conv(torch.tensor([0, -1, 3], device=dev), ei, et)
    from scaling_rgcn_training_amd._lib import RgcnLibraryError
    with pytest.raises((ValueError, RgcnLibraryError)):     # x = None: N = in_channels, edges past it are out of range
        conv(None, torch.tensor([[0, 60], [1, 2]], device=dev), et)


def test_aifb_shaped_training_loss_falls(dev):
    """AIFB's shape (8,285 nodes, 90 relations, 16 wide): a featureless layer, ReLU, a 16 -> 4 layer; a few Adam steps"""
    from scaling_rgcn_training_amd.conv import RGCNConv
    n, r, e = 8285, 90, 58000
    g = torch.Generator().manual_seed(0)
    ei = torch.stack([torch.randint(0, n, (e,), generator=g), torch.randint(0, n, (e,), generator=g)]).to(dev)
    et = torch.randint(0, r, (e,), generator=g).to(dev)
    labelled = torch.randperm(n, generator=g)[:176].to(dev)
    y = torch.randint(0, 4, (176,), generator=g).to(dev)
    torch.manual_seed(0)
    l1 = RGCNConv(n, 16, r, featureless=True).to(dev)
    l2 = RGCNConv(16, 4, r).to(dev)
    opt = torch.optim.Adam(list(l1.parameters()) + list(l2.parameters()), lr=0.01)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        h = torch.relu(l1(None, ei, et))
        loss = torch.nn.functional.cross_entropy(l2(h, ei, et)[labelled], y)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] - 0.05, losses


def test_table_offsets_past_4_gib(dev):
    """R * in * out * 4 > 4 GiB: rows of the last relation gathered from past the 4 GiB offset (64-bit addressing), against an
    fp64 sum of the gathered rows only"""
    from scaling_rgcn_training_amd.conv import RGCNConv
    r, in_rows, dout, n = 4, 2_500_000, 128, 64
    assert r * in_rows * dout * 4 > (4 << 30)
    conv = RGCNConv(in_rows, dout, r, aggr="sum", root_weight=False, bias=False, featureless=True).to(dev)
    gen = torch.Generator().manual_seed(4)
    x = torch.randint(in_rows - 100_000, in_rows, (n,), generator=gen)
    assert (r - 1) * in_rows * dout * 4 + int(x.min()) * dout * 4 > (4 << 30)
    src = torch.randint(0, n, (400,), generator=gen)
    dst = torch.randint(0, n, (400,), generator=gen)
    typ = torch.full((400,), r - 1, dtype=torch.int64)
    typ[:40] = 0
    xd = x.to(dev)
    out = conv(xd, torch.stack([src, dst]).to(dev), typ.to(dev))
    gout = torch.randn(n, dout, generator=gen)
    out.backward(gout.to(dev))
    torch.cuda.synchronize()
    rows = conv.weight.detach()[typ.to(dev), xd[src.to(dev)]].cpu().double()        # the gathered rows only
    ref = torch.zeros(n, dout, dtype=torch.float64).index_add_(0, dst, rows)
    cond = torch.zeros(n, dout, dtype=torch.float64).index_add_(0, dst, rows.abs())
    assert_close(out.detach().cpu().numpy(), ref.numpy(), cond.numpy(), "featureless out past 4 GiB")
    # d_weight at the gathered rows of the last relation: sum over the edges of g[dst]
    dw = conv.weight.grad
    keys = x[src[40:]]
    refw = torch.zeros(in_rows, dout, dtype=torch.float64)
    refw.index_add_(0, keys, gout.double()[dst[40:]])
    uk = keys.unique()
    got = dw[r - 1, uk.to(dev)].cpu().double()
    cw = torch.zeros(in_rows, dout, dtype=torch.float64).index_add_(0, keys, gout.double().abs()[dst[40:]])
    assert_close(got.numpy(), refw[uk].numpy(), cw[uk].numpy(), "featureless d_weight past 4 GiB")
    del conv, out, dw
    torch.cuda.empty_cache()


def test_basis_weights_are_never_materialised(dev):
    from scaling_rgcn_training_amd.conv import RGCNConv
    n, r, dout, e = 20000, 200, 16, 100_000
    dense_bytes = r * n * dout * 4
    gen = torch.Generator().manual_seed(8)
    ei = torch.randint(0, n, (2, e), generator=gen).to(dev)
    et = torch.randint(0, r, (e,), generator=gen).to(dev)
    conv = RGCNConv(n, dout, r, num_bases=2, featureless=True).to(dev)
    conv(None, ei, et).sum().backward()          # plans built outside the measurement
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    for p in conv.parameters():
        p.grad = None
    conv(None, ei, et).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < dense_bytes / 8, (peak, dense_bytes)
