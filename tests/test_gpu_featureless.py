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
    return out.detach().cpu(), {k: p.grad.detach().cpu().clone() for k, p in conv.named_parameters() if p.requires_grad}


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


# ---- against the sparse fp64 reference (oracle.featureless_reference): tiles above 16, hubs, long reduction loops ------------
def _layer(in_rows, dout, r, nb, aggr, seed, root_bias=True):
    from scaling_rgcn_training_amd.conv import RGCNConv
    torch.manual_seed(seed)
    conv = RGCNConv(in_rows, dout, r, num_bases=nb, aggr=aggr, root_weight=root_bias, bias=root_bias, featureless=True).cuda()
    if root_bias:
        with torch.no_grad():
            conv.bias.uniform_(-1, 1)
    return conv


def _run_dev(conv, x, ei, et, g):
    """(out, grads) with the gradients left on the device"""
    for p in conv.parameters():
        p.grad = None
    out = conv(x, ei, et)
    out.backward(g)
    torch.cuda.synchronize()
    return out.detach(), {k: p.grad for k, p in conv.named_parameters()}


def _check_sparse(conv, x, ei, et, g, aggr, tag, got=None):
    """output and every gradient against the sparse reference; the rows of d_weight (d_bases) no edge gathers: exact zeros,
    checked on the device.  Returns the device results."""
    dev = torch.device("cuda:0")
    xd = None if x is None else x.to(dev)
    if got is None:
        got = _run_dev(conv, xd, ei.to(dev), et.to(dev), g.to(dev))
    out, grads = got
    p = {k: None if v is None else v.detach().cpu() for k, v in
         (("weight", conv.weight), ("comp", conv.comp), ("root", conv.root), ("bias", conv.bias))}
    ref, cond = O.featureless_reference(x, ei, et, p["weight"], p["comp"], p["root"], p["bias"], g, aggr, dense=False)
    assert_close(out.cpu().numpy(), ref["out"].numpy(), cond["out"].numpy(), f"featureless out {tag}")
    dw = grads["weight"].view(-1, conv.out_channels)
    rows = ref["weight_rows"].to(dev)
    assert_close(dw[rows].cpu().numpy(), ref["weight"].numpy(), cond["weight"].numpy(), f"featureless d_weight rows {tag}")
    nz = (dw != 0).any(1)
    nz[rows] = False
    assert not bool(nz.any()), f"{tag}: {int(nz.sum())} d_weight rows no edge gathers are not zero"
    for k in ("comp", "root", "bias"):
        if p[k] is not None:
            assert_close(grads[k].cpu().numpy(), ref[k].numpy(), cond[k].numpy(), f"featureless d_{k} {tag}")
    return got


def _big_graph(n, e, r, seed):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, n, (e,), generator=g)
    typ = torch.randint(0, r - 1, (e,), generator=g)          # relation r - 1 without edges
    return torch.stack([src, dst]), typ


# (n, out, bases, aggr, in_rows of an integer x or None) -> the tile rgcn_featureless_geometry picks.  No n is a multiple of
# its tile; every case has thousands of tiles and, per relation, hundreds of units (fl_bias_reduce / fl_comp_reduce loops).
TILE_CASES = {
    (600_000, 16, None, "mean", None): 128,
    (400_000, 16, None, "sum", 150_000): 96,
    (270_000, 24, 2, "mean", 40_000): 64,          # L = 8
    (200_000, 24, None, "sum", None): 48,          # L = 8
    (140_010, 100, None, "mean", None): 32,        # L = 32
    (300_017, 40, 2, "sum", None): 32,             # L = 16
}


@pytest.mark.parametrize("key", list(TILE_CASES), ids=lambda k: "n%d-out%d-b%s-%s-x%s" % k)
def test_featureless_tiles_against_sparse_fp64(dev, key):
    from scaling_rgcn_training_amd import _lib
    n, dout, nb, aggr, in_rows = key
    tile = TILE_CASES[key]
    assert _lib.featureless_geometry(n, dout, nb or 0) == (tile, 64)
    assert n % tile != 0
    r = 4
    ei, et = _big_graph(n, 2 * n, r, seed=n % 1000)
    x = None
    if in_rows is not None:
        x = torch.randint(0, in_rows - 10, (n,), generator=torch.Generator().manual_seed(3))
    conv = _layer(in_rows or n, dout, r, nb, aggr, seed=dout)
    g = torch.randn(n, dout, generator=torch.Generator().manual_seed(6))
    out, grads = _check_sparse(conv, x, ei, et, g, aggr, f"tile {tile}")
    if tile == 128:                 # bit-reproducible at the largest tile as well
        out2, grads2 = _run_dev(conv, None if x is None else x.to(dev), ei.to(dev), et.to(dev), g.to(dev))
        assert torch.equal(out, out2)
        for k in grads:
            assert torch.equal(grads[k], grads2[k]), k
    del conv, out, grads
    torch.cuda.empty_cache()


WIDTHS = [1, 3, 4, 5, 16, 17, 31, 32, 33, 64, 65, 127]


@pytest.mark.parametrize("mode", ["full", "basis"])
@pytest.mark.parametrize("dout", WIDTHS)
def test_featureless_width_sweep(dev, dout, mode):
    """both sides of every lanes-per-slot boundary (out 16 / 32 / 64) and of dout % 4; full weights with x = None and mean,
    bases with an integer x and sum; against the dense fp64 oracle at x = one_hot(x)"""
    n, r = 150, 4
    aggr = "mean" if mode == "full" else "sum"
    in_rows = n if mode == "full" else 70
    ei, et = _graph(n, 1200, r, seed=dout)
    conv = _layer(in_rows, dout, r, 2 if mode == "basis" else None, aggr, seed=dout)
    x = None if mode == "full" else torch.randint(0, in_rows - 5, (n,), generator=torch.Generator().manual_seed(dout))
    g = torch.randn(n, dout, generator=torch.Generator().manual_seed(dout + 1))
    out, grads = _run(conv, None if x is None else x.to(dev), ei.to(dev), et.to(dev), g.to(dev))
    xoh = np.eye(n) if x is None else torch.nn.functional.one_hot(x, in_rows).double().numpy()
    p_cpu = tuple(None if p is None else p.detach().cpu() for p in (conv.weight, conv.comp, conv.root, conv.bias))
    ref, rg = _reference(xoh, ei, et, p_cpu, r, in_rows, dout, g, aggr)
    c_out, cg = _reference(xoh, ei, et, p_cpu, r, in_rows, dout, g, aggr, absolute=True)
    assert_close(out.numpy(), ref, c_out, f"featureless out {mode} {dout}")
    for k in ("weight", "comp", "root", "bias"):
        if k in grads:
            assert_close(grads[k].numpy(), rg[k], cg[k], f"featureless d_{k} {mode} {dout}")


@pytest.mark.parametrize("mode,indexed", [("full", False), ("full", True), ("basis", False), ("basis", True)])
def test_featureless_hubs(dev, mode, indexed):
    """a destination with 5,000 in-edges of one relation (its run crosses row tiles, unroll groups and ~80 chunks of the
    forward walk), a source with 5,000 out-edges (the same in the transposed walk), and under integer x one table row shared
    by 1,000 nodes"""
    n, r, dout = 6000, 3, 33 if mode == "basis" else 16
    gen = torch.Generator().manual_seed(12)
    ei, et = _big_graph(n, 12_000, r, seed=12)
    hub_in = torch.stack([torch.randint(0, n, (5000,), generator=gen), torch.full((5000,), 17)])
    hub_out = torch.stack([torch.full((5000,), 23), torch.randint(0, n, (5000,), generator=gen)])
    ei = torch.cat([ei, hub_in, hub_out], 1)
    et = torch.cat([et, torch.full((5000,), 1), torch.zeros(5000, dtype=torch.int64)])
    in_rows, x = n, None
    if indexed:
        in_rows = 2500
        x = torch.randint(0, in_rows, (n,), generator=gen)
        x[torch.randperm(n, generator=gen)[:1000]] = 7
        assert int((x == 7).sum()) >= 1000
    conv = _layer(in_rows, dout, r, 2 if mode == "basis" else None, "mean", seed=4)
    g = torch.randn(n, dout, generator=gen)
    _check_sparse(conv, x, ei, et, g, "mean", f"hubs {mode} indexed={indexed}")


@pytest.mark.parametrize("indexed", [False, True], ids=["x-none", "x-index"])
def test_featureless_gradient_subsets_are_bit_identical(dev, indexed):
    """freeze weight, then comp, then root, then everything but bias: every gradient still computed equals the one of the
    all-gradients call bit for bit"""
    n, r, dout = 900, 5, 20
    ei, et = _graph(n, 6000, r, seed=31)
    in_rows = 400 if indexed else n
    x = torch.randint(0, in_rows, (n,), generator=torch.Generator().manual_seed(2)).to(dev) if indexed else None
    conv = _layer(in_rows, dout, r, 3, "mean", seed=5)
    g = torch.randn(n, dout, generator=torch.Generator().manual_seed(8)).to(dev)
    eid, etd = ei.to(dev), et.to(dev)
    out, full = _run(conv, x, eid, etd, g)
    names = [k for k, _ in conv.named_parameters()]
    assert set(names) == {"weight", "comp", "root", "bias"}
    for frozen in (["weight"], ["comp"], ["root"], ["weight", "comp", "root"]):
        for k, p in conv.named_parameters():
            p.requires_grad_(k not in frozen)
        out2, sub = _run(conv, x, eid, etd, g)
        assert torch.equal(out, out2)
        assert set(sub) == set(names) - set(frozen), (frozen, set(sub))
        for k in sub:
            assert torch.equal(sub[k], full[k]), (frozen, k)
    for p in conv.parameters():
        p.requires_grad_(True)


@pytest.mark.parametrize("mode", ["full", "basis"])
def test_featureless_index_identities(dev, mode):
    """bit for bit: x = arange(N) is x = None; x = perm with tables T is x = None with the row-permuted tables T[:, perm]
    (gradients un-permuted)"""
    n, r, dout = 700, 4, 12
    nb = 3 if mode == "basis" else None
    ei, et = _graph(n, 5000, r, seed=41)
    eid, etd = ei.to(dev), et.to(dev)
    g = torch.randn(n, dout, generator=torch.Generator().manual_seed(1)).to(dev)
    conv = _layer(n, dout, r, nb, "mean", seed=9)
    out0, gr0 = _run(conv, None, eid, etd, g)
    out1, gr1 = _run(conv, torch.arange(n, device=dev), eid, etd, g)
    assert torch.equal(out0, out1)
    assert set(gr0) == set(gr1)
    for k in gr0:
        assert torch.equal(gr0[k], gr1[k]), k
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(4)).to(dev)
    outp, grp = _run(conv, perm, eid, etd, g)
    convp = _layer(n, dout, r, nb, "mean", seed=9)
    with torch.no_grad():
        convp.weight.copy_(conv.weight[:, perm])
        convp.root.copy_(conv.root[perm])
        convp.bias.copy_(conv.bias)
        if nb:
            convp.comp.copy_(conv.comp)
    outq, grq = _run(convp, None, eid, etd, g)
    assert torch.equal(outp, outq)
    inv = torch.argsort(perm).cpu()
    assert torch.equal(grp["weight"], grq["weight"][:, inv])
    assert torch.equal(grp["root"], grq["root"][inv])
    assert torch.equal(grp["bias"], grq["bias"])
    if nb:
        assert torch.equal(grp["comp"], grq["comp"])


def test_featureless_one_basis_of_ones_is_full_weights(dev):
    """B = 1, comp = 1: W_r = V for every r.  The output equals full weights [V] * R bit for bit; d_bases is the sum of the
    full d_weight over relations in relation order"""
    n, r, dout = 500, 4, 24
    ei, et = _graph(n, 4000, r, seed=5)
    eid, etd = ei.to(dev), et.to(dev)
    g = torch.randn(n, dout, generator=torch.Generator().manual_seed(2)).to(dev)
    basis = _layer(n, dout, r, 1, "mean", seed=3)
    full = _layer(n, dout, r, None, "mean", seed=3)
    with torch.no_grad():
        basis.comp.fill_(1.0)
        full.weight.copy_(basis.weight.expand(r, n, dout))
        full.root.copy_(basis.root)
        full.bias.copy_(basis.bias)
    ob, gb = _run(basis, None, eid, etd, g)
    of, gf = _run(full, None, eid, etd, g)
    assert torch.equal(ob, of)
    acc = torch.zeros(n, dout)
    for rel in range(r):
        acc = acc + gf["weight"][rel]
    assert torch.equal(gb["weight"][0], acc)
    assert torch.equal(gb["root"], gf["root"]) and torch.equal(gb["bias"], gf["bias"])


def test_featureless_degenerate_graphs(dev):
    """E = 0: out = bias + root[x], d_weight zeros, d_root = g summed per row.  N = 1.  in_channels = 1 (one table row shared
    by every node)."""
    from scaling_rgcn_training_amd.conv import RGCNConv
    n, r, dout = 300, 3, 10
    g = torch.randn(n, dout, generator=torch.Generator().manual_seed(3))
    empty_ei, empty_et = torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)
    for mode in ("full", "basis"):
        for x in (None, torch.randint(0, 50, (n,), generator=torch.Generator().manual_seed(1))):
            conv = _layer(n if x is None else 50, dout, r, 2 if mode == "basis" else None, "mean", seed=2)
            xd = None if x is None else x.to(dev)
            out, grads = _run(conv, xd, empty_ei.to(dev), empty_et.to(dev), g.to(dev))
            rows = torch.arange(n) if x is None else x
            assert torch.equal(out, conv.root.detach().cpu()[rows] + conv.bias.detach().cpu()), mode
            assert bool((grads["weight"] == 0).all())
            if mode == "basis":
                assert bool((grads["comp"] == 0).all())
            _check_sparse(conv, x, empty_ei, empty_et, g, "mean", f"E = 0 {mode}")
    # one node, a self loop
    conv = _layer(1, 7, 2, None, "sum", seed=1)
    ei, et = torch.zeros(2, 1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
    _check_sparse(conv, None, ei, et, torch.randn(1, 7), "sum", "N = 1")
    # in_channels = 1: every node gathers row 0
    ei, et = _graph(n, 2000, r, seed=3)
    for nb in (None, 2):
        conv = RGCNConv(1, dout, r, num_bases=nb, featureless=True).to(dev)
        _check_sparse(conv, torch.zeros(n, dtype=torch.int64), ei, et, g, "mean", f"in_channels = 1 bases={nb}")
