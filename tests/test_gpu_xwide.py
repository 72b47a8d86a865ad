"""RGCNConv wider than 128 on the GPU (``wide=True``, csrc/rgcn_xwide.hip): output, dX, d_weight (dense, basis, blocks), d_root
and d_bias against the fp64 dense oracle under oracle/tolerance.py (bound (1) with the condition sums, and no worse than 2 x the
fp32 CPU loop), at widths up to 512 per side, on graphs with duplicate triples, self loops, an empty relation, isolated nodes,
no edges at all and a hub of in-degree > 10^4.  Also: the raw entry points against rgcn_fwd / rgcn_bwd_dx / rgcn_bwd_dw at 64 and
128, fused activations in the model wrappers, bit-reproducibility, hipGraph capture, Trainer epochs, matrices past 4 GiB, and
narrow layers unchanged by the flag."""
import numpy as np
import pytest
import torch

from oracle import rgcn_oracle as O
from oracle.tolerance import U32, abs_condition, assert_close, cpu32_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from scaling_rgcn_training_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _graph(n, e, r, seed, hub=0):
    """random edges among the first n - 20 nodes (the last 20 isolated), relation r - 1 without edges, 40 self loops, the first
    200 triples repeated; ``hub``: that many more edges into node 0 (relation 0)"""
    g = torch.Generator().manual_seed(seed)
    m = n - 20
    src = torch.randint(0, m, (e,), generator=g)
    dst = torch.randint(0, m, (e,), generator=g)
    typ = torch.randint(0, r - 1, (e,), generator=g)
    loops = torch.arange(40)
    src, dst, typ = torch.cat([src, loops]), torch.cat([dst, loops]), torch.cat([typ, loops % (r - 1)])
    src, dst, typ = torch.cat([src, src[:200]]), torch.cat([dst, dst[:200]]), torch.cat([typ, typ[:200]])
    if hub:
        src = torch.cat([src, torch.randint(0, m, (hub,), generator=g)])
        dst = torch.cat([dst, torch.zeros(hub, dtype=torch.int64)])
        typ = torch.cat([typ, torch.zeros(hub, dtype=torch.int64)])
    return torch.stack([src, dst]), typ


def _layer(din, dout, r, mode, aggr, root_bias, seed):
    from scaling_rgcn_training_amd.conv import RGCNConv
    kw = {"full": {}, "basis": {"num_bases": 3}}[mode] if mode != "block" else {"num_blocks": _blocks(din, dout)}
    torch.manual_seed(seed)
    conv = RGCNConv(din, dout, r, aggr=aggr, root_weight=root_bias, bias=root_bias, wide=True, **kw)
    if root_bias:
        with torch.no_grad():
            conv.bias.uniform_(-1, 1)
    return conv


def _blocks(din, dout):
    for nb in (4, 3, 8, 2):
        if din % nb == 0 and dout % nb == 0:
            return nb
    raise ValueError((din, dout))


def _run(conv, x, ei, et, g, dev):
    for p in conv.parameters():
        p.grad = None
    xd = x.to(dev).requires_grad_(True)
    out = conv(xd, ei.to(dev), et.to(dev))
    out.backward(g.to(dev))
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu().clone() for k, p in conv.named_parameters() if p.requires_grad}
    return out.detach().cpu(), xd.grad.detach().cpu(), grads


def _check(conv, x, ei, et, g, out, dx, grads, aggr, tag):
    """every output against the fp64 dense oracle of the equivalent dense layer; a decomposition's gradients pushed from the
    dense d_W through ``effective_weight`` by fp64 autograd (their condition: the same on absolute values)"""
    r, din, dout = conv.num_relations, conv.in_channels, conv.out_channels
    w = conv.weight.detach().cpu().double()
    comp = None if conv.comp is None else conv.comp.detach().cpu().double()
    root = None if conv.root is None else conv.root.detach().cpu().double().numpy()
    bias = None if conv.bias is None else conv.bias.detach().cpu().double().numpy()
    wf = O.effective_weight(w, comp, r, conv.num_blocks, din, dout).numpy()
    xn, gn, ein, etn = x.double().numpy(), g.double().numpy(), ei.numpy(), et.numpy()
    ref = O.rgcn_conv_dense(xn, ein, etn, wf, root, bias, aggr=aggr)
    rg = O.rgcn_conv_grads_dense(xn, ein, etn, wf, root, gn, aggr=aggr)
    c_out, cg = abs_condition(xn, ein, etn, wf, root, bias, gn, aggr=aggr)
    cpu_out, cpu_g = cpu32_reference(xn, ein, etn, wf, root, bias, gn, aggr=aggr)
    assert_close(out.numpy(), ref, c_out, f"xwide out {tag}", cpu32=cpu_out)
    assert_close(dx.numpy(), rg["x"], cg["x"], f"xwide d_x {tag}", cpu32=cpu_g["x"])
    if conv.root is not None and "root" in grads:
        assert_close(grads["root"].numpy(), rg["root"], cg["root"], f"xwide d_root {tag}", cpu32=cpu_g["root"])
    if conv.bias is not None and "bias" in grads:
        assert_close(grads["bias"].numpy(), rg["bias"], cg["bias"], f"xwide d_bias {tag}", cpu32=cpu_g["bias"])
    if "weight" not in grads and "comp" not in grads:
        return
    if conv.comp is None and conv.num_blocks is None:
        assert_close(grads["weight"].numpy(), rg["weight"], cg["weight"], f"xwide d_weight {tag}", cpu32=cpu_g["weight"])
        return

    def push(wv, cv, dw):
        wv = wv.clone().requires_grad_(True)
        cv = None if cv is None else cv.clone().requires_grad_(True)
        full = O.effective_weight(wv, cv, r, conv.num_blocks, din, dout)
        return torch.autograd.grad(full, [t for t in (wv, cv) if t is not None], torch.from_numpy(dw))

    want = push(w, comp, rg["weight"])
    cond = push(w.abs(), None if comp is None else comp.abs(), np.abs(cg["weight"]))
    if "weight" in grads:
        assert_close(grads["weight"].numpy(), want[0].numpy(), cond[0].numpy(), f"xwide d_weight {tag}")
    if "comp" in grads:
        assert_close(grads["comp"].numpy(), want[1].numpy(), cond[1].numpy(), f"xwide d_comp {tag}")


CASES = [((129, 129), "mean", True, "full"), ((129, 129), "sum", False, "block"),
         ((255, 256), "mean", True, "basis"), ((255, 256), "sum", True, "full"),
         ((256, 16), "mean", False, "full"), ((256, 16), "sum", True, "block"),
         ((16, 256), "mean", True, "block"), ((16, 256), "sum", False, "basis"),
         ((512, 512), "mean", True, "full"), ((512, 512), "sum", True, "basis"),
         ((512, 64), "mean", True, "full"), ((512, 64), "sum", False, "block"),
         ((64, 512), "mean", True, "basis"), ((64, 512), "sum", True, "full"),
         ((200, 7), "mean", True, "full"), ((200, 7), "sum", True, "basis"),
         ((7, 300), "mean", False, "full"), ((7, 300), "sum", True, "full")]


@pytest.mark.parametrize("widths,aggr,root_bias,mode", CASES)
def test_xwide_against_fp64(dev, widths, aggr, root_bias, mode):
    din, dout = widths
    n, r = 300, 5
    ei, et = _graph(n, 2500, r, seed=din + dout)
    conv = _layer(din, dout, r, mode, aggr, root_bias, seed=1).to(dev)
    assert conv.xwide
    gen = torch.Generator().manual_seed(9)
    x, g = torch.randn(n, din, generator=gen), torch.randn(n, dout, generator=gen)
    out, dx, grads = _run(conv, x, ei, et, g, dev)
    assert out.shape == (n, dout) and dx.shape == (n, din)
    _check(conv, x, ei, et, g, out, dx, grads, aggr, f"{din}x{dout}/{aggr}/{root_bias}/{mode}")
    if mode == "full":
        assert torch.all(grads["weight"][r - 1] == 0)         # the relation without edges
    # bit-reproducible
    out2, dx2, grads2 = _run(conv, x, ei, et, g, dev)
    assert torch.equal(out, out2) and torch.equal(dx, dx2)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k


@pytest.mark.parametrize("mode", ["full", "basis"])
def test_frozen_parameters(dev, mode):
    din, dout, n, r = 255, 256, 300, 5
    ei, et = _graph(n, 2500, r, seed=4)
    gen = torch.Generator().manual_seed(3)
    x, g = torch.randn(n, din, generator=gen), torch.randn(n, dout, generator=gen)
    for frozen in (("weight",), ("root", "bias"), ("weight", "root", "bias") + (("comp",) if mode == "basis" else ())):
        conv = _layer(din, dout, r, mode, "mean", True, seed=2).to(dev)
        for k in frozen:
            getattr(conv, k).requires_grad_(False)
        out, dx, grads = _run(conv, x, ei, et, g, dev)
        assert not set(frozen) & set(grads)
        assert all(getattr(conv, k).grad is None for k in frozen)
        _check(conv, x, ei, et, g, out, dx, grads, "mean", f"frozen {frozen} {mode}")


def test_edgeless_graph(dev):
    n, r, din, dout = 200, 3, 300, 140
    ei, et = torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)
    conv = _layer(din, dout, r, "full", "mean", True, seed=5).to(dev)
    gen = torch.Generator().manual_seed(5)
    x, g = torch.randn(n, din, generator=gen), torch.randn(n, dout, generator=gen)
    out, dx, grads = _run(conv, x, ei, et, g, dev)
    _check(conv, x, ei, et, g, out, dx, grads, "mean", "edgeless")
    assert torch.all(grads["weight"] == 0)


@pytest.mark.parametrize("widths,aggr", [((300, 129), "mean"), ((129, 512), "sum")])
def test_hub_spans_many_chunks(dev, widths, aggr):
    """node 0 gathers 10,500 edges of relation 0: its (tile, relation) group spans more than 160 chunks"""
    din, dout = widths
    n, r = 600, 4
    ei, et = _graph(n, 3000, r, seed=6, hub=10_500)
    assert int(((ei[1] == 0) & (et == 0)).sum()) >= 10_000
    conv = _layer(din, dout, r, "full", aggr, True, seed=6).to(dev)
    gen = torch.Generator().manual_seed(6)
    x, g = torch.randn(n, din, generator=gen), torch.randn(n, dout, generator=gen)
    out, dx, grads = _run(conv, x, ei, et, g, dev)
    _check(conv, x, ei, et, g, out, dx, grads, aggr, f"hub {din}x{dout}/{aggr}")


def _plans(ei, et, n, r, din, dout, aggr="mean"):
    from scaling_rgcn_training_amd import _lib
    from scaling_rgcn_training_amd.plan import cached_graph_plans
    tile, chunk = _lib.xwide_geometry(n, din, dout)
    return cached_graph_plans(ei, et, n, r, tile, aggr, chunk=chunk, split=False, dw_tiles=False, paths=("ring", "ring"),
                              extra_key=("xwide",))


@pytest.mark.parametrize("width", [64, 128])
def test_cross_check_against_the_narrow_kernels(dev, width):
    """rgcn_xwide_* and rgcn_fwd / rgcn_bwd_dx (FLAG_EXACT_FP32) / rgcn_bwd_dw on the same plans: both within the oracle's bound"""
    from scaling_rgcn_training_amd import _lib
    n, r = 300, 5
    ei, et = _graph(n, 2500, r, seed=width)
    eid, etd = ei.to(dev), et.to(dev)
    plans = _plans(eid, etd, n, r, width, width)
    w, root, bias = O.synthetic_params(r, width, width, seed=1)
    gen = torch.Generator().manual_seed(7)
    x, g = torch.randn(n, width, generator=gen), torch.randn(n, width, generator=gen)
    xd, gd, wd, rd, bd = (t.to(dev).contiguous() for t in (x, g, w, root, bias))
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    op = torch.cat([wd, rd[None]]).contiguous()
    opt = op.transpose(1, 2).contiguous()
    fp, bp = _lib.plan_struct(plans.fwd), _lib.plan_struct(plans.bwd)
    res = {}
    o1, o2, d1, d2 = nan(n, width), nan(n, width), nan(n, width), nan(n, width)
    _lib.xwide_fwd(fp, xd, width, op, bd, o1, width)
    _lib.fwd(fp, xd, width, _lib.pack_weights(wd, rd, False), bd, o2, width, _lib.ACT_NONE, _lib.FLAG_EXACT_FP32)
    _lib.xwide_bwd_dx(bp, gd, width, opt, d1, width)
    _lib.bwd_dx(bp, gd, width, _lib.pack_weights(wd, rd, True), d2, width, None, _lib.FLAG_EXACT_FP32)
    w1, r1, b1 = nan(r, width, width), nan(width, width), nan(width)
    w2, r2, b2 = nan(r, width, width), nan(width, width), nan(width)
    _lib.xwide_bwd_dw(fp, xd, width, gd, width, w1, r1, b1)
    _lib.bwd_dw(fp, xd, width, gd, width, w2, r2, b2)
    torch.cuda.synchronize()
    xn, gn, wn, rn, bn = (t.double().numpy() for t in (x, g, w, root, bias))
    ref = O.rgcn_conv_dense(xn, ei.numpy(), et.numpy(), wn, rn, bn)
    rg = O.rgcn_conv_grads_dense(xn, ei.numpy(), et.numpy(), wn, rn, gn)
    c_out, cg = abs_condition(xn, ei.numpy(), et.numpy(), wn, rn, bn, gn)
    cpu_out, cpu_g = cpu32_reference(xn, ei.numpy(), et.numpy(), wn, rn, bn, gn)
    for tag, (o, d, dw_, dr_, db_) in (("xwide", (o1, d1, w1, r1, b1)), ("narrow", (o2, d2, w2, r2, b2))):
        assert_close(o.cpu().numpy(), ref, c_out, f"{tag} {width} out", cpu32=cpu_out)
        assert_close(d.cpu().numpy(), rg["x"], cg["x"], f"{tag} {width} d_x", cpu32=cpu_g["x"])
        assert_close(dw_.cpu().numpy(), rg["weight"], cg["weight"], f"{tag} {width} d_weight", cpu32=cpu_g["weight"])
        assert_close(dr_.cpu().numpy(), rg["root"], cg["root"], f"{tag} {width} d_root", cpu32=cpu_g["root"])
        assert_close(db_.cpu().numpy(), rg["bias"], cg["bias"], f"{tag} {width} d_bias", cpu32=cpu_g["bias"])
    # and against each other, elementwise within the same bound
    assert_close(o1.cpu().numpy(), o2.cpu().double().numpy(), c_out, f"xwide vs narrow {width} out")
    assert_close(d1.cpu().numpy(), d2.cpu().double().numpy(), cg["x"], f"xwide vs narrow {width} d_x")
    assert_close(w1.cpu().numpy(), w2.cpu().double().numpy(), cg["weight"], f"xwide vs narrow {width} d_weight")


def test_activation_epilogues_raw(dev):
    """the fused store of rgcn_xwide_fwd (ReLU, sigmoid) and the ReLU mask of rgcn_xwide_bwd_dx, against torch on the plain result"""
    from scaling_rgcn_training_amd import _lib
    n, r, din, dout = 300, 5, 255, 200
    ei, et = _graph(n, 2500, r, seed=8)
    eid, etd = ei.to(dev), et.to(dev)
    plans = _plans(eid, etd, n, r, din, dout)
    gen = torch.Generator(device=dev).manual_seed(8)
    x = torch.zeros(n, 256, device=dev)
    x[:, :din] = torch.randn(n, din, generator=gen, device=dev)
    g = torch.randn(n, dout, generator=gen, device=dev)
    op = torch.randn(r + 1, din, dout, generator=gen, device=dev) * 0.05
    opt = op.transpose(1, 2).contiguous()
    bias = torch.randn(dout, generator=gen, device=dev)
    fp, bp = _lib.plan_struct(plans.fwd), _lib.plan_struct(plans.bwd)
    outs = {}
    for act in (_lib.ACT_NONE, _lib.ACT_RELU, _lib.ACT_SIGMOID):
        outs[act] = torch.full((n, dout), float("nan"), device=dev)
        _lib.xwide_fwd(fp, x, din, op, bias, outs[act], dout, act)
    z = outs[_lib.ACT_NONE]
    assert torch.equal(outs[_lib.ACT_RELU], torch.relu(z))
    torch.testing.assert_close(outs[_lib.ACT_SIGMOID], torch.sigmoid(z), rtol=1e-6, atol=1e-7)
    d0, dm = torch.full((n, 256), float("nan"), device=dev), torch.full((n, 256), float("nan"), device=dev)
    _lib.xwide_bwd_dx(bp, g, dout, opt, d0, din)
    _lib.xwide_bwd_dx(bp, g, dout, opt, dm, din, x)
    assert torch.equal(dm, d0 * (x > 0))
    assert torch.all(d0[:, din:] == 0) and torch.all(z.isfinite())


def _emb_setup(n, r, c, seed):
    from scaling_rgcn_training_amd.data import Data
    ei, et = O.synthetic_graph(n, 8 * n, r, seed=seed)
    g = torch.Generator().manual_seed(seed)
    y = torch.nn.functional.one_hot(torch.randint(0, c, (n,), generator=g), c).float()
    perm = torch.randperm(n, generator=g)
    data = Data(edge_index=ei)
    data.edge_type = et
    data.x_train, data.y_train = perm[:400], y[perm[:400]]
    data.x_val, data.y_val = perm[400:600], y[perm[400:600]]
    return data, y, perm[:400]


@pytest.mark.parametrize("fuse", [True, False])
def test_emb_layers_wide_one_step_against_cpu_twin(dev, monkeypatch, fuse):
    """RGCN_WIDE on through the module default: Emb_Layers with emb 255 and hidden 256 builds and trains; loss and every
    parameter gradient of one step against the CPU twin (oracle convolutions, unfused tail)"""
    from scaling_rgcn_training_amd import conv as conv_mod
    from scaling_rgcn_training_amd.layers import Emb_Layers
    from tests.twins import cpu_twin
    monkeypatch.setattr(conv_mod, "_WIDE_DEFAULT", True)
    n, r, c, emb, hid = 1200, 6, 4, 255, 256
    data, y, idx = _emb_setup(n, r, c, seed=3)
    torch.manual_seed(0)
    model = Emb_Layers(r, hid, c, n, emb, None)
    assert model.rgcn1.xwide and model.rgcn2.xwide
    model.fuse_activations = fuse
    twin = cpu_twin(model)
    model = model.to(dev)
    loss = torch.nn.functional.binary_cross_entropy(model(data.to(dev), torch.sigmoid)[idx.to(dev)], y[idx].to(dev))
    loss.backward()
    c_loss = torch.nn.functional.binary_cross_entropy(twin(data, torch.sigmoid)[idx], y[idx])
    c_loss.backward()
    np.testing.assert_allclose(loss.item(), c_loss.item(), rtol=1e-5, atol=1e-6)
    cg = dict(twin.named_parameters())
    for k, p in model.named_parameters():
        a, b = p.grad.cpu().numpy(), cg[k].grad.numpy()
        np.testing.assert_allclose(a, b, rtol=2e-4, atol=2e-5 * max(1.0, float(np.abs(b).max())), err_msg=k)


def test_hipgraph_capture_replays_eager(dev):
    n, r, din, dout = 2000, 5, 255, 256
    ei, et = _graph(n, 16000, r, seed=12)
    eid, etd = ei.to(dev), et.to(dev)
    conv = _layer(din, dout, r, "full", "mean", True, seed=12).to(dev)
    gen = torch.Generator(device=dev).manual_seed(12)
    x = torch.randn(n, din, generator=gen, device=dev).requires_grad_(True)
    g = torch.randn(n, dout, generator=gen, device=dev)

    def step():
        x.grad = None
        for p in conv.parameters():
            p.grad = None
        out = conv(x, eid, etd, _activation="relu")
        out.backward(g)
        return out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = step().detach().clone()
        want = [x.grad.clone()] + [p.grad.clone() for p in conv.parameters()]
        step()
    torch.cuda.current_stream().wait_stream(side)
    x.grad = None
    for p in conv.parameters():
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = conv(x, eid, etd, _activation="relu")
        out.backward(g)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        got = [x.grad] + [p.grad for p in conv.parameters()]
        for a, b in zip(got, want):
            assert torch.equal(a, b)


def test_trainer_hipgraph_epochs_match_eager_epochs(dev, monkeypatch):
    import copy

    from scaling_rgcn_training_amd import conv as conv_mod
    from scaling_rgcn_training_amd.layers import Emb_Layers
    from scaling_rgcn_training_amd.trainer import Trainer, bce_loss
    monkeypatch.setattr(conv_mod, "_WIDE_DEFAULT", True)
    n, r, c, emb, hid = 1500, 7, 4, 200, 300
    data, _, _ = _emb_setup(n, r, c, seed=5)

    class _Graph:
        pass

    torch.manual_seed(0)
    model0 = Emb_Layers(r, hid, c, n, emb, None)
    assert model0.rgcn1.xwide and model0.rgcn2.xwide     # 200 -> 300 -> 4
    runs = {}
    for mode in (False, True):
        gobj = _Graph()
        gobj.training_data = data
        tr = Trainer(None, hid, epochs=8, emb_dim=emb, lr=0.01, weight_d=5e-5, verbose=False, hipgraph=mode)
        model = copy.deepcopy(model0)
        acc, losses, _, _ = tr.train(model, gobj, bce_loss, torch.sigmoid, sum_graph=False)
        assert tr.last_train_mode == ("hipgraph" if mode else "eager")
        runs[mode] = (acc, losses, {k: v.detach().cpu() for k, v in model.state_dict().items()})
    np.testing.assert_allclose(runs[True][1], runs[False][1], rtol=1e-5, atol=1e-6)
    assert runs[True][0] == runs[False][0]
    # parameters: Adam's first steps move an element whose gradient is ~0 by about lr * sign(gradient), so the last-bit
    # difference of the capturable Adam's bias correction flips a few of them (up to 0.5 % here); the rest agree to 1e-4
    for k in runs[True][2]:
        a, b = runs[True][2][k].numpy(), runs[False][2][k].numpy()
        off = ~np.isclose(a, b, rtol=1e-4, atol=1e-5)
        assert off.mean() < 0.01 and np.abs(a - b).max() < 8 * 0.01, (k, off.mean(), np.abs(a - b).max())
    assert runs[False][1][-1] < runs[False][1][0]


@pytest.mark.parametrize("mode", ["full", "basis"])
def test_narrow_layer_unchanged_by_the_flag(dev, mode):
    n, r = 500, 5
    ei, et = _graph(n, 4000, r, seed=13)
    gen = torch.Generator().manual_seed(13)
    x, g = torch.randn(n, 64, generator=gen), torch.randn(n, 64, generator=gen)
    from scaling_rgcn_training_amd.conv import RGCNConv
    res = []
    for wide in (False, True):
        torch.manual_seed(13)
        conv = RGCNConv(64, 64, r, num_bases=3 if mode == "basis" else None, wide=wide).to(dev)
        assert not conv.xwide
        res.append(_run(conv, x, ei, et, g, dev))
    (o0, d0, g0), (o1, d1, g1) = res
    assert torch.equal(o0, o1) and torch.equal(d0, d1)
    assert g0.keys() == g1.keys() and all(torch.equal(g0[k], g1[k]) for k in g0)


# ---- past 4 GiB ----------------------------------------------------------------------------------------------------------
def _bound1(name, got, ref, cond):
    """bound (1) of oracle/tolerance.py on every element (row blocks on the device; NaN fails)"""
    got = got[:, :ref.shape[1]] if got.dim() == 2 else got
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    bad, worst = 0, 0.0
    for lo in range(0, ref.shape[0], 1 << 20):
        sl = slice(lo, lo + (1 << 20))
        err = (got[sl].double() - ref[sl]).abs()
        tol = 1e-5 + 1e-5 * ref[sl].abs() + 4 * U32 * cond[sl]
        bad += int((~(err <= tol)).sum())
        worst = max(worst, float(torch.nan_to_num(err - tol, nan=float("inf")).max()))
    assert bad == 0, f"{name}: {bad} of {ref.numel()} elements outside bound (1), worst excess {worst:.3e}"


@pytest.mark.parametrize("din,dout", [(512, 16), (16, 512)])
def test_past_4gib(dev, din, dout):
    """2,100,000 nodes: the 512-wide side (x and dX, or out and g) passes 4 GiB; ~4.15M edges over 4 relations (one dead), the
    last row as source and destination; raw-ABI outputs start as NaN"""
    import gc

    from scaling_rgcn_training_amd import _lib
    from scaling_rgcn_training_amd.plan import clear_plan_cache
    from tests.test_gpu_past_4gib import aggregate, make_features, make_graph, make_params, weight_grads
    n, r = 2_100_000, 4
    assert n * 512 * 4 > 1 << 32
    G = make_graph(n, r, dev, seed=din)
    x, dg = make_features(n, din, dev, seed=1), make_features(n, dout, dev, seed=2)
    w, root, bias = make_params(r, din, dout, dev, seed=3)
    plans = _plans(G["ei"], G["et"], n, r, din, dout)
    op = torch.cat([w, root[None]]).contiguous()
    out = torch.full((n, dout), float("nan"), device=dev)
    _lib.xwide_fwd(_lib.plan_struct(plans.fwd), x, din, op, bias, out, dout)
    _bound1("out", out, aggregate(G, x, w, root, bias, torch.float64), aggregate(G, x, w, root, bias, torch.float64, True))
    del out, op
    opt = torch.cat([w, root[None]]).transpose(1, 2).contiguous()
    dx = torch.full((n, din), float("nan"), device=dev)
    _lib.xwide_bwd_dx(_lib.plan_struct(plans.bwd), dg, dout, opt, dx, din)
    _bound1("dx", dx, aggregate(G, dg, w, root, None, torch.float64, transposed=True),
            aggregate(G, dg, w, root, None, torch.float64, True, transposed=True))
    del dx, opt
    gc.collect()
    dw, dr, db = (torch.full(s, float("nan"), device=dev) for s in ((r, din, dout), (din, dout), (dout,)))
    _lib.xwide_bwd_dw(_lib.plan_struct(plans.fwd), x, din, dg, dout, dw, dr, db)
    ref, cond = weight_grads(G, x, dg, torch.float64), weight_grads(G, x, dg, torch.float64, True)
    for name, got, rf, cd in zip(("d_weight", "d_root", "d_bias"), (dw, dr, db), ref, cond):
        _bound1(name, got if got.dim() > 1 else got[None], rf if rf.dim() > 1 else rf[None], cd if cd.dim() > 1 else cd[None])
    assert torch.all(dw[r - 1] == 0)
    del plans
    clear_plan_cache()
    torch.cuda.empty_cache()
