"""Parity of the HIP path (through the C ABI) against the oracle and the committed golden vectors.
Needs an MI355X: run with ``pytest -m gpu``.  Tolerance: BASELINE.json's 1e-5 (fp32), atol = rtol."""
import numpy as np
import pytest
import torch

from oracle import rgcn_oracle as O

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-5, atol=1e-5)
from oracle.tolerance import abs_condition, assert_close, cpu32_reference  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from scaling_rgcn_training_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _abi_layer(dev, ei, et, n, num_rel, x, w_full, root, bias, dout_grad, tile=None, aggr="mean", chunk=None, flags=0, split=False):
    """forward, dX, dW through the raw C-ABI wrappers (no autograd)."""
    from scaling_rgcn_training_amd import _lib, plan as P
    from scaling_rgcn_training_amd.conv import layout_for, _rows16, _round4
    din, dout = w_full.shape[1], w_full.shape[2]
    t0, c0 = layout_for(din, dout, n, int(et.shape[0]), num_rel)
    tile, chunk = tile or t0, chunk or c0
    plans = P.build_graph_plans(ei.to(dev), et.to(dev), n, num_rel, tile, aggr, chunk=chunk, split=split)
    xd = _rows16(x.to(dev), din)
    gd = _rows16(dout_grad.to(dev), dout)
    wd = w_full.to(dev).contiguous()
    rd = None if root is None else root.to(dev).contiguous()
    bd = None if bias is None else bias.to(dev).contiguous()
    out = torch.full((n, _round4(dout)), float("nan"), device=dev)
    _lib.fwd(_lib.plan_struct(plans.fwd), xd, din, _lib.pack_weights(wd, rd, False), bd, out, dout, 0, flags)
    dx = torch.full((n, _round4(din)), float("nan"), device=dev)
    _lib.bwd_dx(_lib.plan_struct(plans.bwd), gd, dout, _lib.pack_weights(wd, rd, True), dx, din, None, flags)
    dw = torch.full((num_rel, din, dout), float("nan"), device=dev)
    dr = torch.full((din, dout), float("nan"), device=dev)
    db = torch.full((dout,), float("nan"), device=dev)
    _lib.bwd_dw(_lib.plan_struct(plans.fwd), xd, din, gd, dout, dw, dr, db, flags)
    torch.cuda.synchronize()
    return (out[:, :dout].cpu().numpy(), dx[:, :din].cpu().numpy(), dw.cpu().numpy(), dr.cpu().numpy(),
            db.cpu().numpy())


def _check_layer(res, ref_out, gr, x, ei, et, w, root, bias, dg, aggr="mean", tag=""):
    """out, dX, dW, dRoot, db of the HIP path against the float64 oracle under BOTH bounds of oracle/tolerance.py:
    the a-priori one (flat 1e-5 + 4 u cond) and 'no more than twice the fp32 CPU loop's own error over flat 1e-5'."""
    out, dx, dw, dr, db = res
    c_out, c = abs_condition(x, ei, et, w, root, bias, dg, aggr=aggr)
    o32, g32 = cpu32_reference(x, ei, et, w, root, bias, dg, aggr=aggr)
    assert_close(out, ref_out, c_out, "out" + tag, cpu32=o32)
    assert_close(dx, gr["x"], c["x"], "d_x" + tag, cpu32=g32["x"])
    assert_close(dw, gr["weight"], c["weight"], "d_weight" + tag, cpu32=g32["weight"])
    assert_close(dr, gr["root"], c["root"], "d_root" + tag, cpu32=g32["root"])
    if bias is not None:
        assert_close(db, gr["bias"], c["bias"], "d_bias" + tag, cpu32=g32["bias"])


@pytest.mark.parametrize("chunk", [64, 128])
def test_abi_matches_golden(dev, golden, chunk):
    if str(golden["mode"]) != "full":
        pytest.skip("weight modes are covered at module level")
    g = golden
    f = lambda k: torch.from_numpy(g[k])
    out, dx, dw, dr, db = _abi_layer(dev, f("edge_index").long(), f("edge_type").long(), int(g["num_nodes"]),
                                     int(g["num_relations"]), f("x"), f("weight"), f("root"), f("bias"), f("dout"),
                                     chunk=chunk)
    gr = {"x": g["d_x"], "weight": g["d_wfull"], "root": g["d_root"], "bias": g["d_bias"]}
    _check_layer((out, dx, dw, dr, db), g["out"], gr, g["x"], g["edge_index"], g["edge_type"], g["weight"], g["root"],
                 g["bias"], g["dout"], tag=f" [{g['name']}]")


def _module_from_golden(dev, g):
    from scaling_rgcn_training_amd.conv import RGCNConv
    mode = str(g["mode"])
    din, dout = g["x"].shape[1], g["out"].shape[1]
    kw = {}
    if mode == "basis":
        kw["num_bases"] = g["weight"].shape[0]
    if mode == "block":
        kw["num_blocks"] = int(g["nb"])
    conv = RGCNConv(din, dout, int(g["num_relations"]), **kw).to(dev)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(g["weight"]))
        conv.root.copy_(torch.from_numpy(g["root"]))
        conv.bias.copy_(torch.from_numpy(g["bias"]))
        if mode == "basis":
            conv.comp.copy_(torch.from_numpy(g["comp"]))
    return conv


def test_module_autograd_matches_golden(dev, golden):
    g = golden
    conv = _module_from_golden(dev, g)
    x = torch.from_numpy(g["x"]).to(dev).requires_grad_(True)
    ei = torch.from_numpy(g["edge_index"]).long().to(dev)
    et = torch.from_numpy(g["edge_type"]).long().to(dev)
    out = conv(x, ei, et)
    out.backward(torch.from_numpy(g["dout"]).to(dev))
    mode = str(g["mode"])
    wf64 = O.effective_weight(torch.from_numpy(g["weight"]).double(),
                              torch.from_numpy(g["comp"]).double() if mode == "basis" else None,
                              int(g["num_relations"]), int(g["nb"]) if mode == "block" else None,
                              g["x"].shape[1], g["out"].shape[1]).numpy()
    c_out, c = abs_condition(g["x"], g["edge_index"], g["edge_type"], wf64, g["root"], g["bias"], g["dout"])
    assert_close(out.detach().cpu().numpy(), g["out"], c_out, "out")
    assert_close(x.grad.cpu().numpy(), g["d_x"], c["x"], "d_x")
    assert_close(conv.root.grad.cpu().numpy(), g["d_root"], c["root"], "d_root")
    assert_close(conv.bias.grad.cpu().numpy(), g["d_bias"], c["bias"], "d_bias")
    if mode == "full":
        assert_close(conv.weight.grad.cpu().numpy(), g["d_wfull"], c["weight"], "d_weight")
    else:  # chain rule of the oracle's effective weight, fp64
        w = torch.from_numpy(g["weight"]).double().requires_grad_(True)
        comp = torch.from_numpy(g["comp"]).double().requires_grad_(True) if mode == "basis" else None
        wf = O.effective_weight(w, comp, int(g["num_relations"]), int(g["nb"]) if mode == "block" else None,
                                g["x"].shape[1], g["out"].shape[1])
        wf.backward(torch.from_numpy(g["d_wfull"]))
        # condition numbers of the same chain rule: |V|, |comp| and the abs-sum of d_wfull
        wa = torch.from_numpy(np.abs(g["weight"])).double().requires_grad_(True)
        ca = torch.from_numpy(np.abs(g["comp"])).double().requires_grad_(True) if mode == "basis" else None
        O.effective_weight(wa, ca, int(g["num_relations"]), int(g["nb"]) if mode == "block" else None,
                           g["x"].shape[1], g["out"].shape[1]).backward(torch.from_numpy(c["weight"]))
        assert_close(conv.weight.grad.cpu().numpy(), w.grad.numpy(), wa.grad.numpy(), "d_weight (decomposed)")
        if comp is not None:
            assert_close(conv.comp.grad.cpu().numpy(), comp.grad.numpy(), ca.grad.numpy(), "d_comp")


WIDTHS = [(64, 64), (63, 16), (16, 5), (16, 16), (32, 64), (64, 32), (48, 100), (128, 128), (128, 16), (7, 128),
          (1, 1), (100, 36)]


@pytest.mark.parametrize("din,dout", WIDTHS)
def test_random_graph_all_width_classes(dev, din, dout):
    n, e, r = 1500, 20000, 9
    ei, et = O.synthetic_graph(n, e, r, seed=din * 131 + dout)
    et = et.clamp(max=r - 2)  # last relation empty (the reference's dead 2R slot)
    ei[:, 10] = ei[:, 9]      # duplicate edge
    ei[1, 11] = ei[0, 11]     # self loop
    w, root, bias = O.synthetic_params(r, din, dout, seed=3)
    g = torch.Generator().manual_seed(11)
    bias = torch.randn(dout, generator=g) * 0.1
    x = torch.randn(n, din, generator=g)
    dg = torch.randn(n, dout, generator=g)
    ref, gr = O.rgcn_conv_segments(x.numpy(), ei.numpy(), et.numpy(), w.numpy(), root.numpy(), bias.numpy(), dg.numpy())
    res = _abi_layer(dev, ei, et, n, r, x, w, root, bias, dg)
    _check_layer(res, ref, gr, x, ei, et, w, root, bias, dg, tag=f" [{din}->{dout}]")   # d_weight: ~2k edges per relation
    assert np.all(res[2][r - 1] == 0.0)


@pytest.mark.parametrize("din,dout,tile", [(64, 64, 128), (64, 64, 352), (32, 16, 64), (16, 64, 256), (50, 33, 96)])
def test_chunk128_plans(dev, din, dout, tile):
    """128-slot chunks (two 64-row parts per ring slot, dW walking 64-row units): groups of ~100 edges so that
    chunks hold 1..8 row tiles, repeated destinations included."""
    n, e, r = 3000, 60000, 5
    ei, et = O.synthetic_graph(n, e, r, seed=din + 7 * dout + tile)
    ei[:, 100:140] = ei[:, 60:100]          # duplicate edges
    ei[1, 200:260] = ei[1, 200]             # a small hub inside one relation
    et[200:260] = et[200]
    w, root, bias = O.synthetic_params(r, din, dout, seed=5)
    g = torch.Generator().manual_seed(12)
    bias = torch.randn(dout, generator=g) * 0.1
    x = torch.randn(n, din, generator=g)
    dg = torch.randn(n, dout, generator=g)
    ref, gr = O.rgcn_conv_segments(x.numpy(), ei.numpy(), et.numpy(), w.numpy(), root.numpy(), bias.numpy(), dg.numpy())
    res = _abi_layer(dev, ei, et, n, r, x, w, root, bias, dg, tile=tile, chunk=128)
    _check_layer(res, ref, gr, x, ei, et, w, root, bias, dg, tag=f" [chunk128 {din}->{dout} T{tile}]")
    # and bit-identical gradients of the weights to the 64-slot layout?  No: the walk differs; same tolerance only.


@pytest.mark.parametrize("chunk,din,dout", [(64, 64, 64), (128, 64, 64), (128, 50, 33), (64, 63, 40)])
def test_dw_direct_kernel(dev, chunk, din, dout):
    """The direct-gather dW kernel (64 x 64; normally chosen for large walks only) against the oracle and, bit for
    bit in its root / bias parts' inputs, against the ring kernel on the same plan."""
    from scaling_rgcn_training_amd import _lib
    n, e, r = 5000, 90000, 7
    ei, et = O.synthetic_graph(n, e, r, seed=21)
    ei[:, 50:90] = ei[:, 10:50]             # duplicate edges
    w, root, bias = O.synthetic_params(r, din, dout, seed=6)
    g = torch.Generator().manual_seed(13)
    x = torch.randn(n, din, generator=g)
    dg = torch.randn(n, dout, generator=g)
    ref, gr = O.rgcn_conv_segments(x.numpy(), ei.numpy(), et.numpy(), w.numpy(), root.numpy(), bias.numpy(), dg.numpy())
    out, dx, dw, dr, db = _abi_layer(dev, ei, et, n, r, x, w, root, bias, dg, tile=128, chunk=chunk,
                                     flags=_lib.FLAG_DW_DIRECT)
    c_out, c = abs_condition(x, ei, et, w, root, bias, dg)
    assert_close(dw, gr["weight"], c["weight"], "d_weight (direct)")
    assert_close(dr, gr["root"], c["root"], "d_root (direct)")
    assert_close(db, gr["bias"], c["bias"], "d_bias (direct)")
    _, _, dw0, dr0, db0 = _abi_layer(dev, ei, et, n, r, x, w, root, bias, dg, tile=128, chunk=chunk,
                                     flags=_lib.FLAG_DW_RING)
    assert_close(dw, dw0, c["weight"], "direct vs ring d_weight")
    assert_close(db, db0, c["bias"], "direct vs ring d_bias")


def test_skewed_hub_graph_and_sum_aggr(dev):
    n, e, r, din, dout = 4000, 60000, 5, 64, 64
    ei, et = O.synthetic_graph(n, e, r, seed=5, skew=True)
    w, root, bias = O.synthetic_params(r, din, dout, seed=4)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(n, din, generator=g)
    dg = torch.randn(n, dout, generator=g)
    for aggr in ("mean", "sum"):
        ref, gr = O.rgcn_conv_segments(x.numpy(), ei.numpy(), et.numpy(), w.numpy(), root.numpy(), bias.numpy(),
                                       dg.numpy(), aggr=aggr)
        res = _abi_layer(dev, ei, et, n, r, x, w, root, bias, dg, aggr=aggr)
        _check_layer(res, ref, gr, x, ei, et, w, root, bias, dg, aggr=aggr, tag=f" [hub {aggr}]")


def test_empty_graph_and_tiny_tiles(dev):
    n, r, din, dout = 37, 3, 12, 20
    ei = torch.zeros(2, 0, dtype=torch.long)
    et = torch.zeros(0, dtype=torch.long)
    w, root, bias = O.synthetic_params(r, din, dout, seed=1)
    bias = bias + 0.5
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n, din, generator=g)
    dg = torch.randn(n, dout, generator=g)
    out, dx, dw, dr, db = _abi_layer(dev, ei, et, n, r, x, w, root, bias, dg, tile=16)
    np.testing.assert_allclose(out, (x @ root + bias).numpy(), **TOL)
    np.testing.assert_allclose(dx, (dg @ root.T).numpy(), **TOL)
    assert np.all(dw == 0)
    assert_close(dr, (x.double().T @ dg.double()).numpy(), (x.abs().double().T @ dg.abs().double()).numpy(), "d_root")
    assert_close(db, dg.double().sum(0).numpy(), dg.abs().double().sum(0).numpy(), "d_bias")


def test_run_to_run_bitwise_determinism(dev):
    n, e, r = 3000, 50000, 6
    ei, et = O.synthetic_graph(n, e, r, seed=9)
    w, root, bias = O.synthetic_params(r, 64, 64, seed=9)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n, 64, generator=g)
    dg = torch.randn(n, 64, generator=g)
    a = _abi_layer(dev, ei, et, n, r, x, w, root, bias, dg)
    b = _abi_layer(dev, ei, et, n, r, x, w, root, bias, dg)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_frozen_params_and_override_contract(dev):
    """override_params re-binds fresh (possibly frozen) Parameters (model/layers.py:33-46)."""
    from scaling_rgcn_training_amd.layers import Emb_Layers
    from scaling_rgcn_training_amd.data import Data
    torch.manual_seed(0)
    n, r = 200, 5
    ei, et = O.synthetic_graph(n, 1500, r, seed=1)
    data = Data(edge_index=ei)
    data.edge_type = et
    data = data.to(dev)
    m = Emb_Layers(r, 16, 4, n, 63, None).to(dev)
    src = Emb_Layers(r, 16, 4, n, 63, None).to(dev)
    m.override_params(src.rgcn1.weight.clone(), src.rgcn1.bias.clone(), src.rgcn1.root.clone(),
                      src.rgcn2.weight.clone(), src.rgcn2.bias.clone(), src.rgcn2.root.clone(), grad=False)
    out = m(data, torch.sigmoid)
    out.sum().backward()
    assert m.rgcn1.weight.grad is None and m.rgcn2.root.grad is None and m.rgcn1.bias.grad is None
    assert m.embedding.weight.grad is not None and torch.isfinite(m.embedding.weight.grad).all()
    # forward equals the oracle evaluated with the transferred parameters
    with torch.no_grad():
        h = O.rgcn_conv_loop(m.embedding.weight.cpu().double(), ei, et, src.rgcn1.weight.cpu().double(),
                             src.rgcn1.root.cpu().double(), src.rgcn1.bias.cpu().double()).relu()
        ref = torch.sigmoid(O.rgcn_conv_loop(h, ei, et, src.rgcn2.weight.cpu().double(),
                                             src.rgcn2.root.cpu().double(), src.rgcn2.bias.cpu().double()))
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.numpy(), **TOL)


def test_pointer_gather_fallback_path(dev):
    """Matrices of 4 GiB and more (or >= 2^24 rows) cannot go through a buffer descriptor; the kernels then
    gather through 64-bit pointers.  Forced here on a small input so the fallback is covered."""
    from scaling_rgcn_training_amd import _lib
    for din, dout in ((64, 64), (63, 16), (128, 32)):
        n, e, r = 1200, 15000, 6
        ei, et = O.synthetic_graph(n, e, r, seed=21)
        w, root, bias = O.synthetic_params(r, din, dout, seed=5)
        g = torch.Generator().manual_seed(4)
        x = torch.randn(n, din, generator=g)
        dg = torch.randn(n, dout, generator=g)
        ref, gr = O.rgcn_conv_segments(x.numpy(), ei.numpy(), et.numpy(), w.numpy(), root.numpy(), bias.numpy(), dg.numpy())
        out, dx, dw, dr, db = _abi_layer(dev, ei, et, n, r, x, w, root, bias, dg, flags=_lib.FLAG_POINTER_GATHER)
        c_out, c = abs_condition(x, ei, et, w, root, bias, dg)
        assert_close(out, ref, c_out, "out")
        assert_close(dx, gr["x"], c["x"], "d_x")
        assert_close(dw, gr["weight"], c["weight"], "d_weight")
        assert_close(dr, gr["root"], c["root"], "d_root")


@pytest.mark.parametrize("din,hid,dout,final", [(63, 16, 4, "sigmoid"), (64, 64, 64, "none"), (32, 50, 7, "sigmoid")])
def test_fused_activations_match_oracle(dev, din, hid, dout, final):
    """rgcn1 -> ReLU -> rgcn2 -> activation with the activations fused into the kernels (ReLU / sigmoid in the
    forward store, the ReLU backward as the mask of the next layer's dX store: reference model/layers.py:21-24)
    against the float64 oracle ``rgcn_conv_loop(...).relu()`` under autograd, and against the unfused torch ops."""
    from scaling_rgcn_training_amd.conv import RGCNConv
    n, e, r = 2500, 30000, 7
    ei, et = O.synthetic_graph(n, e, r, seed=din + hid)
    g = torch.Generator().manual_seed(31)
    x0 = torch.randn(n, din, generator=g)
    dg = torch.randn(n, dout, generator=g)
    w1, r1, b1 = O.synthetic_params(r, din, hid, seed=7)
    w2, r2, b2 = O.synthetic_params(r, hid, dout, seed=8)
    b1 = torch.randn(hid, generator=g) * 0.1
    b2 = torch.randn(dout, generator=g) * 0.1
    # float64 oracle
    P = [t.double().clone().requires_grad_(True) for t in (x0, w1, r1, b1, w2, r2, b2)]
    h = O.rgcn_conv_loop(P[0], ei, et, P[1], P[2], P[3]).relu()
    z = O.rgcn_conv_loop(h, ei, et, P[4], P[5], P[6])
    ref = torch.sigmoid(z) if final == "sigmoid" else z
    ref.backward(dg.double())
    # fp32 CPU loop (the reference-style path) for bound (2)
    Q = [t.float().clone().requires_grad_(True) for t in (x0, w1, r1, b1, w2, r2, b2)]
    h32 = O.rgcn_conv_loop(Q[0], ei, et, Q[1], Q[2], Q[3]).relu()
    z32 = O.rgcn_conv_loop(h32, ei, et, Q[4], Q[5], Q[6])
    (torch.sigmoid(z32) if final == "sigmoid" else z32).backward(dg)
    out32 = (torch.sigmoid(z32) if final == "sigmoid" else z32).detach()

    def run(fused):
        c1, c2 = RGCNConv(din, hid, r).to(dev), RGCNConv(hid, dout, r).to(dev)
        with torch.no_grad():
            for c, (w, rt, b) in ((c1, (w1, r1, b1)), (c2, (w2, r2, b2))):
                c.weight.copy_(w); c.root.copy_(rt); c.bias.copy_(b)
        x = x0.to(dev).requires_grad_(True)
        eid, etd = ei.to(dev), et.to(dev)
        if fused:
            hh = c1(x, eid, etd, _activation="relu", _grad_premasked=True)
            out = c2(hh, eid, etd, _activation="sigmoid" if final == "sigmoid" else None, _input_relu=True)
        else:
            hh = torch.relu(c1(x, eid, etd))
            out = c2(hh, eid, etd)
            out = torch.sigmoid(out) if final == "sigmoid" else out
        out.backward(dg.to(dev))
        torch.cuda.synchronize()
        return [out.detach().cpu()] + [t.grad.cpu() for t in (x, c1.weight, c1.root, c1.bias, c2.weight, c2.root, c2.bias)]

    fused, plain = run(True), run(False)
    names = ["out", "d_x", "d_w1", "d_root1", "d_b1", "d_w2", "d_root2", "d_b2"]
    refs = [ref.detach()] + [p.grad for p in P]
    c32 = [out32] + [q.grad for q in Q]
    for nm, f, pl, rf, c in zip(names, fused, plain, refs, c32):
        # summation-order slack: |.| evaluated terms are not available for the 2-layer chain; bound (2) carries it
        err = (f.double() - rf).abs()
        cpu_err = float((c.double() - rf).abs().max())
        excess = float((err - (1e-5 + 1e-5 * rf.abs())).max())
        assert excess <= 2 * cpu_err, f"{nm}: excess over flat 1e-5 {excess:.3e} > 2 x fp32 CPU loop error {cpu_err:.3e}"
        from oracle.tolerance import SLACK_LOG
        SLACK_LOG.append((f"fused {nm} [{din}->{hid}->{dout} {final}]", excess, cpu_err))
    # the fused forward is the unfused forward bit for bit where the activation is exact (ReLU); sigmoid differs
    # from torch's by rounding only
    if final == "none":
        assert torch.equal(fused[0], plain[0])
    else:
        assert torch.allclose(fused[0], plain[0], rtol=0, atol=3e-7)
    for f, pl in zip(fused[1:], plain[1:]):
        assert torch.allclose(f, pl, rtol=1e-5, atol=1e-5)


def test_fused_activation_standalone_relu_backward(dev):
    """A fused ReLU whose consumer does NOT fold the mask: the layer differentiates its own activation
    (rgcn_act_backward), same gradients as torch.relu outside."""
    from scaling_rgcn_training_amd.conv import RGCNConv
    n, e, r, din, dout = 1200, 9000, 4, 20, 12
    ei, et = O.synthetic_graph(n, e, r, seed=3)
    conv = RGCNConv(din, dout, r).to(dev)
    g = torch.Generator().manual_seed(5)
    x0, dg = torch.randn(n, din, generator=g).to(dev), torch.randn(n, dout, generator=g).to(dev)
    res = []
    for fused in (True, False):
        x = x0.clone().requires_grad_(True)
        conv.zero_grad()
        out = conv(x, ei.to(dev), et.to(dev), _activation="relu") if fused else torch.relu(conv(x, ei.to(dev), et.to(dev)))
        out.backward(dg)
        res.append([out.detach(), x.grad, conv.weight.grad.clone(), conv.root.grad.clone(), conv.bias.grad.clone()])
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("split", [False, True], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("n,e,r,skew", [(5000, 90000, 7, False), (20000, 600000, 32, False), (3000, 200000, 3, True), (700, 5000, 32, False)])
def test_dw_tile_major_kernel(dev, n, e, r, skew, split):
    """rgcn_bwd_dw_tiles (tile-major d_weight: one relation per wave, gradient rows staged in LDS) + the root-only walk of
    rgcn_bwd_dw against the oracle, and against the relation-major kernels on the same inputs."""
    from scaling_rgcn_training_amd import _lib, plan as P
    din = dout = 64
    ei, et = O.synthetic_graph(n, e, r, seed=n + r, skew=skew)
    if r > 2:
        et = et.clamp(max=r - 2)                 # dead last relation
    ei[:, 10:60] = ei[:, 70:120]                 # duplicate triples
    et[10:60] = et[70:120]
    w, root, bias = O.synthetic_params(r, din, dout, seed=2)
    g = torch.Generator().manual_seed(23)
    x = torch.randn(n, din, generator=g)
    dg = torch.randn(n, dout, generator=g)
    ref, gr = O.rgcn_conv_segments(x.numpy(), ei.numpy(), et.numpy(), w.numpy(), root.numpy(), bias.numpy(), dg.numpy())
    t_dw, walkers, max_rel = _lib.dw_tiles_geometry()
    assert r <= max_rel
    plans = P.build_graph_plans_device(ei.to(dev), et.to(dev), n, r, 128, dw_tiles=True)
    assert plans.dw is not None and plans.dw.tile == t_dw and plans.dw.chunk == 64 and plans.dw_walk.shape == (r, walkers + 1)
    # rgcn_dw_tiles_walk (integer work: bit-exact) against its torch form
    assert torch.equal(plans.dw_walk, P.dw_walk_table(plans.dw, walkers))
    xd, gd = x.to(dev), dg.to(dev)
    dw = torch.full((r, din, dout), float("nan"), device=dev)
    # split: the same walk with both operands cut into three bf16 pieces by the wave that uses them (fp32-equivalent; same bounds)
    _lib.bwd_dw_tiles(_lib.plan_struct(plans.dw), plans.dw_walk, xd, din, gd, dout, dw, _lib.FLAG_SPLIT_PRODUCERS if split else 0)
    dr = torch.full((din, dout), float("nan"), device=dev)
    db = torch.full((dout,), float("nan"), device=dev)
    _lib.bwd_dw(_lib.plan_struct(plans.fwd), xd, din, gd, dout, None, dr, db, _lib.FLAG_DW_ROOT_ONLY)
    dw0, dr0, db0 = torch.empty_like(dw), torch.empty_like(dr), torch.empty_like(db)
    _lib.bwd_dw(_lib.plan_struct(plans.fwd), xd, din, gd, dout, dw0, dr0, db0)
    torch.cuda.synchronize()
    c_out, c = abs_condition(x, ei, et, w, root, bias, dg)
    _, g32 = cpu32_reference(x, ei, et, w, root, bias, dg)
    assert_close(dw.cpu().numpy(), gr["weight"], c["weight"], f"d_weight (tile-major) [n{n} r{r}]", cpu32=g32["weight"])
    assert_close(dr.cpu().numpy(), gr["root"], c["root"], f"d_root (root-only walk) [n{n} r{r}]", cpu32=g32["root"])
    assert_close(db.cpu().numpy(), gr["bias"], c["bias"], f"d_bias (root-only walk) [n{n} r{r}]", cpu32=g32["bias"])
    assert_close(dw.cpu().numpy(), dw0.cpu().numpy(), c["weight"], "tile-major vs relation-major d_weight")
    # (same units, but cut into workgroup ranges of their own: same sums up to fp32 re-association)
    assert_close(dr.cpu().numpy(), dr0.cpu().numpy(), c["root"], "root-only vs full walk d_root")
    assert_close(db.cpu().numpy(), db0.cpu().numpy(), c["bias"], "root-only vs full walk d_bias")
    if r > 2:
        assert torch.all(dw[r - 1] == 0)


@pytest.mark.parametrize("rows,din,dout", [(1, 64, 64), (3, 5, 7), (50, 63, 16), (4097, 64, 64), (20011, 16, 33),
                                           (300000, 64, 64)])
def test_dw_root_streaming_kernel(dev, rows, din, dout):
    """rgcn_bwd_dw_root (plan-free d_root = x^T g, d_bias = column sums of g; widths up to 64, any row count, padded row
    strides) against float64 and against the fp32 CPU matmul's own error; bit-reproducible; both outputs optional."""
    from scaling_rgcn_training_amd import _lib
    g = torch.Generator().manual_seed(rows + din)
    ldx, ldg = (din + 3) // 4 * 4, (dout + 3) // 4 * 4
    x = torch.zeros(rows, ldx)
    x[:, :din] = torch.randn(rows, din, generator=g)
    dg = torch.zeros(rows, ldg)
    dg[:, :dout] = torch.randn(rows, dout, generator=g)
    xd, gd = x.to(dev), dg.to(dev)
    dr, db = torch.full((din, dout), 7.0, device=dev), torch.full((dout,), 7.0, device=dev)
    _lib.bwd_dw_root(xd, din, gd, dout, dr, db)
    x64, g64 = x[:, :din].double().numpy(), dg[:, :dout].double().numpy()
    ref_r, ref_b = x64.T @ g64, g64.sum(0)
    cond_r, cond_b = np.abs(x64).T @ np.abs(g64), np.abs(g64).sum(0)
    cpu_r = (x[:, :din].t() @ dg[:, :dout]).numpy()
    cpu_b = dg[:, :dout].sum(0).numpy()
    assert_close(dr.cpu().numpy(), ref_r, cond_r, f"d_root (streaming kernel) [{rows}x{din}x{dout}]", cpu32=cpu_r)
    assert_close(db.cpu().numpy(), ref_b, cond_b, f"d_bias (streaming kernel) [{rows}x{din}x{dout}]", cpu32=cpu_b)
    dr2, db2 = torch.empty_like(dr), torch.empty_like(db)
    _lib.bwd_dw_root(xd, din, gd, dout, dr2, None)
    _lib.bwd_dw_root(xd, din, gd, dout, None, db2)
    assert torch.equal(dr, dr2) and torch.equal(db, db2)


@pytest.mark.parametrize("teams", [False, True], ids=["layout0-one-team", "layout1"])
@pytest.mark.parametrize("n,e,r,tile,skew", [(3000, 330000, 3, 224, False), (2000, 200000, 4, 128, True), (5000, 90000, 7, 224, False),
                                             (800, 120000, 2, 64, True), (40, 300, 2, 16, False), (3000, 60000, 40, 224, True)])
def test_split_producers_kernel_matches_oracle(dev, n, e, r, tile, skew, teams):
    """The bf16 x 3 forward / dX kernel whose PRODUCER waves split the gathered rows (csrc/rgcn_tile3p.hip; 64 x 64, 128-slot
    chunks, tiles up to 224) on layout-0 plans and on layout-1 plans (plan.team_placement: the destination-disjoint parts of
    every chunk), which it walks like any other.  Hubs and duplicate triples so that row tiles repeat destinations and take
    the run-sum path and some chunks' parts share a destination (flag 256), chunks of 1 to 8 row tiles, a graph of three
    tiles.  Against the
    float64 oracle under both bounds of oracle/tolerance.py, and against the exact-fp32 kernel on the same plan;
    bit-reproducible."""
    from scaling_rgcn_training_amd import _lib
    din = dout = 64
    ei, et = O.synthetic_graph(n, e, r, seed=n + r, skew=skew)
    ei[:, 100:160] = ei[:, 20:80]           # duplicate triples
    et[100:160] = et[20:80]
    w, root, bias = O.synthetic_params(r, din, dout, seed=9)
    g = torch.Generator().manual_seed(17)
    bias = torch.randn(dout, generator=g) * 0.1
    x = torch.randn(n, din, generator=g)
    dg = torch.randn(n, dout, generator=g)
    ref, gr = O.rgcn_conv_segments(x.numpy(), ei.numpy(), et.numpy(), w.numpy(), root.numpy(), bias.numpy(), dg.numpy())
    res3 = _abi_layer(dev, ei, et, n, r, x, w, root, bias, dg, tile=tile, chunk=128, flags=_lib.FLAG_SPLIT_PRODUCERS, split=teams)
    _check_layer(res3, ref, gr, x, ei, et, w, root, bias, dg, tag=f" [bf16x3 producers T{tile} n{n} layout {int(teams)}]")
    res1 = _abi_layer(dev, ei, et, n, r, x, w, root, bias, dg, tile=tile, chunk=128, split=teams)      # exact-fp32 kernels, same plan
    if teams:
        _check_layer(res1, ref, gr, x, ei, et, w, root, bias, dg, tag=f" [fp32 on layout 1 T{tile} n{n}]")
    for a, b in zip(res3[:2], res1[:2]):
        assert np.max(np.abs(a - b)) <= 2e-5 * max(1.0, float(np.abs(b).max()))
    assert np.array_equal(res3[2], res1[2])          # dW does not depend on the forward kernel
    again = _abi_layer(dev, ei, et, n, r, x, w, root, bias, dg, tile=tile, chunk=128, flags=_lib.FLAG_SPLIT_PRODUCERS, split=teams)
    assert np.array_equal(res3[0], again[0]) and np.array_equal(res3[1], again[1])


def test_split_kernels_on_extreme_magnitudes(dev):
    """the bf16 x 3 kernels cut every fp32 operand into round-to-nearest bf16 pieces.  bf16 has fp32's exponent
    range, so huge (1e30) and tiny (1e-30) finite values split exactly like ordinary ones and the split kernels agree with the
    exact-fp32 kernels relative to the row's magnitude; fp32 denormals (1e-40) are flushed by both forms -- their
    contributions are 1e-35 below the tolerance.  What differs is documented, not hidden: an Inf (or a finite value above
    bf16's largest, 3.39e38) makes the high piece Inf and the residual NaN, so the rows such a value reaches come out NaN
    where the exact kernel says +-Inf / NaN -- non-finite in both, finite and equal everywhere else."""
    from scaling_rgcn_training_amd import _lib
    n, e, r = 3000, 60000, 3
    ei, et = O.synthetic_graph(n, e, r, seed=21)
    w, root, bias = O.synthetic_params(r, 64, 64, seed=21)
    g = torch.Generator().manual_seed(21)
    x = torch.randn(n, 64, generator=g)
    dg = torch.randn(n, 64, generator=g)
    x[10] *= 1e30
    x[11] *= 1e-30
    x[12] = 1e-40                                   # fp32 denormals
    x[13, 5] = float("inf")
    res3 = _abi_layer(dev, ei, et, n, r, x, w, root, bias, dg, tile=224, chunk=128, flags=_lib.FLAG_SPLIT_PRODUCERS)
    res1 = _abi_layer(dev, ei, et, n, r, x, w, root, bias, dg, tile=224, chunk=128)
    out3, out1 = res3[0], res1[0]
    reached = np.zeros(n, dtype=bool)               # rows the Inf reaches: node 13 itself and the destinations of its out-edges
    reached[13] = True
    reached[ei[1][ei[0] == 13].numpy()] = True
    assert not np.isfinite(out3[reached]).all(axis=1).any() and not np.isfinite(out1[reached]).all(axis=1).any()
    assert np.isfinite(out3[~reached]).all() and np.isfinite(out1[~reached]).all()
    scale = np.maximum(1.0, np.abs(out1[~reached]).max(axis=1, keepdims=True))          # per row: 1e30-sized rows compare relatively
    assert np.max(np.abs(out3[~reached] - out1[~reached]) / scale) <= 2e-5
    # dX does not see x; finite and equal throughout
    assert np.isfinite(res3[1]).all() and np.max(np.abs(res3[1] - res1[1])) <= 2e-5 * max(1.0, float(np.abs(res1[1]).max()))


def test_split_producers_through_the_module(dev):
    """``RGCNConv.split_producers`` on / off through autograd: the producer-split kernel (tiles of at most 224 nodes) against the exact-fp32
    kernel, 63 -> 64 (padded input rows), the ReLU mask of the input in the dX store, all four gradients; and the fused
    ReLU forward.  (The backward comparison runs without a fused output activation: its mask ``out > 0`` is a step function of
    outputs that legitimately differ in the last bits between two kernels.)"""
    from scaling_rgcn_training_amd.conv import RGCNConv
    n, e, r = 6000, 200000, 5
    ei, et = O.synthetic_graph(n, e, r, seed=4)
    g = torch.Generator().manual_seed(3)
    x = torch.relu(torch.randn(n, 63, generator=g))
    dg = torch.randn(n, 64, generator=g)
    outs = []
    for on in (False, True):
        torch.manual_seed(0)
        conv = RGCNConv(63, 64, r).to(dev)
        conv.split_producers = on
        eid, etd = ei.to(dev), et.to(dev)
        xd = x.to(dev).requires_grad_(True)
        out = conv(xd, eid, etd, _input_relu=True)
        out.backward(dg.to(dev))
        assert conv._plans(xd, eid, etd).fwd.tile <= (224 if on else 352)
        with torch.no_grad():
            act = conv(xd, eid, etd, _activation="relu")
        outs.append([t.detach().cpu().numpy() for t in (out, xd.grad, conv.weight.grad, conv.root.grad, conv.bias.grad, act)])
    for a, b in zip(outs[1], outs[0]):
        np.testing.assert_allclose(a, b, rtol=2e-5, atol=2e-5 * max(1.0, float(np.abs(b).max())))


@pytest.mark.parametrize("split", [False, True], ids=["fp32", "bf16x3"])
def test_tile_major_dw_through_the_module(dev, monkeypatch, split):
    """The backward the headline configuration takes -- d_weight by ``rgcn_bwd_dw_tiles`` (both forms), d_root / d_bias by the
    streaming kernel on the side stream beside dX, one flat gradient buffer -- forced onto a graph the oracle finishes in
    seconds (the module takes this path from 4M edges / 262,144 nodes on), all four gradients against the float64 oracle."""
    from scaling_rgcn_training_amd import conv as C
    monkeypatch.setattr(C, "DW_TILES_MIN_EDGES", 1)
    monkeypatch.setattr(C, "_SIDE_STREAM_MIN_ROWS", 1)
    n, e, r = 20000, 500000, 32
    ei, et = O.synthetic_graph(n, e, r, seed=12)
    et = et.clamp(max=r - 2)                      # dead last relation: its wave walks no unit at all
    w, root, bias = O.synthetic_params(r, 64, 64, seed=5)
    g = torch.Generator().manual_seed(31)
    x = torch.randn(n, 64, generator=g)
    dg = torch.randn(n, 64, generator=g)
    ref, gr = O.rgcn_conv_segments(x.numpy(), ei.numpy(), et.numpy(), w.numpy(), root.numpy(), bias.numpy(), dg.numpy())
    conv = C.RGCNConv(64, 64, r).to(dev)
    conv.split_producers = split
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.root.copy_(root)
        conv.bias.copy_(bias)
    eid, etd = ei.to(dev), et.to(dev)
    xd = x.to(dev).requires_grad_(True)
    out = conv(xd, eid, etd)
    plans = conv._plans(xd, eid, etd)
    assert plans.dw is not None and plans.dw.tile == C._lib.dw_tiles_geometry()[0]            # the tile-major plan exists: backward takes that path
    out.backward(dg.to(dev))
    torch.cuda.synchronize()
    c_out, c = abs_condition(x, ei, et, w, root, bias, dg)
    _, g32 = cpu32_reference(x, ei, et, w, root, bias, dg)
    assert_close(out.detach().cpu().numpy(), ref, c_out, f"module out [{split}]")
    assert_close(xd.grad.cpu().numpy(), gr["x"], c["x"], f"module d_x [{split}]", cpu32=g32["x"])
    assert_close(conv.weight.grad.cpu().numpy(), gr["weight"], c["weight"], f"module d_weight (tile-major) [{split}]", cpu32=g32["weight"])
    assert_close(conv.root.grad.cpu().numpy(), gr["root"], c["root"], f"module d_root (side stream) [{split}]", cpu32=g32["root"])
    assert_close(conv.bias.grad.cpu().numpy(), gr["bias"], c["bias"], f"module d_bias (side stream) [{split}]", cpu32=g32["bias"])
    assert torch.all(conv.weight.grad[r - 1] == 0)


def test_tile_major_dw_falls_back_when_not_buffer_addressable(dev, monkeypatch):
    """rgcn_bwd_dw_tiles gathers through buffer descriptors only (< 2^24 rows, < 4 GiB); on larger operands
    the library answers RGCN_ERR_ADDRESS and the module must not plan for that kernel -- its backward then runs the relation-
    major kernels (64-bit pointer gathers) and still matches the oracle.  The size limit is faked (a 16.7M-node graph does not
    fit a test): RGCN_FLAG_POINTER_GATHER for the raw call, ``_lib.buffer_addressable`` patched for the module."""
    from scaling_rgcn_training_amd import _lib, conv as C, plan as P
    monkeypatch.setattr(C, "DW_TILES_MIN_EDGES", 1)
    n, e, r = 5000, 100000, 6
    ei, et = O.synthetic_graph(n, e, r, seed=2)
    w, root, bias = O.synthetic_params(r, 64, 64, seed=2)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(n, 64, generator=g)
    dg = torch.randn(n, 64, generator=g)
    eid, etd = ei.to(dev), et.to(dev)
    # the raw entry point: a distinct status, not "inconsistent graph plan"
    plans = P.build_graph_plans_device(eid, etd, n, r, 224, chunk=128, dw_tiles=True)
    dw = torch.empty(r, 64, 64, device=dev)
    with pytest.raises(_lib.RgcnLibraryError) as err:
        _lib.bwd_dw_tiles(_lib.plan_struct(plans.dw), plans.dw_walk, x.to(dev), 64, dg.to(dev), 64, dw, _lib.FLAG_POINTER_GATHER)
    assert err.value.status == _lib.ERR_ADDRESS and "buffer descriptor" in str(err.value)
    P.clear_plan_cache()
    # the module: no tile-major plan, relation-major backward
    monkeypatch.setattr(_lib, "buffer_addressable", lambda rows, ld: False)
    conv = C.RGCNConv(64, 64, r).to(dev)
    conv.kernel_flags = _lib.FLAG_POINTER_GATHER
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.root.copy_(root)
        conv.bias.copy_(bias)
    xd = x.to(dev).requires_grad_(True)
    out = conv(xd, eid, etd)
    assert conv._plans(xd, eid, etd).dw is None
    out.backward(dg.to(dev))
    ref, gr = O.rgcn_conv_segments(x.numpy(), ei.numpy(), et.numpy(), w.numpy(), root.numpy(), bias.numpy(), dg.numpy())
    c_out, c = abs_condition(x, ei, et, w, root, bias, dg)
    _, g32 = cpu32_reference(x, ei, et, w, root, bias, dg)
    assert_close(out.detach().cpu().numpy(), ref, c_out, "fallback out")
    assert_close(xd.grad.cpu().numpy(), gr["x"], c["x"], "fallback d_x", cpu32=g32["x"])
    assert_close(conv.weight.grad.cpu().numpy(), gr["weight"], c["weight"], "fallback d_weight", cpu32=g32["weight"])
    assert_close(conv.root.grad.cpu().numpy(), gr["root"], c["root"], "fallback d_root", cpu32=g32["root"])
    P.clear_plan_cache()


@pytest.mark.parametrize("seed", range(5))
def test_dw_tile_major_split_random_shapes_against_exact_fp32(dev, seed):
    """The bf16 x 3 form of the tile-major d_weight kernel vs its exact-fp32 form on the SAME plan: random node counts (partial
    last tile, fewer tiles than walkers), 1..32 relations with an empty one, widths 33..64, hubs, strided operand rows."""
    from scaling_rgcn_training_amd import _lib, plan as P
    from scaling_rgcn_training_amd.conv import _rows16
    g = torch.Generator().manual_seed(500 + seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
    n, r = (ri(50, 3000) if seed % 2 else ri(3000, 60000)), ri(1, 32)
    e = ri(n, 30 * n)
    din, dout = ri(33, 64), ri(33, 64)
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, n, (e,), generator=g)
    if seed % 2 == 0:
        m = torch.rand(e, generator=g) < 0.2
        dst[m] = torch.randint(0, 8, (int(m.sum()),), generator=g)
    et = torch.randint(0, max(1, r - 1), (e,), generator=g)
    plans = P.build_graph_plans_device(torch.stack([src, dst]).to(dev), et.to(dev), n, r, 128, dw_tiles=True)
    x = _rows16(torch.randn(n, din, generator=g).to(dev), din)
    dg = _rows16(torch.randn(n, dout, generator=g).to(dev), dout)
    res = []
    for fl in (0, _lib.FLAG_SPLIT_PRODUCERS):
        dw = torch.full((r, din, dout), float("nan"), device=dev)
        _lib.bwd_dw_tiles(_lib.plan_struct(plans.dw), plans.dw_walk, x, din, dg, dout, dw, fl)
        res.append(dw.cpu().numpy())
    scale = max(1.0, float(np.abs(res[0]).max()))
    assert np.isfinite(res[1]).all()
    np.testing.assert_allclose(res[1], res[0], rtol=0, atol=2e-5 * scale)
    if r > 1:
        assert not res[1][r - 1].any()


@pytest.mark.parametrize("seed", range(6))
def test_split_producers_random_shapes_against_exact_fp32(dev, seed):
    """Producer-split kernel vs the exact-fp32 kernel on the SAME plan for random graphs: node counts that leave a partial last
    tile, tiles of 16..224 nodes, 1..40 relations, widths 33..64, hubs (run-sum path), relations without edges; and one graph
    of more than 4,096 tiles, where its workgroups walk several tiles (the ring's chunk sequence crosses tile boundaries)."""
    from scaling_rgcn_training_amd import _lib, plan as P
    from scaling_rgcn_training_amd.conv import _rows16, _round4
    g = torch.Generator().manual_seed(100 + seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
    if seed == 5:
        n, e, r, tile = 1_000_003, 3_000_000, 6, 224          # 4,465 tiles: persistent workgroups
    else:
        n, r, tile = ri(50, 30000), ri(1, 40), 16 * ri(1, 14)
        e = ri(n, 40 * n)
    din, dout = ri(33, 64), ri(33, 64)
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, n, (e,), generator=g)
    if seed % 2 == 0:
        m = torch.rand(e, generator=g) < 0.2
        dst[m] = torch.randint(0, 8, (int(m.sum()),), generator=g)
    et = torch.randint(0, max(1, r - 1), (e,), generator=g)          # the last relation stays empty when r > 1
    ei = torch.stack([src, dst]).to(dev)
    plans = P.build_graph_plans_device(ei, et.to(dev), n, r, tile, chunk=128, dw_tiles=False)
    x = _rows16(torch.randn(n, din, generator=g).to(dev), din)
    dg = _rows16(torch.randn(n, dout, generator=g).to(dev), dout)
    w = (torch.randn(r, din, dout, generator=g) * 0.2).to(dev)
    root = (torch.randn(din, dout, generator=g) * 0.2).to(dev)
    bias = torch.randn(dout, generator=g).to(dev)
    F = _lib.FLAG_SPLIT_PRODUCERS
    o = [torch.full((n, _round4(dout)), float("nan"), device=dev) for _ in range(2)]
    pk = _lib.pack_weights(w, root, False)
    for k, fl in enumerate((0, F)):
        _lib.fwd(_lib.plan_struct(plans.fwd), x, din, pk, bias, o[k], dout, _lib.ACT_RELU if seed % 3 == 0 else 0, fl)
    d = [torch.full((n, _round4(din)), float("nan"), device=dev) for _ in range(2)]
    pkt = _lib.pack_weights(w, root, True)
    for k, fl in enumerate((0, F)):
        _lib.bwd_dx(_lib.plan_struct(plans.bwd), dg, dout, pkt, d[k], din, x if seed % 2 else None, fl)
    torch.cuda.synchronize()
    for a, b, width, what in ((o[1], o[0], dout, "forward"), (d[1], d[0], din, "dX")):
        a, b = a[:, :width], b[:, :width]
        assert not torch.isnan(a).any(), what
        scale = max(1.0, float(b.abs().max()))
        assert float((a - b).abs().max()) <= 2e-5 * scale, (what, n, e, r, tile, din, dout, float((a - b).abs().max()), scale)
