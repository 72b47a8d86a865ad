"""RGCNConv(aggr="max") on the GPU (csrc/rgcn_segmax.hip + the edge-parallel transform and sums, eplan.MaxPlan): the raw C ABI
(H and T bit-identical to torch, C of rgcn_segment_max_bwd equal to the same fp32 operations by torch), the module's output and all five gradients against the float64 reference of
tests/max_reference.py at every width class, weight mode and graph case, a two-layer model fused and unfused, hipGraph-replayed
training, bit-reproducibility, and the device-built plan against the CPU-built one."""
import copy

import numpy as np
import pytest
import torch

from oracle.tolerance import assert_close
from tests import max_reference as M

pytestmark = pytest.mark.gpu

N, R = 300, 5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from scaling_rgcn_training_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def graphs(dev):
    """the graph cases on the device, built once (the plan cache keys on the tensors' identity)"""
    out = {}
    for name in ("plain", "hubs", "empty"):
        ei, et = M.graph_case(name, n=N, r=R)
        out[name] = (ei, et, ei.to(dev), et.to(dev))
    return out


def _conv(din, dout, mode, root_bias=True, seed=0):
    from scaling_rgcn_training_amd.conv import RGCNConv
    torch.manual_seed(seed)
    kw = {"num_bases": 3} if mode == "basis" else ({"num_blocks": M.num_blocks_for(din, dout)} if mode == "block" else {})
    conv = RGCNConv(din, dout, R, aggr="max", root_weight=root_bias, bias=root_bias, **kw)
    if conv.bias is not None:
        with torch.no_grad():
            conv.bias.uniform_(-1, 1)
    return conv


def _check(conv, dev, graph, feat="normal", need_x=True, split=True, tag=""):
    ei, et, eid, etd = graph
    conv = conv.to(dev)
    conv.split_producers = split
    x = M.features(feat, N, conv.in_channels)
    g = torch.randn(N, conv.out_channels, generator=torch.Generator().manual_seed(3))
    for p in conv.parameters():
        p.grad = None
    xd = x.to(dev).requires_grad_(need_x)
    out = conv(xd, eid, etd)
    out.backward(g.to(dev))
    torch.cuda.synchronize()
    ref, grads = M.reference(conv, x, ei, et, g)
    c_out, conds = M.conditions(conv, x, ei, et, g)
    assert_close(out.detach().cpu().numpy(), ref, c_out, f"max out {tag}")
    if need_x:
        assert_close(xd.grad.cpu().numpy(), grads["x"], conds["x"], f"max d_x {tag}")
    else:
        assert xd.grad is None
    for name in ("weight", "comp", "root", "bias"):
        p = getattr(conv, name)
        if p is None:
            continue
        if not p.requires_grad:
            assert p.grad is None, name
            continue
        assert_close(p.grad.cpu().numpy(), grads[name], conds[name], f"max d_{name} {tag}")


WIDTHS = [(1, 1), (7, 5), (16, 16), (33, 64), (63, 16), (64, 64), (100, 128), (128, 128)]


@pytest.mark.parametrize("mode", ["full", "basis", "block"])
@pytest.mark.parametrize("din,dout", WIDTHS)
def test_max_layer_widths_and_modes(dev, graphs, din, dout, mode):
    _check(_conv(din, dout, mode), dev, graphs["plain"], tag=f"{din}x{dout} {mode}")
    if (din, dout) == (64, 64):         # the bf16 x 3 transform (default) and the exact-fp32 one
        _check(_conv(din, dout, mode), dev, graphs["plain"], split=False, tag=f"{din}x{dout} {mode} exact")


@pytest.mark.parametrize("graph,feat", [("plain", "ties"), ("plain", "negative"), ("hubs", "ties"), ("hubs", "normal"),
                                        ("empty", "normal")])
@pytest.mark.parametrize("din,dout", [(16, 16), (64, 64)])
def test_max_layer_graph_cases(dev, graphs, graph, feat, din, dout):
    _check(_conv(din, dout, "full"), dev, graphs[graph], feat=feat, tag=f"{graph} {feat} {din}x{dout}")
    _check(_conv(din, dout, "basis"), dev, graphs[graph], feat=feat, tag=f"{graph} {feat} {din}x{dout} basis")


@pytest.mark.parametrize("mode", ["full", "basis", "block"])
def test_max_layer_without_root_bias_frozen_and_constant_x(dev, graphs, mode):
    _check(_conv(32, 16, mode, root_bias=False), dev, graphs["hubs"], tag=f"no root / bias {mode}")
    conv = _conv(32, 16, mode)
    conv.weight.requires_grad_(False)
    conv.root.requires_grad_(False)
    _check(conv, dev, graphs["hubs"], tag=f"frozen weight / root {mode}")
    conv = _conv(96, 16, mode)           # (above 64 columns: d_root / d_bias by rgcn_bwd_dw's root-only walk)
    conv.bias.requires_grad_(False)
    _check(conv, dev, graphs["hubs"], need_x=False, tag=f"x without grad, frozen bias {mode}")


@pytest.mark.parametrize("piece", [8, 256])
@pytest.mark.parametrize("feat", ["normal", "ties"])
def test_segment_max_abi_bit_identical_to_torch(dev, graphs, piece, feat):
    """rgcn_segment_max level by level: H and T of every (destination, relation) segment against torch scatter_reduce amax on the
    same fp32 input and the plain count of the edges that attain it"""
    from scaling_rgcn_training_amd import _lib, eplan as E
    ei, et, eid, etd = graphs["hubs"]
    din = 20
    mp = E.build_max_plan(eid, etd, N, R, piece=piece)
    assert len(mp.ep.heavy.levels) >= 2
    x = M.features(feat, N, din).to(dev)
    xp = torch.nn.functional.pad(x, (0, 4 - din % 4)) if din % 4 else x
    h, t = _lib.max_aggregate(mp, xp.contiguous(), din, with_t=True)
    hh = mp.ep.heavy
    rel = hh.unit_rel.repeat_interleave(64)[mp.seg_dh.long()].long()
    dst = hh.slot_row[mp.seg_dh.long()].long()
    ref = torch.stack(M.max_aggregate(x, eid, etd, R))[rel, dst]                  # [n_seg, din]
    assert torch.equal(h[:, :din].view(torch.int32), ref.view(torch.int32))
    seg_of_edge = torch.searchsorted(rel * N + dst, etd * N + eid[1])
    hit = (x[eid[0]] == ref[seg_of_edge]).float()
    tref = torch.zeros_like(ref).index_add_(0, seg_of_edge, hit)
    assert torch.equal(t[:, :din], tref)
    h2, t2 = _lib.max_aggregate(mp, xp.contiguous(), din, with_t=False)
    assert t2 is None and torch.equal(h2, h)


@pytest.mark.parametrize("piece", [8, 256])
@pytest.mark.parametrize("feat", ["normal", "ties"])
def test_segment_max_bwd_abi_equal_to_torch(dev, graphs, piece, feat):
    """rgcn_segment_max_bwd on its own: C of every segment row on a random dH against where(x[src] == H[s], (w dH[seg_dh[s]]) /
    (T[s] + (H[s] == 0)), 0) by torch ops in fp32 -- one correctly rounded product and quotient on either side, so equal as values
    (check_c of tests/test_gpu_max_past_4gib.py, which runs the same comparison past 2^24 segments); with and without seg_dh and
    row_w; 18 columns: the pad columns of C are +0.0"""
    from scaling_rgcn_training_amd import _lib, eplan as E
    from tests.test_gpu_max_past_4gib import check_c
    ei, et, eid, etd = graphs["hubs"]
    din = 18
    mp = E.build_max_plan(eid, etd, N, R, piece=piece)
    xp = torch.nn.functional.pad(M.features(feat, N, din).to(dev), (0, 2)).contiguous()
    h, t = _lib.max_aggregate(mp, xp, din, with_t=True)
    if feat == "ties":
        assert int((h[:, :din] == 0).sum()) > 0 and int((t[:, :din] > 1).sum()) > 0        # N = T + 1 and N = T > 1 both occur
    assert bool((t[:, din:].view(torch.int32) == 0).all()) and bool((h[:, din:].view(torch.int32) == 0).all())
    for k, (seg_dh, row_w) in enumerate(((True, True), (False, True), (True, False), (False, False))):
        c = check_c(mp, xp, din, h, t, seed=20 + k, seg_dh=seg_dh, row_w=row_w)
        assert int((c[:, :din] != 0).sum()) >= mp.n_seg * din


@pytest.mark.parametrize("piece", [8, 256])
def test_segment_max_abi_signed_zeros_and_nan(dev, graphs, piece):
    """rgcn_segment_max on integer features with half the zeros stored as -0.0 and a few NaNs: -0 ties with +0 (T counts both),
    a NaN makes its segment's column NaN through every level, every other column is torch's max and its plain count"""
    from scaling_rgcn_training_amd import _lib, eplan as E
    ei, et, eid, etd = graphs["hubs"]
    din = 12
    mp = E.build_max_plan(eid, etd, N, R, piece=piece)
    g = torch.Generator().manual_seed(11)
    x = M.features("ties", N, din)
    neg = (x == 0) & (torch.rand(N, din, generator=g) < 0.5)
    x[neg] = -0.0
    nan = torch.rand(N, din, generator=g) < 0.01
    nan[0, 0] = nan[1, 1] = True              # (node 1: the source hub; node 0's rows reach the destination hub)
    x[nan] = float("nan")
    h, t = _lib.max_aggregate(mp, x.to(dev).contiguous(), din, with_t=True)
    h, t = h.cpu(), t.cpu()
    hh = mp.ep.heavy
    rel = hh.unit_rel.repeat_interleave(64)[mp.seg_dh.long()].long().cpu()
    dst = hh.slot_row[mp.seg_dh.long()].long().cpu()
    seg_of_edge = torch.searchsorted(rel * N + dst, et * N + ei[1])
    nan_seg = torch.zeros(h.shape[0], din).index_add_(0, seg_of_edge, nan[ei[0]].float()) > 0
    ref = torch.stack(M.max_aggregate(torch.where(nan, float("-inf"), x), ei, et, R))[rel, dst]
    hd = h[:, :din]
    assert nan_seg.any() and torch.equal(torch.isnan(hd), nan_seg)
    assert torch.equal(hd[~nan_seg], ref[~nan_seg])                               # (-0 == +0)
    hit = (x[ei[0]] == ref[seg_of_edge]).float()
    tref = torch.zeros_like(ref).index_add_(0, seg_of_edge, hit)
    assert torch.equal(t[:, :din][~nan_seg], tref[~nan_seg])
    # the case is there: maxima of zero attained by -0.0 and +0.0 rows of one segment column
    zero = (ref[seg_of_edge] == 0) & ~nan_seg[seg_of_edge]
    both = (torch.zeros_like(ref).index_add_(0, seg_of_edge, (zero & torch.signbit(x[ei[0]])).float()) > 0) & \
           (torch.zeros_like(ref).index_add_(0, seg_of_edge, (zero & ~torch.signbit(x[ei[0]])).float()) > 0)
    assert both.any()


def test_max_layer_refuses_edges_off_the_device_of_x(dev, graphs):
    """x on the GPU, the edges still on the CPU (or one of them): a RuntimeError, before any plan is built or kernel launched"""
    from scaling_rgcn_training_amd import _lib, eplan as E
    from scaling_rgcn_training_amd.plan import _CACHE
    ei, et, eid, etd = graphs["plain"]
    conv = _conv(16, 8, "full").to(dev)
    x = torch.randn(N, 16, device=dev, requires_grad=True)
    n_cached = len(_CACHE)
    for a, b in ((ei, et), (ei, etd), (eid, et)):
        with pytest.raises(RuntimeError, match="must be on the device of x"):
            conv(x, a, b)
    assert len(_CACHE) == n_cached
    # the library's own guard: a CPU-built plan never reaches rgcn_segment_max / rgcn_segment_max_bwd
    mp = E.build_max_plan(ei, et, N, R)
    with pytest.raises(_lib.RgcnLibraryError, match="max plan must live on"):
        _lib.max_aggregate(mp, x.detach(), 16, with_t=True)
    gp = torch.zeros(N, 8, device=dev)
    with pytest.raises(_lib.RgcnLibraryError, match="max plan must live on"):
        _lib.max_layer_dx(mp, x.detach(), None, None, gp, 8, gp, torch.empty(N, 16, device=dev), 16)
    out = conv(x, eid, etd)                   # the same layer on device edges still runs
    out.sum().backward()
    torch.cuda.synchronize()
    assert x.grad is not None and torch.isfinite(x.grad).all()


def test_max_plan_device_build_equals_cpu_build(dev, graphs):
    from scaling_rgcn_training_amd import eplan as E
    for name, (ei, et, eid, etd) in graphs.items():
        for piece in (8, E.PIECE):
            a, b = E.build_max_plan(eid, etd, N, R, piece=piece), E.build_max_plan(ei, et, N, R, piece=piece)
            same = lambda u, v: (u is None and v is None) or (torch.is_tensor(u) and torch.equal(u.cpu(), v)) or u == v
            assert a.n_hrows == b.n_hrows and a.n_seg == b.n_seg
            for k in ("row_src", "row_w", "row_seg", "seg_dh", "bwd_slot_src"):
                assert same(getattr(a, k), getattr(b, k)), (name, k)
            assert len(a.bwd_levels) == len(b.bwd_levels)
            for la, lb in zip(a.bwd_levels, b.bwd_levels):
                assert all(same(u, v) for u, v in zip(la, lb)), name
            for k in ("unit_rel", "unit_cnt", "slot_src", "slot_w", "slot_row"):
                assert same(getattr(a.ep, k), getattr(b.ep, k)), (name, k)
            for la, lb in zip(a.ep.levels, b.ep.levels):
                assert all(same(u, v) for u, v in zip(la, lb)), name
            assert (a.ep.heavy is None) == (b.ep.heavy is None)
            if a.ep.heavy is not None:
                for k in ("unit_rel", "unit_cnt", "slot_src", "slot_w", "slot_row"):
                    assert same(getattr(a.ep.heavy, k), getattr(b.ep.heavy, k)), (name, k)
                assert len(a.ep.heavy.levels) == len(b.ep.heavy.levels)
                for la, lb in zip(a.ep.heavy.levels, b.ep.heavy.levels):
                    assert all(same(u, v) for u, v in zip(la, lb)), name


def test_max_layer_is_bit_reproducible(dev, graphs):
    ei, et, eid, etd = graphs["hubs"]
    conv = _conv(64, 64, "basis").to(dev)
    x = M.features("ties", N, 64).to(dev)
    g = torch.randn(N, 64, device=dev)
    runs = []
    for _ in range(2):
        for p in conv.parameters():
            p.grad = None
        xd = x.clone().requires_grad_(True)
        out = conv(xd, eid, etd, _activation="relu", _input_relu=True)
        out.backward(g)
        runs.append([out.detach().clone(), xd.grad.clone()] + [p.grad.clone() for p in conv.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _max_model(r, hid, c, n, emb, seed=0):
    from scaling_rgcn_training_amd.conv import RGCNConv
    from scaling_rgcn_training_amd.layers import Emb_Layers
    torch.manual_seed(seed)
    model = Emb_Layers(r, hid, c, n, emb, None)
    model.rgcn1 = RGCNConv(emb, hid, r, aggr="max")
    model.rgcn2 = RGCNConv(hid, c, r, aggr="max")
    with torch.no_grad():
        model.rgcn1.bias.uniform_(-0.5, 0.5)
    return model


def test_emb_layers_with_max_convs_fused_unfused_and_float64(dev, graphs):
    from scaling_rgcn_training_amd.data import Data
    ei, et, eid, etd = graphs["hubs"]
    model = _max_model(R, 16, 4, N, 24).to(dev)
    data = Data(edge_index=eid)
    data.edge_type = etd
    gout = torch.randn(N, 4, generator=torch.Generator().manual_seed(5))
    res = {}
    for fuse in (True, False):
        model.fuse_activations = fuse
        model.zero_grad(set_to_none=True)
        out = model(data, torch.sigmoid)
        out.backward(gout.to(dev))
        res[fuse] = [out.detach().cpu()] + [p.grad.cpu() for p in model.parameters()]
    for a, b in zip(res[True], res[False]):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-5, atol=1e-6)
    # float64: the same two layers by the reference
    d = lambda t: t.detach().cpu().double().clone().requires_grad_(True)
    ps = [d(p) for p in model.parameters()]
    names = [k for k, _ in model.named_parameters()]
    p = dict(zip(names, ps))
    h = torch.relu(M.max_layer(p["embedding.weight"], ei, et, p["rgcn1.weight"], None, p["rgcn1.root"], p["rgcn1.bias"], R))
    o = torch.sigmoid(M.max_layer(h, ei, et, p["rgcn2.weight"], None, p["rgcn2.root"], p["rgcn2.bias"], R))
    o.backward(gout.double())
    np.testing.assert_allclose(res[True][0].numpy(), o.detach().numpy(), rtol=1e-4, atol=1e-5)
    for a, q, k in zip(res[True][1:], ps, names):
        np.testing.assert_allclose(a.numpy(), q.grad.numpy(), rtol=1e-4, atol=1e-5, err_msg=k)


def test_trainer_hipgraph_epochs_match_eager_epochs_with_max_convs(dev):
    """``Trainer.train`` replayed from hipGraphs against the same loop run eagerly, for Emb_Layers with both convs max and, from
    the same initial parameters, with both convs mean (the setup of test_trainer_hipgraph_epochs_match_eager_epochs).  The first
    epoch's loss is bit-identical and the accuracies are equal; afterwards the two modes differ by the optimizer (eager Adam
    against capturable Adam, whose device-side step count changes the bias corrections in the last fp32 bits).  The mean model
    holds the mean test's bounds; in the max model that difference moves which edge attains some maxima, and the bounds below
    are the measured size of that effect."""
    from oracle import rgcn_oracle as O
    from scaling_rgcn_training_amd.conv import RGCNConv
    from scaling_rgcn_training_amd.data import Data
    from scaling_rgcn_training_amd.layers import Emb_Layers
    from scaling_rgcn_training_amd.trainer import Trainer, bce_loss
    n, e, r, emb, hid, c = 3000, 24000, 11, 63, 16, 4
    ei, et = O.synthetic_graph(n, e, r, seed=5)
    g = torch.Generator().manual_seed(2)
    y = torch.nn.functional.one_hot(torch.randint(0, c, (n,), generator=g), c).float()
    perm = torch.randperm(n, generator=g)
    data = Data(edge_index=ei)
    data.edge_type = et
    data.x_train, data.y_train = perm[:500], y[perm[:500]]
    data.x_val, data.y_val = perm[500:700], y[perm[500:700]]

    class _Graph:
        pass

    torch.manual_seed(0)
    mean0 = Emb_Layers(r, hid, c, n, emb, None)
    max0 = copy.deepcopy(mean0)
    for name in ("rgcn1", "rgcn2"):
        old = getattr(mean0, name)
        conv = RGCNConv(old.in_channels, old.out_channels, r, aggr="max")
        conv.load_state_dict(old.state_dict())
        setattr(max0, name, conv)
    drift = {}
    for tag, model0 in (("mean", mean0), ("max", max0)):
        runs = {}
        for mode in (False, True):
            gobj = _Graph()
            gobj.training_data = data
            tr = Trainer(None, hid, epochs=12, emb_dim=emb, lr=0.01, weight_d=5e-5, verbose=False, hipgraph=mode)
            model = copy.deepcopy(model0)
            acc, losses, f1w, f1m = tr.train(model, gobj, bce_loss, torch.sigmoid, sum_graph=False)
            assert tr.last_train_mode == ("hipgraph" if mode else "eager")
            assert model.rgcn1.aggr == model.rgcn2.aggr == tag
            runs[mode] = (acc, np.asarray(losses), {k: v.detach().cpu() for k, v in model.state_dict().items()})
            assert all(q.grad is not None for q in model.parameters())
        assert len(runs[True][1]) == len(runs[False][1]) == 12
        assert runs[True][1][0] == runs[False][1][0], tag                  # before the first optimizer step: the same bits
        assert runs[True][0] == runs[False][0], tag                        # validation accuracies equal
        drift[tag] = float(np.max(np.abs(runs[True][1] - runs[False][1]) / np.abs(runs[False][1])))
        for k in runs[True][2]:
            a, b = runs[True][2][k].numpy(), runs[False][2][k].numpy()
            if tag == "mean":
                np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5, err_msg=f"{tag} {k}")
            else:
                # measured: where a last-bit difference moves which edge attains a max, the row that now receives the gradient
                # takes a whole Adam step (about lr = 0.01) the other mode's row does not: embedding elements up to 0.0098 apart,
                # relation weights up to 0.0018.  Held to two Adam steps.
                assert np.abs(a - b).max() <= 2 * 0.01, (k, float(np.abs(a - b).max()))
        assert runs[False][1][-1] < runs[False][1][0], tag                 # it trains
    # the mean model holds the mean test's 1e-5; the max model passes the optimizer's last-bit difference on through the argmax
    # flips above (measured: 1.4e-4 relative by epoch 12 against the mean model's 1.1e-5)
    assert drift["mean"] <= 2e-5 and drift["max"] <= 1e-3, drift
