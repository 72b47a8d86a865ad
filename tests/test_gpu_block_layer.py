"""``RGCNConv.forward_block`` (csrc/rgcn_minibatch.hip) against the fp64 reference of the equivalent bipartite layer
``conv((x, x[:n_dst]), edge_index, edge_type)`` (tests/bipartite_reference.py) under oracle/tolerance.py: the output and every
gradient, at every width class, on hubs cut into several rows, duplicates, isolated destinations, empty relations, one-row sides,
``n_dst == n_src``, blocks without edges or destinations, every option, and a sampler-made pair of blocks chained through
``forward_blocks(..., block_kernels=True)``.  The single gradient of ``x`` is the reference's source-side gradient with the root
term's added into its first ``n_dst`` rows -- the same composition for the condition sums and the fp32 CPU comparison."""
import numpy as np
import pytest
import torch

from oracle import rgcn_oracle as O
from oracle.tolerance import assert_close
from tests import bipartite_reference as B
from tests import sampling_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _conv(din, dout, r, seed=0, **kw):
    from scaling_rgcn_training_amd.conv import RGCNConv
    torch.manual_seed(seed)
    conv = RGCNConv(din, dout, r, **kw)
    if conv.bias is not None:
        with torch.no_grad():
            conv.bias.normal_(0, 0.5)
    return conv.to(DEV)


def _block(ei, et, n_src, n_dst):
    from scaling_rgcn_training_amd.sampling import Block
    return Block(ei.to(DEV), et.to(DEV), n_src, n_dst, torch.arange(n_src, device=DEV))


def _run(conv, x, block, g, index=None, x_grad=True):
    conv.zero_grad()
    xd = x.to(DEV).requires_grad_(x_grad)
    out = conv.forward_block(xd, block, index)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    got = {"out": out.detach().cpu()}
    if x_grad:
        got["x"] = xd.grad.cpu()
    for k in ("weight", "comp", "root", "bias"):
        p = getattr(conv, k)
        if p is not None and p.grad is not None:
            got[k] = p.grad.cpu()
    return got


def _check(conv, x, ei, et, n_dst, g, got, aggr, tag):
    din, dout, r = conv.in_channels, conv.out_channels, conv.num_relations
    w = conv.weight.detach().cpu().double()
    comp = None if conv.comp is None else conv.comp.detach().cpu().double()
    cpu = lambda p: None if p is None else p.detach().cpu()
    wf = O.effective_weight(w, comp, r, conv.num_blocks, din, dout)
    ref, cond, cpu32 = B.reference(x, x[:n_dst], ei, et, wf, cpu(conv.root), cpu(conv.bias), g, aggr)
    for d in (ref, cond, cpu32):          # forward_block's single x: the source side plus the root term in the first n_dst rows
        v = np.array(d["x_src"], copy=True)
        if "x_dst" in d:
            v[:n_dst] += d["x_dst"]
        d["x"] = v
    for k in ("out", "x", "root", "bias"):
        if k in got:
            assert tuple(got[k].shape) == ref[k].shape, (k, tag)
            assert_close(got[k].numpy(), ref[k], cond[k], f"forward_block {k} {tag}", cpu32=cpu32[k])
    if "weight" not in got and "comp" not in got:
        return
    if conv.comp is None and conv.num_blocks is None:
        assert_close(got["weight"].numpy(), ref["weight"], cond["weight"], f"forward_block d_weight {tag}", cpu32=cpu32["weight"])
        return

    def push(wv, cv, dw):
        wv = wv.clone().requires_grad_(True)
        cv = None if cv is None else cv.clone().requires_grad_(True)
        full = O.effective_weight(wv, cv, r, conv.num_blocks, din, dout)
        return torch.autograd.grad(full, [t for t in (wv, cv) if t is not None], torch.from_numpy(dw))

    want = push(w, comp, ref["weight"])
    cnd = push(w.abs(), None if comp is None else comp.abs(), np.abs(cond["weight"]))
    if "weight" in got:
        assert_close(got["weight"].numpy(), want[0].numpy(), cnd[0].numpy(), f"forward_block d_weight {tag}")
    if "comp" in got:
        assert_close(got["comp"].numpy(), want[1].numpy(), cnd[1].numpy(), f"forward_block d_comp {tag}")


def _data(n_src, n_dst, din, dout, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n_src, din, generator=g), torch.randn(n_dst, dout, generator=g)


WIDTHS = [(64, 64), (16, 16), (128, 128), (64, 16), (5, 3), (1, 1), (33, 100)]


@pytest.mark.parametrize("r", [1, 3, 33])
@pytest.mark.parametrize("din,dout", WIDTHS)
def test_widths_and_relations(din, dout, r):
    n_src, n_dst = 700, 300
    ei, et = B.bipartite_graph(n_src, n_dst, r, seed=din + r)
    conv = _conv(din, dout, r, seed=r)
    x, g = _data(n_src, n_dst, din, dout, 3)
    got = _run(conv, x, _block(ei, et, n_src, n_dst), g)
    assert set(got) == {"out", "x", "weight", "root", "bias"}
    _check(conv, x, ei, et, n_dst, g, got, "mean", f"{din}x{dout} r={r}")


@pytest.mark.parametrize("n_src,n_dst", [(1, 1), (40, 1), (90, 90)])
@pytest.mark.parametrize("din,dout", [(64, 64), (5, 3)])
def test_one_row_sides_and_square(din, dout, n_src, n_dst):
    ei, et = B.bipartite_graph(n_src, n_dst, 3, seed=5, e=400, hub=300, dup=20)
    conv = _conv(din, dout, 3)
    x, g = _data(n_src, n_dst, din, dout, 4)
    _check(conv, x, ei, et, n_dst, g, _run(conv, x, _block(ei, et, n_src, n_dst), g), "mean", f"{n_src}->{n_dst} {din}x{dout}")


@pytest.mark.parametrize("din,dout", [(64, 64), (5, 3)])
def test_no_edges_and_no_destinations(din, dout):
    conv = _conv(din, dout, 3)
    none = (torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    x, g = _data(9, 5, din, dout, 6)
    got = _run(conv, x, _block(*none, 9, 5), g)
    x64, g64 = x.double(), g.double()
    root, bias = conv.root.detach().cpu().double(), conv.bias.detach().cpu().double()
    assert_close(got["out"].numpy(), (x64[:5] @ root + bias).numpy(), (x64[:5].abs() @ root.abs() + bias.abs()).numpy(), "no edges: out")
    dx = torch.zeros(9, din, dtype=torch.float64)
    dx[:5] = g64 @ root.t()
    assert_close(got["x"].numpy(), dx.numpy(), None, "no edges: d_x")
    assert not bool(got["x"][5:].any()) and not bool(got["weight"].any())
    assert_close(got["root"].numpy(), (x64[:5].t() @ g64).numpy(), (x64[:5].abs().t() @ g64.abs()).numpy(), "no edges: d_root")
    assert_close(got["bias"].numpy(), g64.sum(0).numpy(), g64.abs().sum(0).numpy(), "no edges: d_bias")
    got = _run(conv, x[:4], _block(*none, 4, 0), g[:0])
    assert tuple(got["out"].shape) == (0, dout) and tuple(got["x"].shape) == (4, din)
    assert not any(bool(v.any()) for v in got.values())


OPTIONS = [dict(aggr="sum"), dict(num_bases=2), dict(num_blocks=True), dict(root_weight=False), dict(bias=False),
           dict(aggr="sum", num_bases=2, root_weight=False)]


@pytest.mark.parametrize("opt", OPTIONS, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
@pytest.mark.parametrize("din,dout", [(64, 64), (5, 3)])
def test_options(din, dout, opt):
    opt = dict(opt)
    if opt.get("num_blocks"):
        if (din, dout) == (5, 3):
            din, dout = 6, 3          # (blocks must divide both widths: 3 blocks of 2 x 1)
        opt["num_blocks"] = 4 if din == 64 else 3
    n_src, n_dst, r = 700, 300, 3
    ei, et = B.bipartite_graph(n_src, n_dst, r, seed=8)
    conv = _conv(din, dout, r, **opt)
    x, g = _data(n_src, n_dst, din, dout, 9)
    got = _run(conv, x, _block(ei, et, n_src, n_dst), g)
    assert ("root" in got) == (conv.root is not None) and ("bias" in got) == (conv.bias is not None) and ("comp" in got) == (conv.comp is not None)
    _check(conv, x, ei, et, n_dst, g, got, opt.get("aggr", "mean"), f"{din}x{dout} {opt}")


@pytest.mark.parametrize("din,dout", [(64, 64), (5, 3)])
def test_frozen_parameters_and_inputs(din, dout):
    n_src, n_dst, r = 700, 300, 3
    ei, et = B.bipartite_graph(n_src, n_dst, r, seed=8)
    x, g = _data(n_src, n_dst, din, dout, 9)
    block = _block(ei, et, n_src, n_dst)
    for frozen in ("weight", "comp", "root", "bias", None):
        conv = _conv(din, dout, r, num_bases=2)
        if frozen is not None:
            getattr(conv, frozen).requires_grad_(False)
        got = _run(conv, x, block, g, x_grad=frozen is not None)
        assert frozen is None or getattr(conv, frozen).grad is None
        assert ("x" in got) == (frozen is not None)
        assert set(got) - {"out", "x"} == {"weight", "comp", "root", "bias"} - {frozen}
        _check(conv, x, ei, et, n_dst, g, got, "mean", f"{din}x{dout} frozen {frozen}")


@pytest.mark.parametrize("din,dout", [(64, 64), (33, 100)])
def test_deterministic_and_prebuilt_index(din, dout):
    from scaling_rgcn_training_amd.sampling import block_index
    n_src, n_dst, r = 700, 300, 33
    ei, et = B.bipartite_graph(n_src, n_dst, r, seed=2)
    conv = _conv(din, dout, r)
    x, g = _data(n_src, n_dst, din, dout, 1)
    block = _block(ei, et, n_src, n_dst)
    a, b = _run(conv, x, block, g), _run(conv, x, block, g)
    c = _run(conv, x, block, g, index=block_index(block, r, "mean"))
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: two runs differ"
        assert torch.equal(a[k], c[k]), f"{k}: a prebuilt index changes the result"
    with pytest.raises(ValueError, match="index"):
        conv.forward_block(x.to(DEV), block, block_index(block, r, "sum"))


# ---- a sampler-made pair of blocks through the model, as tests/test_gpu_sampling.py::test_sampled_forward_and_gradients_match_float64
def test_sampled_blocks_through_the_model():
    from scaling_rgcn_training_amd.layers import Emb_Layers
    from scaling_rgcn_training_amd.sampling import NeighborSampler
    from scaling_rgcn_training_amd.trainer import do_nothing
    from tests.test_gpu_sampling import _net64
    n, e, r, emb, hid, lab = 2000, 20000, 5, 16, 12, 5
    ei, et = R.hub_graph(n, e, r, seed=9, hub_edges=1400)
    torch.manual_seed(0)
    model = Emb_Layers(r, hid, lab, n, emb, None)
    with torch.no_grad():
        model.rgcn1.bias.normal_(0, 0.1)
        model.rgcn2.bias.normal_(0, 0.1)
    params = {k: v.detach().clone().double() for k, v in model.state_dict().items()}
    model = model.to(DEV)
    gen = torch.Generator().manual_seed(1)
    seeds = torch.cat([torch.tensor([0]), 1 + torch.randperm(n - 1, generator=gen)[:63]])
    blocks = NeighborSampler(ei.to(DEV), et.to(DEV), n, r).sample(seeds.to(DEV), (5, -1), 2)
    cpu_blocks = [R.Block(*[t.cpu() if torch.is_tensor(t) else t for t in b]) for b in blocks]
    dg = torch.randn(seeds.numel(), lab, generator=gen)
    model.zero_grad()
    out = model.forward_blocks(blocks, do_nothing, block_kernels=True)
    out.backward(dg.to(DEV))
    torch.cuda.synchronize()

    def run(absolute):
        p = {k: (v.abs() if absolute else v).clone().requires_grad_(True) for k, v in params.items()}
        o = _net64(p, cpu_blocks)
        o.backward(dg.double().abs() if absolute else dg.double())
        return o.detach(), {k: v.grad for k, v in p.items()}

    ref, ref_g = run(False)
    cond, cond_g = run(True)
    assert_close(out.detach().cpu().numpy(), ref.numpy(), 2 * cond.numpy(), "forward_blocks(block_kernels=True)")
    for name, q in model.named_parameters():
        assert q.grad is not None, name
        assert_close(q.grad.cpu().numpy(), ref_g[name].numpy(), 4 * cond_g[name].numpy(), f"d_{name} block_kernels=True")
    touched = torch.zeros(n, dtype=torch.bool)
    touched[cpu_blocks[0].src_nodes] = True
    assert not bool(model.embedding.weight.grad.cpu()[~touched].any())
