"""Bipartite RGCNConv without a GPU: the fp64 reference helper against a direct restatement of PyG's bipartite loop, the
constructor's parameter shapes, every refusal that needs no device, ``target_block`` against a numpy loop, and the argument
refusals of rgcn_rows_transform / rgcn_rows_dw (host dummy pointers: every call stops at an argument check, nothing is launched)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import rgcn_oracle as O
from tests.bipartite_reference import bipartite_graph, device_reference, pyg_bipartite_loop, reference


# ---- the reference helper ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(300, 180), (180, 300), (200, 200)])
@pytest.mark.parametrize("aggr", ["mean", "sum"])
def test_reference_equals_pyg_bipartite_loop(sizes, aggr):
    n_src, n_dst = sizes
    r, in_src, in_dst, out = 5, 7, 5, 6
    ei, et = bipartite_graph(n_src, n_dst, r, seed=n_src + n_dst)
    assert int((ei[1] == 0).sum()) >= 600 and not bool((et == r - 1).any()) and int(ei[1].max()) < n_dst - 5
    trip = torch.stack([ei[0], ei[1], et]).t()
    assert trip.unique(dim=0).shape[0] < trip.shape[0]          # duplicate triples
    gen = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    xs, xd, w, root, bias, g = rnd(n_src, in_src), rnd(n_dst, in_dst), rnd(r, in_src, out), rnd(in_dst, out), rnd(out), rnd(n_dst, out)
    leaves = [t.clone().requires_grad_(True) for t in (xs, xd, w, root, bias)]
    y = pyg_bipartite_loop(leaves[0], leaves[1], ei, et, leaves[2], leaves[3], leaves[4], aggr)
    y.backward(g)
    ref, cond, cpu32 = reference(xs, xd, ei, et, w, root, bias, g, aggr)
    want = {"out": y.detach(), "x_src": leaves[0].grad, "x_dst": leaves[1].grad, "weight": leaves[2].grad, "root": leaves[3].grad,
            "bias": leaves[4].grad}
    for k, v in want.items():
        assert ref[k].shape == tuple(v.shape), k
        assert float(np.abs(ref[k] - v.numpy()).max()) < 1e-11 * max(1.0, float(np.abs(v.numpy()).max())), k
        assert cond[k].shape == ref[k].shape and bool((cond[k] >= np.abs(ref[k]) * (1 - 1e-12)).all()), k
        assert cpu32[k].shape == ref[k].shape and float(np.abs(cpu32[k] - ref[k]).max()) < 1e-3 * max(1.0, float(cond[k].max())), k


def test_reference_without_root_and_bias():
    ei, et = bipartite_graph(40, 30, 3, seed=0, e=200, hub=20, dup=5)
    gen = torch.Generator().manual_seed(2)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    xs, xd, w, g = rnd(40, 4), rnd(30, 3), rnd(3, 4, 5), rnd(30, 5)
    ref, cond, cpu32 = reference(xs, xd, ei, et, w, None, None, g)
    assert sorted(ref) == ["out", "weight", "x_src"]
    y = pyg_bipartite_loop(xs, xd, ei, et, w, None, None)
    assert float(np.abs(ref["out"] - y.numpy()).max()) < 1e-12


@pytest.mark.parametrize("sizes", [(300, 180), (180, 300)])
@pytest.mark.parametrize("aggr", ["mean", "sum"])
@pytest.mark.parametrize("root_bias", [(True, True), (False, False)])
def test_device_reference_equals_reference(sizes, aggr, root_bias, monkeypatch):
    """the torch form used past 2^24 rows (tests/test_gpu_bipartite_past_4gib.py) against the numpy composition, on the CPU:
    values, condition sums, and its fp32 evaluation within fp32 rounding of the float64 one; row blocks smaller than the sides"""
    from tests import bipartite_reference
    monkeypatch.setattr(bipartite_reference, "BATCH_ROWS", 32)      # (its batched float64 products, with a remainder, at these sizes)
    n_src, n_dst = sizes
    r, in_src, in_dst, out = 5, 7, 5, 6
    ei, et = bipartite_graph(n_src, n_dst, r, seed=n_src + 3 * n_dst)
    gen = torch.Generator().manual_seed(4)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    xs, xd, w, g = rnd(n_src, in_src), rnd(n_dst, in_dst), rnd(r, in_src, out), rnd(n_dst, out)
    root, bias = (rnd(in_dst, out) if root_bias[0] else None), (rnd(out) if root_bias[1] else None)
    ref, cond, _ = reference(xs, xd, ei, et, w, root, bias, g, aggr)
    got = device_reference(xs, xd, ei, et, w, root, bias, g, aggr, torch.float64, False, block=64)
    gcond = device_reference(xs, xd, ei, et, w, root, bias, g, aggr, torch.float64, True, block=64)
    g32 = device_reference(xs, xd, ei, et, w, root, bias, g, aggr, torch.float32, False, block=64)
    assert sorted(got) == sorted(ref) == sorted(gcond) == sorted(g32)
    for k in ref:
        assert tuple(got[k].shape) == ref[k].shape and got[k].dtype == torch.float64 and g32[k].dtype == torch.float32, k
        scale = max(1.0, float(np.abs(cond[k]).max()))
        assert float(np.abs(got[k].numpy() - ref[k]).max()) < 1e-12 * scale, k
        assert float(np.abs(gcond[k].numpy() - cond[k]).max()) < 1e-12 * scale, k
        assert float(np.abs(g32[k].double().numpy() - ref[k]).max()) < 1e-5 * scale, k
    assert not bool(got["weight"][r - 1].any())


# ---- constructor ---------------------------------------------------------------------------------------------------------------
def _conv(*a, **k):
    from scaling_rgcn_training_amd.conv import RGCNConv
    return RGCNConv(*a, **k)


def test_parameter_shapes_and_order():
    for kw, wshape in (({}, (5, 24, 16)), ({"num_bases": 3}, (3, 24, 16)), ({"num_blocks": 4}, (5, 4, 6, 4))):
        conv = _conv((24, 10), 16, 5, **kw)
        names = [n for n, _ in conv.named_parameters()]
        assert names == (["weight", "comp", "root", "bias"] if "num_bases" in kw else ["weight", "root", "bias"])
        assert tuple(conv.weight.shape) == wshape and tuple(conv.root.shape) == (10, 16) and tuple(conv.bias.shape) == (16,)
        assert conv.in_channels == 24 and conv.in_channels_l == 24 and conv.in_channels_r == 10
        assert isinstance(conv.in_channels, int)
        assert tuple(conv.effective_weight().shape) == (5, 24, 16)
        assert float(conv.root.detach().abs().max()) <= (6.0 / 26) ** 0.5 and float(conv.bias.detach().abs().max()) == 0.0       # PyG's glorot / zeros
    conv = _conv((24, 10), 16, 5, root_weight=False, bias=False)
    assert conv.root is None and conv.bias is None
    for pair in ((1, 128), (128, 1), (128, 128), (1, 1)):
        assert _conv(pair, 3, 2).in_channels_r == pair[1]


def test_equal_pair_is_the_plain_layer():
    torch.manual_seed(3)
    a = _conv((12, 12), 8, 4, num_bases=2)
    torch.manual_seed(3)
    b = _conv(12, 8, 4, num_bases=2)
    assert a.in_channels == b.in_channels == 12 and a.in_channels_l == b.in_channels_l == a.in_channels_r == b.in_channels_r == 12
    assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
    for (_, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p, q)
    assert repr(a) == repr(b)
    assert _conv((12, 12), 8, 4, aggr="max").aggr == "max"      # (the homogeneous max layer, as before)


def test_constructor_refusals():
    with pytest.raises(NotImplementedError):
        _conv((12, 8), 8, 4, aggr="max")
    with pytest.raises(NotImplementedError):
        _conv((12, 200), 8, 4, wide=True)
    with pytest.raises(NotImplementedError):
        _conv((200, 12), 8, 4, wide=True)
    with pytest.raises(NotImplementedError):
        _conv((12, 8), 300, 4, wide=True)
    for bad in ((12, 0), (12, 129), (0, 12), (129, 12)):
        with pytest.raises(ValueError):
            _conv(bad, 8, 4)
    with pytest.raises(ValueError):
        _conv((12, 8, 4), 8, 4)
    with pytest.raises(ValueError):
        _conv((12, 8), 8, 4, featureless=True)
    assert _conv((12, 8), 8, 4, wide=True).in_channels_r == 8       # both sides narrow: runs as without the flag


# ---- forward refusals that need no device ---------------------------------------------------------------------------------------
def _edges():
    return torch.tensor([[0, 1, 2], [1, 0, 1]]), torch.tensor([0, 1, 0])


def test_forward_refusals_without_a_device():
    ei, et = _edges()
    xs, xd = torch.randn(5, 12), torch.randn(4, 8)
    conv = _conv((12, 8), 6, 3)
    with pytest.raises(ValueError, match="pair"):
        conv(xs, ei, et)                                        # a plain tensor on an (a, b) layer
    with pytest.raises(NotImplementedError):
        _conv(12, 6, 3, featureless=True)((xs, xs), ei, et)
    with pytest.raises(NotImplementedError):
        _conv(12, 6, 3, aggr="max")((xs, xs), ei, et)
    with pytest.raises(NotImplementedError):
        _conv(200, 6, 3, wide=True)((torch.randn(5, 200), torch.randn(4, 200)), ei, et)
    dist_layer = _conv((12, 8), 6, 3)
    dist_layer.dist = object()
    with pytest.raises(NotImplementedError):
        dist_layer((xs, xd), ei, et)
    for kw in ({"_activation": "relu"}, {"_input_relu": True}, {"_grad_premasked": True}):
        with pytest.raises(ValueError):
            conv((xs, xd), ei, et, **kw)
    for pair in ((None, xd), (xs, None), (xs, torch.zeros(4, dtype=torch.int64)), (torch.zeros(5, 12, dtype=torch.int32), xd)):
        with pytest.raises(NotImplementedError):
            conv(pair, ei, et)
    for pair in ((xs[:, :11], xd), (xs, xd[:, :7]), (xs[0], xd), (xs, xd[None]), (xs, xd, xd), (xs.double(), xd)):
        with pytest.raises(ValueError):
            conv(pair, ei, et)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv((xs, xd), ei, et)                                  # CPU tensors: as every layer
    # a tuple on a layer built with an int is the same dispatch (both widths equal)
    with pytest.raises(ValueError):
        _conv(12, 6, 3)((xs, xd), ei, et)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _conv(12, 6, 3)((xs, torch.randn(4, 12)), ei, et)


# ---- target_block ---------------------------------------------------------------------------------------------------------------
def test_target_block_against_a_loop():
    from scaling_rgcn_training_amd import target_block
    n, r = 60, 4
    g = torch.Generator().manual_seed(5)
    ei = torch.randint(0, n, (2, 400), generator=g)
    et = torch.randint(0, r, (400,), generator=g)
    ei, et = torch.cat([ei, ei[:, :30]], 1), torch.cat([et, et[:30]])           # duplicates
    rows = torch.randperm(n, generator=g)[:17]
    sub, typ = target_block(ei, et, rows, n)
    pos = {int(v): i for i, v in enumerate(rows.tolist())}
    want = [(int(s), pos[int(d)], int(t)) for s, d, t in zip(ei[0].tolist(), ei[1].tolist(), et.tolist()) if int(d) in pos]
    got = list(zip(sub[0].tolist(), sub[1].tolist(), typ.tolist()))
    assert got == want and len(got) > 0
    assert len(set(want)) < len(want)                           # duplicates kept
    assert sub.dtype == torch.int64 and sub.is_contiguous() and sub.data_ptr() != ei.data_ptr()
    sub0, typ0 = target_block(ei, et, torch.zeros(0, dtype=torch.int64), n)
    assert tuple(sub0.shape) == (2, 0) and tuple(typ0.shape) == (0,)
    for bad in (torch.tensor([1, 2, 1]), torch.tensor([0, n]), torch.tensor([-1, 3]), torch.tensor([1, 2], dtype=torch.int32),
                torch.tensor([[1, 2]])):
        with pytest.raises(ValueError):
            target_block(ei, et, bad, n)


# ---- the two entry points: argument refusals ------------------------------------------------------------------------------------
_BUF = (ctypes.c_float * 64)()      # host memory the argument checks see as non-NULL and never read
OK, ERR_NULL, ERR_WIDTH, ERR_STRIDE, ERR_WORKSPACE = 0, -1, -2, -3, -6


def _lib_():
    from scaling_rgcn_training_amd import _lib
    return _lib.load()


def test_rows_transform_refusals():
    lib, p = _lib_(), ctypes.addressof(_BUF)
    tf = lambda x=p, ldx=16, din=16, w=p, add=p, lda=16, y=p, ldy=16, dout=16, rows=100: lib.rgcn_rows_transform(
        x, ldx, din, w, 0, add, lda, p, y, ldy, dout, rows, None)
    for width in (0, 129, -1):
        assert tf(din=width, ldx=132) == ERR_WIDTH and tf(dout=width, ldy=132, lda=132) == ERR_WIDTH
    for width, ld in ((16, 12), (5, 4), (128, 124), (16, 18)):
        assert tf(din=width, ldx=ld) == ERR_STRIDE
        assert tf(dout=width, ldy=ld, lda=128) == ERR_STRIDE
        assert tf(dout=width, ldy=128, lda=ld) == ERR_STRIDE
    assert tf(x=None) == ERR_NULL and tf(w=None) == ERR_NULL and tf(y=None) == ERR_NULL
    assert tf(add=None, lda=0, rows=0) == OK            # add is optional (its stride is then not read); no rows: nothing to do
    assert tf(rows=-1) != OK


def test_rows_dw_refusals():
    lib, p = _lib_(), ctypes.addressof(_BUF)
    need = lib.rgcn_rows_dw_workspace_bytes(16, 16)
    assert need > 0 and lib.rgcn_rows_dw_workspace_bytes(128, 128) >= 4 * 64 * 64 * 4
    for bad in ((0, 16), (16, 0), (129, 16), (16, 129), (-1, 16), (16, -1)):
        assert lib.rgcn_rows_dw_workspace_bytes(*bad) == 0
    dw = lambda x=p, ldx=16, din=16, g=p, ldg=16, dout=16, ws=p, nbytes=need, d_w=p: lib.rgcn_rows_dw(
        x, ldx, din, g, ldg, dout, 100, ws, nbytes, d_w, None)
    for width in (0, 129, -1):
        assert dw(din=width, ldx=132) == ERR_WIDTH and dw(dout=width, ldg=132) == ERR_WIDTH
    for width, ld in ((16, 12), (5, 4), (128, 124), (16, 18)):
        assert dw(din=width, ldx=ld) == ERR_STRIDE and dw(dout=width, ldg=ld) == ERR_STRIDE
    assert dw(x=None) == ERR_NULL and dw(g=None) == ERR_NULL and dw(ws=None) == ERR_NULL and dw(d_w=None) == ERR_NULL
    assert dw(nbytes=need - 1) == ERR_WORKSPACE
    assert dw(din=128, ldx=128, dout=128, ldg=128, nbytes=lib.rgcn_rows_dw_workspace_bytes(128, 128) - 1) == ERR_WORKSPACE


def test_bindings_declare_the_rows_entry_points():
    from scaling_rgcn_training_amd import _lib
    assert {"rgcn_rows_transform", "rgcn_rows_dw_workspace_bytes", "rgcn_rows_dw"} <= set(_lib.EXPORTS)
    assert callable(_lib.rows_transform) and callable(_lib.rows_dw)
    assert _lib.load().rgcn_abi_version() == 19
