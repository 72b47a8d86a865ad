"""The bipartite layer past 2^24 rows and 4 GiB, in the manner of tests/test_gpu_past_4gib.py (whose conventions, ``check`` and
memory fixture are used as they are): its natural use is a huge x_src with few target rows.

  the kernels behind rgcn_rows_transform and rgcn_rows_dw through the binding, rows = 2^24 + 4099 ("Row offsets are 64-bit: rows x ld may pass 2^31"):
    3 -> 5      rows past 2^24 alone (0.27 / 0.54 GB per matrix)
    64 -> 4     x passes 2^32 bytes, y / add / g do not
    4 -> 64     y / add / g pass 2^32 bytes, x does not
    128 -> 8    x holds more than 2^31 elements
  the module, (N_src, N_dst) = (2^24 + 4099, 50,000) and (50,000, 2^24 + 4099), 16 / 16 -> 16, 5 relations, about 10^6 edges that
  include the last source row and the last destination row, duplicate triples and a dead relation; path "ring" and the default
  "auto", which must stay off the edge-parallel path past eplan.EP_MAX_OWNED: _BipartiteFn pads x_src or g to max(N_src, N_dst)
  rows, takes gp[:n_dst] and cuts dxp to [:n_src] on top of the kernels' own row arithmetic.

Each case asserts its regime from its sizes first, then compares whole tensors ON THE DEVICE, in row blocks, with a float64
evaluation by plain torch ops (tests/bipartite_reference.device_reference for the layer: it shares nothing with the plans) under
bound (1) of oracle/tolerance.py and no worse than 2.5 x the stock fp32 evaluation of the same sums.  Outputs start as NaN."""
import pytest
import torch

from tests.bipartite_reference import device_reference, tall_t_matmul
from tests.test_gpu_bipartite import _bound1
from tests.test_gpu_past_4gib import BLK, Ref, _dev, _free_between_cases, check, make_features, nan_like  # noqa: F401  (the fixture: autouse)

pytestmark = pytest.mark.gpu

ROWS = (1 << 24) + 4099
NAN = float("nan")
KERNEL_WIDTHS = [(3, 5), (64, 4), (4, 64), (128, 8)]


def _r4(w):
    return (w + 3) // 4 * 4


def _padded_features(rows, width, dev, seed):
    """[rows, width rounded up to 4] random values, the pad columns zero"""
    t = make_features(rows, _r4(width), dev, seed)
    t[:, width:] = 0
    return t


def _regime(din, dout):
    """the sizes the case claims, from its inputs"""
    xb, yb = ROWS * _r4(din) * 4, ROWS * _r4(dout) * 4
    assert ROWS > 1 << 24
    assert ((din, dout) == (3, 5)) == (xb < 1 << 32 and yb < 1 << 32), "rows past 2^24 alone"
    if (din, dout) == (64, 4):
        assert xb > 1 << 32 > yb
    if (din, dout) == (4, 64):
        assert yb > 1 << 32 > xb
    if (din, dout) == (128, 8):
        assert ROWS * _r4(din) > 1 << 31 and yb < 1 << 32
    print(f"\nrows {ROWS}, {din} -> {dout}: x {xb / 2 ** 30:.2f} GiB ({ROWS * _r4(din)} elements), y / g {yb / 2 ** 30:.2f} GiB")


def _spots(ld):
    """row slices named by the issue: the first 16 rows, the last 4,099 and, where the matrix passes it, the rows around byte
    offset 2^32"""
    s = {"first 16 rows": slice(0, 16), "last 4,099 rows": slice(ROWS - 4099, ROWS)}
    if ROWS * ld * 4 > 1 << 32:
        r = (1 << 32) // (ld * 4)
        s["rows around byte 2^32"] = slice(r - 64, r + 64)
    return s


def _blocks(fn, rows=ROWS):
    return torch.cat([fn(slice(lo, min(lo + BLK, rows))) for lo in range(0, rows, BLK)])


@pytest.mark.parametrize("din,dout", KERNEL_WIDTHS)
def test_rows_transform_past_2_24_rows(din, dout):
    from scaling_rgcn_training_amd import _lib
    dev = _dev()
    _regime(din, dout)
    x = _padded_features(ROWS, din, dev, 51)
    g = torch.Generator(device=dev).manual_seed(52)
    w = torch.randn(din, dout, generator=g, device=dev)
    bias = torch.randn(dout, generator=g, device=dev)
    wt = w.t().contiguous()
    add0 = _padded_features(ROWS, dout, dev, 53)

    def xw(dt, absval, with_add):
        f = (lambda t: t.abs()) if absval else (lambda t: t)
        wm, bs = f(w.to(dt)), f(bias.to(dt))
        return _blocks(lambda sl: f(x[sl, :din].to(dt)) @ wm + bs + (f(add0[sl, :dout].to(dt)) if with_add else 0))

    spots = dict(_spots(_r4(din)), **_spots(_r4(dout)))
    for with_add in (False, True):
        R = Ref(lambda dt, a: xw(dt, a, with_add))
        for transpose in ((False, True) if not with_add else (False,)):
            add = add0.clone() if with_add else None               # aliased to y: a lane reads the 16 bytes it stores later
            y = add if with_add else nan_like(ROWS, _r4(dout), dev)
            _lib.rows_transform(x, din, wt if transpose else w, dout, transpose=transpose, add=add, bias=bias, y=y)
            tag = f"rows_transform rows={ROWS} {din}->{dout} transpose={transpose} add={'aliased' if with_add else 'none'}"
            for name, sl in spots.items():
                _bound1(y[sl, :dout], R.ref[sl], R.cond[sl], f"{tag}, {name}")
            check(tag, y, R)
            assert not bool(y[:, dout:].any()), "pad columns: 0"
            del y, add
        del R


@pytest.mark.parametrize("din,dout", KERNEL_WIDTHS)
def test_rows_dw_past_2_24_rows(din, dout):
    from scaling_rgcn_training_amd import _lib
    lib = _lib.load()
    dev = _dev()
    _regime(din, dout)
    # every range of the kernel runs many trips of its double batch: 2048 / nq ranges of more than 4,096 k-steps
    nq = ((din + 63) // 64) * ((dout + 63) // 64)
    ws_bytes = lib.rgcn_rows_dw_workspace_bytes(din, dout)
    parts = ws_bytes // (4 * 64 * 64) // nq
    assert (ROWS + 3) // 4 // parts >= 2048 * nq
    x, g = _padded_features(ROWS, din, dev, 61), _padded_features(ROWS, dout, dev, 62)

    def xtg(dt, absval):
        f = (lambda t: t.abs()) if absval else (lambda t: t)
        if dt == torch.float32:       # the stock product: one fp32 matmul over all rows
            return x[:, :din].t() @ g[:, :dout]
        acc = torch.zeros(din, dout, dtype=dt, device=dev)
        for lo in range(0, ROWS, BLK):
            acc += tall_t_matmul(f(x[lo:lo + BLK, :din].to(dt)), f(g[lo:lo + BLK, :dout].to(dt)))
        return acc

    R = Ref(xtg)
    d_w = torch.full((din, dout), NAN, device=dev)
    ws = torch.full((ws_bytes // 4,), NAN, device=dev)
    _lib.check(lib.rgcn_rows_dw(x.data_ptr(), x.stride(0), din, g.data_ptr(), g.stride(0), dout, ROWS, ws.data_ptr(), ws_bytes,
                                d_w.data_ptr(), torch.cuda.current_stream().cuda_stream), "rgcn_rows_dw")
    check(f"rows_dw rows={ROWS} {din}x{dout}", d_w, R)


# ---- the module ----------------------------------------------------------------------------------------------------------------
R_LAYER, D = 5, 16
SMALL = 50_000
LAYER_SIZES = [(ROWS, SMALL), (SMALL, ROWS)]


def _graph(n_src, n_dst, dev, seed, e=1_000_000):
    g = torch.Generator(device=dev).manual_seed(seed)
    src = torch.cat([torch.randint(0, n_src, (e,), generator=g, device=dev), torch.tensor([n_src - 1, n_src - 1, 0], device=dev)])
    dst = torch.cat([torch.randint(0, n_dst, (e,), generator=g, device=dev), torch.tensor([n_dst - 1, 0, n_dst - 1], device=dev)])
    et = torch.randint(0, R_LAYER - 1, (src.numel(),), generator=g, device=dev)
    ei = torch.stack([src, dst])
    return torch.cat([ei, ei[:, :50_000]], 1).contiguous(), torch.cat([et, et[:50_000]])


@pytest.mark.parametrize("path", ["ring", "auto"])
@pytest.mark.parametrize("n_src,n_dst", LAYER_SIZES, ids=["src-past-2^24", "dst-past-2^24"])
def test_layer_past_2_24_rows(n_src, n_dst, path):
    from scaling_rgcn_training_amd import _lib, eplan as E
    from scaling_rgcn_training_amd.conv import RGCNConv
    dev = _dev()
    n = max(n_src, n_dst)
    assert n == ROWS > E.EP_MAX_OWNED == 1 << 24 and min(n_src, n_dst) == SMALL and not _lib.buffer_addressable(n, D)
    ei, et = _graph(n_src, n_dst, dev, seed=n_src % 1000 + 7)
    assert int(ei[0].max()) == n_src - 1 and int(ei[1].max()) == n_dst - 1 and int((et == R_LAYER - 1).sum()) == 0
    trip = (ei[0] * n_dst + ei[1]) * R_LAYER + et
    assert trip.unique().numel() < trip.numel(), "duplicate triples"
    del trip
    torch.manual_seed(3)
    conv = RGCNConv((D, D), D, R_LAYER).to(dev)
    with torch.no_grad():
        conv.bias.uniform_(-1, 1)
    assert conv.path == "auto" and conv.kernel_flags == 0
    conv.path = path
    xs, xd, g = make_features(n_src, D, dev, 71), make_features(n_dst, D, dev, 72), make_features(n_dst, D, dev, 73)
    ls, ld = xs.detach().requires_grad_(True), xd.detach().requires_grad_(True)     # (the same storage: xs, xd stay the reference's inputs)
    out = conv((ls, ld), ei, et)
    # ---- the route: both directions on the tile kernels, whole-side ranges on the square graph of n nodes
    plans = conv._bipartite_plans(ei, et, n_src, n_dst)
    assert plans.fwd is not None and plans.bwd is not None and plans.ep_fwd is None and plans.ep_bwd is None, "both directions ring"
    assert plans.dw is None
    assert (plans.fwd.n_nodes, plans.fwd.node_begin, plans.fwd.node_end) == (n, 0, n_dst)
    assert (plans.bwd.n_nodes, plans.bwd.node_begin, plans.bwd.node_end) == (n, 0, n_src)
    route = conv._route(n, int(et.numel()), True, plain=True)
    print(f"\n({n_src}, {n_dst}) path {path}: tile {route.tile} chunk {route.chunk} paths {route.paths}")
    if path == "auto":
        assert E.decide_paths(ei, n, R_LAYER, D, D, route.tile, route.chunk) == ("ring", "ring")
    del plans
    out.backward(g)
    torch.cuda.synchronize()
    got = {"out": out.detach(), "x_src": ls.grad, "x_dst": ld.grad, "weight": conv.weight.grad, "root": conv.root.grad, "bias": conv.bias.grad}
    assert tuple(got["out"].shape) == (n_dst, D) and tuple(got["x_src"].shape) == (n_src, D) and tuple(got["x_dst"].shape) == (n_dst, D)
    w, root, bias = conv.weight.detach(), conv.root.detach(), conv.bias.detach()
    refs = [device_reference(xs, xd, ei, et, w, root, bias, g, "mean", dt, a, block=BLK)
            for dt, a in ((torch.float64, False), (torch.float64, True), (torch.float32, False))]
    tag = f"[({n_src}, {n_dst}) path {path}]"
    for name in ("out", "x_src", "x_dst", "weight", "root", "bias"):
        check(f"bipartite {'d_' if name != 'out' else ''}{name} {tag}", got[name], Ref.of(refs, name))
    assert bool((got["weight"][R_LAYER - 1] == 0).all()), "the dead relation"
    if path == "ring" and n_src == ROWS:
        conv.path = "ep"                        # the dX direction would own more than EP_MAX_OWNED rows: refused before any plan
        with pytest.raises(ValueError, match="EP_MAX_OWNED"):
            conv((xs, xd), ei, et)
