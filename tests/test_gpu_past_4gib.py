"""The layer past 2^24 rows and 4 GiB: where the kernels' gathers leave buffer descriptors for 64-bit pointers.

Every HIP kernel reads its gathered matrix (x forward, dOut for dX / dW) through a buffer descriptor -- 32-bit byte offsets,
a 24-bit row multiply (__umul24) -- where csrc/rgcn_kernels_shared.h buffer_bytes allows it (rows < 2^24 and (rows + 1) * ld * 4
< 0xFFFFFF00, mirrored by _lib.buffer_addressable), and through 64-bit pointers elsewhere.  The host routes around the same rule
(no tile-major d_weight, no layout-3 plans, the edge-parallel path only up to eplan.EP_MAX_OWNED owned rows).  Here the real size
of the matrices, not a flag, picks the path:

  2^24 - 3 (64 x 64)        the last addressable row count: offsets up to 4 GiB - 512
  2^24 - 2 (64 x 64)        the first unaddressable one (by bytes)
  2^24 + 4099 (64 / 16)     rows >= 2^24 (at 16 columns by rows alone: 1 GiB of bytes)
  2^25 + 4099 (64 x 64)     more than 2^31 elements per matrix
  8,388,606 / 8,388,607     16 -> 128: x addressable, dOut addressable / not by its width

Each case asserts its regime from its inputs first, then compares whole tensors ON THE DEVICE with a float64 evaluation by plain
torch ops that shares nothing with the plans (per relation: index_add_ of w_e * feat[gather], then @ W_r; root, bias), under
bound (1) of oracle/tolerance.py (flat 1e-5 + 4 u cond, cond from the same sums over absolute values) and no worse than 2.5 x
the stock fp32 evaluation of the same sums (the factor of tests/test_gpu_fullsize.py).  Raw-ABI outputs start as NaN.  Graphs:
4M uniform edges plus 10^5 edges inside the top 2^16 rows, the last row as source and destination, duplicate triples and a
dead relation; x and dOut random (a wrapped 32-bit offset reads a different row)."""
import gc
import sys

import pytest
import torch

from oracle.tolerance import SLACK_LOG
from tests import kernel_variants as K

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CPU_FACTOR = 2.5            # tests/test_gpu_fullsize.py: no worse than 2.5 x the stock fp32 evaluation
BLK = 1 << 22               # rows per block of the whole-tensor passes (a float64 block of 64 columns: 2 GiB)
E_UNIFORM = 4_000_000
R_RAW = 8                   # raw-ABI graphs: relations 0..6, 7 dead
SPLIT = K.FLAG_SPLIT_PRODUCERS


def _release():
    from scaling_rgcn_training_amd.plan import clear_plan_cache
    sys.last_type = sys.last_value = sys.last_traceback = None      # (a failure's traceback holds its frame's tensors)
    gc.collect()
    clear_plan_cache()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _free_between_cases():
    """every case holds tens of GB: nothing of the previous one may stay alive"""
    _release()
    torch.cuda.reset_peak_memory_stats()
    yield
    print(f"\npeak device memory: {torch.cuda.max_memory_allocated() / 1e9:.1f} GB")
    _release()


def _dev():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from scaling_rgcn_training_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---- graph, inputs, float64 reference ---------------------------------------------------------------------------------
def make_graph(n, r, dev, seed, e=E_UNIFORM, skew=False):
    """uniform (or Zipf-tailed destinations: bench.synthetic_on_device's law) over [0, n), relation r - 1 dead; + 10^5 edges
    with both ends in the top 2^16 rows; the last row as source and destination; the first 50,000 triples once more"""
    g = torch.Generator(device=dev).manual_seed(seed)
    src = torch.randint(0, n, (e,), generator=g, device=dev)
    if skew:
        u = torch.rand(e, generator=g, device=dev, dtype=torch.float64)
        dst = (torch.floor(u.pow(-5.0)).clamp_(max=2.0 ** 62).to(torch.int64) - 1) % n
        del u
    else:
        dst = torch.randint(0, n, (e,), generator=g, device=dev)
    top = n - (1 << 16)
    src = torch.cat([src, torch.randint(top, n, (100_000,), generator=g, device=dev), torch.tensor([n - 1, n - 1, 0], device=dev)])
    dst = torch.cat([dst, torch.randint(top, n, (100_000,), generator=g, device=dev), torch.tensor([n - 1, 0, n - 1], device=dev)])
    et = torch.randint(0, r - 1, (src.numel(),), generator=g, device=dev)
    ei = torch.stack([src, dst])
    ei, et = torch.cat([ei, ei[:, :50_000]], 1).contiguous(), torch.cat([et, et[:50_000]])
    # float64 mean normaliser 1 / c[dst, rel] (duplicates counted) and the edges sorted by relation, for the reference
    _, inv, cnt = torch.unique(ei[1] * r + et, return_inverse=True, return_counts=True)
    perm = torch.argsort(et, stable=True)
    counts = torch.bincount(et, minlength=r).tolist()
    bounds, lo = [], 0
    for c in counts:
        bounds.append((lo, lo + c))
        lo += c
    assert counts[r - 1] == 0
    return dict(n=n, r=r, ei=ei, et=et, src_s=ei[0][perm], dst_s=ei[1][perm], w_s=(1.0 / cnt[inv].double())[perm], bounds=bounds)


def make_params(r, din, dout, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    bw, br = (6.0 / (din * dout)) ** 0.5, (6.0 / (din + dout)) ** 0.5
    w = torch.empty(r, din, dout, device=dev).uniform_(-bw, bw, generator=g)
    root = torch.empty(din, dout, device=dev).uniform_(-br, br, generator=g)
    bias = torch.randn(dout, generator=g, device=dev) * 0.1
    return w, root, bias


def make_features(n, d, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(n, d, generator=g, device=dev)


def aggregate(G, feat, w, root, bias, dtype, absval=False, transposed=False):
    """forward (transposed: dX) of the layer by plain torch ops in ``dtype``: per relation index_add_ of w_e feat[gather_e] @ W_r
    (W_r^T), + feat @ root (root^T) + bias; on absolute values: the condition sums of oracle/tolerance.py bound (1)"""
    f = (lambda t: t.abs()) if absval else (lambda t: t)
    n = feat.shape[0]
    gat, sca = (G["dst_s"], G["src_s"]) if transposed else (G["src_s"], G["dst_s"])
    we = G["w_s"].to(dtype)
    width = w.shape[1] if transposed else w.shape[2]
    out = torch.zeros(n, width, dtype=dtype, device=feat.device)
    for rel, (lo, hi) in enumerate(G["bounds"]):
        if hi > lo:
            wr = w[rel].to(dtype)
            rows = f(feat[gat[lo:hi]].to(dtype)) * we[lo:hi, None]
            out.index_add_(0, sca[lo:hi], rows @ f(wr.t() if transposed else wr))
    rm = f(root.to(dtype).t() if transposed else root.to(dtype))
    for lo in range(0, n, BLK):
        out[lo:lo + BLK] += f(feat[lo:lo + BLK].to(dtype)) @ rm
    if bias is not None and not transposed:
        out += f(bias.to(dtype))
    return out


def weight_grads(G, x, dg, dtype, absval=False):
    """d_weight[r] = H_r^T dOut (H_r: the rows w_e x[src_e] of relation r), d_root = x^T dOut, d_bias = column sums of dOut"""
    f = (lambda t: t.abs()) if absval else (lambda t: t)
    we = G["w_s"].to(dtype)
    dw = torch.zeros(G["r"], x.shape[1], dg.shape[1], dtype=dtype, device=x.device)
    for rel, (lo, hi) in enumerate(G["bounds"]):
        if hi > lo:
            dw[rel] = (f(x[G["src_s"][lo:hi]].to(dtype)) * we[lo:hi, None]).t() @ f(dg[G["dst_s"][lo:hi]].to(dtype))
    dr = torch.zeros(x.shape[1], dg.shape[1], dtype=dtype, device=x.device)
    db = torch.zeros(dg.shape[1], dtype=dtype, device=x.device)
    for lo in range(0, x.shape[0], BLK):
        dr += f(x[lo:lo + BLK].to(dtype)).t() @ f(dg[lo:lo + BLK].to(dtype))
        db += f(dg[lo:lo + BLK].to(dtype)).sum(0)
    return dw, dr, db


class Ref:
    """float64 value, its condition sums and the stock fp32 evaluation of one output"""
    def __init__(self, fn):
        self.ref, self.cond, self.stock = fn(torch.float64, False), fn(torch.float64, True), fn(torch.float32, False)

    @classmethod
    def of(cls, refs, i):
        """the i-th output of (float64, float64 on absolute values, fp32) evaluations"""
        return cls(lambda dt, a: refs[0][i] if dt == torch.float64 and not a else (refs[1][i] if a else refs[2][i]))


def check(name, got, R):
    """bound (1) of oracle/tolerance.py on every element, and the excess over flat 1e-5 no worse than 2.5 x the stock fp32 path's
    error; row blocks on the device, NaN fails"""
    ref, cond, stock = R.ref, R.cond, R.stock
    got = got[:, :ref.shape[1]] if got.dim() == 2 else got
    if ref.dim() != 2:
        got, ref, cond, stock = (t.reshape(-1, t.shape[-1]) for t in (got, ref, cond, stock))
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    bad, excess, stock_err = 0, float("-inf"), 0.0
    for lo in range(0, ref.shape[0], BLK):
        sl = slice(lo, lo + BLK)
        r = ref[sl]
        err = (got[sl].double() - r).abs()
        flat = 1e-5 + 1e-5 * r.abs()
        bad += int((~(err <= flat + 4 * U * cond[sl])).sum())
        excess = max(excess, float(torch.nan_to_num(err - flat, nan=float("inf")).max()))
        stock_err = max(stock_err, float((stock[sl].double() - r).abs().max()))
        del err, flat
    assert bad == 0, f"{name}: {bad} of {ref.numel()} elements outside flat 1e-5 + 4 u cond (worst excess over flat {excess:.3e})"
    assert excess <= CPU_FACTOR * stock_err, (f"{name}: excess over flat 1e-5 {excess:.3e} > {CPU_FACTOR} x the stock fp32 "
                                              f"evaluation's error {stock_err:.3e}")
    SLACK_LOG.append((name, excess, stock_err))
    print(f"\nslack {name}: worst excess over flat 1e-5 {excess:.3e}, stock fp32 error {stock_err:.3e}")


def nan_like(rows, cols, dev):
    return torch.full((rows, cols), float("nan"), device=dev)


def _status(fn):
    from scaling_rgcn_training_amd import _lib
    with pytest.raises(_lib.RgcnLibraryError) as ex:
        fn()
    return ex.value.status


# ---- raw ABI ------------------------------------------------------------------------------------------------------------
def _tile_target(plan, din, dout, flags, addressable):
    return K.run_tile(din, dout, plan.tile, plan.chunk, plan.chunk_rows, plan.layout, flags, addressable, plan.n_tiles)


def _fwd_dx(G, x, dg, w, root, bias, din, dout, runs, dev):
    """runs: [(plan pair, flags, expected forward target, expected dX target)]; an ("err", s) target must be refused with status s
    and leave its output NaN"""
    from scaling_rgcn_training_amd import _lib
    n = G["n"]
    pw, pwt = _lib.pack_weights(w, root, False), _lib.pack_weights(w, root, True)
    R = Ref(lambda dt, a: aggregate(G, x, w, root, bias, dt, a))
    out = nan_like(n, dout, dev)
    for pl, flags, tf, _ in runs:
        out.fill_(float("nan"))
        tag = f"out n={n} {din}x{dout} {tf[:4]} layout {pl.fwd.layout} flags {flags}"
        if tf[0] == "err":
            assert _status(lambda: _lib.fwd(_lib.plan_struct(pl.fwd), x, din, pw, bias, out, dout, 0, flags)) == tf[1], tag
            assert bool(out.isnan().all()), tag
            continue
        _lib.fwd(_lib.plan_struct(pl.fwd), x, din, pw, bias, out, dout, 0, flags)
        check(tag, out, R)
    del out, R
    R = Ref(lambda dt, a: aggregate(G, dg, w, root, None, dt, a, transposed=True))
    dx = nan_like(n, din, dev)
    for pl, flags, _, tb in runs:
        dx.fill_(float("nan"))
        tag = f"d_x n={n} {din}x{dout} {tb[:4]} layout {pl.bwd.layout} flags {flags}"
        if tb[0] == "err":
            assert _status(lambda: _lib.bwd_dx(_lib.plan_struct(pl.bwd), dg, dout, pwt, dx, din, None, flags)) == tb[1], tag
            assert bool(dx.isnan().all()), tag
            continue
        _lib.bwd_dx(_lib.plan_struct(pl.bwd), dg, dout, pwt, dx, din, None, flags)
        check(tag, dx, R)


def _relmajor_dw(G, x, dg, plan, din, dout, addressable, dev, flags=0):
    from scaling_rgcn_training_amd import _lib
    want = K.bwd_dw(din, dout, plan.tile, plan.chunk, plan.chunk_rows, plan.layout, flags, addressable, plan.n_tiles, plan.n_units)
    assert want[0] != "err", want
    r = G["r"]
    dw = torch.full((r, din, dout), float("nan"), device=dev)
    dr = torch.full((din, dout), float("nan"), device=dev)
    db = torch.full((dout,), float("nan"), device=dev)
    _lib.bwd_dw(_lib.plan_struct(plan), x, din, dg, dout, dw, dr, db, flags)
    refs = [weight_grads(G, x, dg, dt, a) for dt, a in ((torch.float64, False), (torch.float64, True), (torch.float32, False))]
    for i, (name, got) in enumerate((("d_weight", dw), ("d_root", dr), ("d_bias", db))):
        R = Ref.of(refs, i)
        check(f"{name} n={G['n']} {din}x{dout} {want[:5]}", got, R)
    assert bool((dw[r - 1] == 0).all()), "the dead relation"
    return refs


@pytest.mark.parametrize("n", [(1 << 24) - 3, (1 << 24) - 2], ids=["2^24-3", "2^24-2"])
def test_raw_abi_at_the_last_addressable_row(n):
    """64 x 64 at the descriptor's edge: rgcn_tile3p_kernel (tile 272 / 112-row chunks, layouts 0 and 3), the exact tile kernel,
    dX both ways, relation-major d_weight, the tile-major d_weight on a layout-0 and a layout-5 plan in both forms -- and one row
    more, where the same calls fall through to the exact pointer kernel or are refused"""
    from scaling_rgcn_training_amd import _lib, plan as P
    dev = _dev()
    addressable = n == (1 << 24) - 3
    assert _lib.buffer_addressable(n, 64) == addressable
    if addressable:
        assert (n + 1) * 64 * 4 == (1 << 32) - 512         # the gather's last padding row ends 512 bytes short of 4 GiB
    G = make_graph(n, R_RAW, dev, seed=n)
    x, dg = make_features(n, 64, dev, 1), make_features(n, 64, dev, 2)
    w, root, bias = make_params(R_RAW, 64, 64, dev, 3)
    p0 = P.build_graph_plans_device(G["ei"], G["et"], n, R_RAW, 272, chunk=P.CHUNK_112, split=0)
    p3 = P.build_graph_plans_device(G["ei"], G["et"], n, R_RAW, 272, chunk=P.CHUNK_112, split=3)
    runs = []
    for pl in (p0, p3):
        assert (pl.fwd.tile, pl.fwd.chunk, pl.fwd.chunk_rows, pl.fwd.layout) == (272, 128, 112, pl.bwd.layout)
        for flags in (SPLIT, 0):
            tf, tb = (_tile_target(pl.fwd, 64, 64, flags, addressable), _tile_target(pl.bwd, 64, 64, flags, addressable))
            if addressable:
                want = ("tile3p", 7, pl.fwd.layout, True) if flags else ("tile", 64, 64, 2, True, 128, pl.fwd.layout == 3)
                assert tf == tb == want, (tf, tb, want)
            elif pl.fwd.layout == 3:
                assert tf == tb == K.err(K.ERR_PLAN)       # layout 3 gathers through descriptors only
            else:
                assert tf == tb == ("tile", 64, 64, 2, False, 128, False)     # the split flag falls through to the pointer kernel
            runs.append((pl, flags, tf, tb))
    _fwd_dx(G, x, dg, w, root, bias, 64, 64, runs, dev)
    del p3, runs
    refs = _relmajor_dw(G, x, dg, p0.fwd, 64, 64, addressable, dev)
    del p0
    # the tile-major kernel: a layout-0 plan of its tile and the layout-5 pair plan, both forms
    t_dw = _lib.dw_tiles_geometry()[0]
    pt = P.build_graph_plans_device(G["ei"], G["et"], n, R_RAW, t_dw, chunk=64, dw_tiles=True)
    R = Ref.of(refs, 0)
    for pl, walk in ((pt.fwd, _lib.dw_tiles_walk(_lib.plan_struct(pt.fwd), dev)), (pt.dw, pt.dw_walk)):
        for flags in (SPLIT, 0):
            want = K.bwd_dw_tiles(64, 64, pl.tile, pl.chunk, pl.chunk_rows, pl.layout, flags, addressable, pl.n_tiles, R_RAW)
            dw = torch.full((R_RAW, 64, 64), float("nan"), device=dev)
            if not addressable:
                assert want == K.err(K.ERR_ADDRESS)
                assert _status(lambda: _lib.bwd_dw_tiles(_lib.plan_struct(pl), walk, x, 64, dg, 64, dw, flags)) == K.ERR_ADDRESS
                assert bool(dw.isnan().all())
                continue
            assert want == ("dw_tiles", bool(flags), pl.layout == 5)
            _lib.bwd_dw_tiles(_lib.plan_struct(pl), walk, x, 64, dg, 64, dw, flags)
            check(f"d_weight (tile-major) n={n} {want}", dw, R)


@pytest.mark.parametrize("width", [64, 16])
def test_raw_abi_rows_past_2_24(width):
    """n = 2^24 + 4099: row indices past __umul24's 24 bits.  At 16 columns the matrices are 1 GiB -- only the row rule keeps them
    off the descriptors.  64 x 64 also: rgcn_bwd_dw_root over every row, and the edge-parallel path over an owned range of exactly
    2^24 rows (the top rows) that gathers from all n rows -- the builder refuses one row more"""
    from scaling_rgcn_training_amd import _lib, eplan as E, plan as P
    dev = _dev()
    n, d = (1 << 24) + 4099, width
    assert not _lib.buffer_addressable(n, d)
    if d == 16:
        assert (n + 1) * d * 4 < 0xFFFFFF00         # by bytes it would fit: the row rule alone sends it to the pointer path
    G = make_graph(n, R_RAW, dev, seed=n + d)
    x, dg = make_features(n, d, dev, 11), make_features(n, d, dev, 12)
    w, root, bias = make_params(R_RAW, d, d, dev, 13)
    tile, chunk = (272, P.CHUNK_112) if d == 64 else (512, 64)
    pl = P.build_graph_plans_device(G["ei"], G["et"], n, R_RAW, tile, chunk=chunk)
    runs = []
    for flags in ((SPLIT, 0) if d == 64 else (0,)):
        tf, tb = _tile_target(pl.fwd, d, d, flags, False), _tile_target(pl.bwd, d, d, flags, False)
        assert tf == tb and tf[0] == "tile" and tf[4] is False, tf
        runs.append((pl, flags, tf, tb))
    _fwd_dx(G, x, dg, w, root, bias, d, d, runs, dev)
    _relmajor_dw(G, x, dg, pl.fwd, d, d, False, dev)
    del pl, runs
    if d != 64:
        return
    # d_root / d_bias by the plan-free streaming kernel over all n rows
    dr, db = torch.full((d, d), float("nan"), device=dev), torch.full((d,), float("nan"), device=dev)
    _lib.bwd_dw_root(x, d, dg, d, dr, db)
    refs = [weight_grads(dict(G, bounds=[]), x, dg, dt, a) for dt, a in ((torch.float64, False), (torch.float64, True),
                                                                          (torch.float32, False))]
    for i, (name, got) in enumerate((("d_root", dr), ("d_bias", db)), start=1):
        R = Ref.of(refs, i)
        check(f"{name} (rgcn_bwd_dw_root) n={n}", got, R)
    # the edge-parallel path over the top 2^24 rows, gathering from every row
    b = n - E.EP_MAX_OWNED
    gp = P.build_graph_plans_device(G["ei"], G["et"], n, R_RAW, 272, fwd_range=(b, n), bwd_range=(b, n), paths=("ep", "ep"))
    assert gp.ep_fwd.n_owned == gp.ep_bwd.n_owned == 1 << 24 and gp.ep_fwd.heavy is None
    assert K.ep_transform(d, d, 16, 64, 0, 2, SPLIT, False, 1) == ("ep", 64, 64)
    pw, pwt = _lib.pack_weights(w, root, False), _lib.pack_weights(w, root, True)
    R = Ref(lambda dt, a: aggregate(G, x, w, root, bias, dt, a)[b:].contiguous())
    out = nan_like(1 << 24, d, dev)
    _lib.ep_layer(gp.ep_fwd, x, d, pw, bias, out, d, 0, None, SPLIT)
    check(f"out (edge-parallel, rows [{b}, n)) n={n}", out, R)
    R = Ref(lambda dt, a: aggregate(G, dg, w, root, None, dt, a, transposed=True)[b:].contiguous())
    out.fill_(float("nan"))
    _lib.ep_layer(gp.ep_bwd, dg, d, pwt, None, out, d, 0, None, SPLIT)
    check(f"d_x (edge-parallel, rows [{b}, n)) n={n}", out, R)
    del out, R, gp
    graph, keep = _lib.graph_struct(G["ei"], G["et"], n, R_RAW)
    ws = _lib.plan_workspace(int(G["et"].numel()), E.EP_MAX_OWNED + 1, R_RAW, 16, dev)
    wts = _lib.edge_weights(graph, "mean", ws)
    assert _status(lambda: _lib.plan_build(graph, wts, False, b - 1, n, 16, 64, ws, 2)) == K.ERR_PLAN
    with pytest.raises(ValueError, match="EP_MAX_OWNED"):
        P.build_graph_plans_device(G["ei"], G["et"], n, R_RAW, 272, fwd_range=(b - 1, n), paths=("ep", "ring"))


def test_raw_abi_past_2_31_elements():
    """n = 2^25 + 4099 at 64 x 64: 8.6 GB per matrix, element offsets past 2^31 -- forward and dX on the exact tile kernel's
    pointer path, relation-major d_weight"""
    from scaling_rgcn_training_amd import _lib, plan as P
    dev = _dev()
    n = (1 << 25) + 4099
    assert not _lib.buffer_addressable(n, 64) and n * 64 > 1 << 31
    G = make_graph(n, R_RAW, dev, seed=n)
    x, dg = make_features(n, 64, dev, 21), make_features(n, 64, dev, 22)
    w, root, bias = make_params(R_RAW, 64, 64, dev, 23)
    pl = P.build_graph_plans_device(G["ei"], G["et"], n, R_RAW, 272, chunk=P.CHUNK_112)
    tf, tb = _tile_target(pl.fwd, 64, 64, 0, False), _tile_target(pl.bwd, 64, 64, 0, False)
    assert tf == tb == ("tile", 64, 64, 2, False, 128, False)
    _fwd_dx(G, x, dg, w, root, bias, 64, 64, [(pl, 0, tf, tb)], dev)
    _relmajor_dw(G, x, dg, pl.fwd, 64, 64, False, dev)


@pytest.mark.parametrize("n", [8_388_606, 8_388_607])
def test_raw_abi_4gib_by_width(n):
    """16 -> 128: x (16 columns) is addressable, dOut (128 columns) is at 8,388,606 rows and is not one row later -- forward, dX and
    relation-major d_weight at KP / NP 128"""
    from scaling_rgcn_training_amd import _lib, plan as P
    dev = _dev()
    din, dout = 16, 128
    x_buf, g_buf = _lib.buffer_addressable(n, din), _lib.buffer_addressable(n, dout)
    assert x_buf and g_buf == (n == 8_388_606)
    G = make_graph(n, R_RAW, dev, seed=n)
    x, dg = make_features(n, din, dev, 31), make_features(n, dout, dev, 32)
    w, root, bias = make_params(R_RAW, din, dout, dev, 33)
    pl = P.build_graph_plans_device(G["ei"], G["et"], n, R_RAW, 272, chunk=64)
    tf, tb = _tile_target(pl.fwd, din, dout, 0, x_buf), _tile_target(pl.bwd, dout, din, 0, g_buf)
    assert tf == ("tile", 16, 128, 4, True, 64, False) and tb == ("tile", 128, 16, 2, g_buf, 64, False), (tf, tb)
    _fwd_dx(G, x, dg, w, root, bias, din, dout, [(pl, 0, tf, tb)], dev)
    _relmajor_dw(G, x, dg, pl.fwd, din, dout, x_buf and g_buf, dev)


# ---- the device plan builder ---------------------------------------------------------------------------------------------
def test_plan_builder_25_bit_ids_and_33_bit_weight_keys():
    """n = 2^24 + 4099: 25-bit node ids in every sort key.  Layout 0 over the whole graph, layouts 3 and 5 over the top tiles (their
    torch twins walk chunks in Python), all bit-identical to the torch twin; the mean weights at 267 relations, where the
    (destination, relation) key n R passes 2^32"""
    from scaling_rgcn_training_amd import _lib, plan as P
    from tests.test_gpu_plan_build import _compare
    dev = _dev()
    n = (1 << 24) + 4099
    G = make_graph(n, 32, dev, seed=5, e=4_000_000)
    ei, et = G["ei"], G["et"]
    _compare(ei, et, n, 32, 272, P.CHUNK_112, split=0)
    b3 = (n // 272 - 8) * 272
    _compare(ei, et, n, 32, 272, P.CHUNK_112, fr=(b3, n), br=(b3, n), split=3)
    t_dw = _lib.dw_tiles_geometry()[0]
    b5 = (n // t_dw - 8) * t_dw
    plans = _compare(ei, et, n, 32, t_dw, 64, fr=(b5, n), br=(b5, n), split=5)
    assert int((plans.fwd.slot_src2 < n).sum()) > 0, "no pair was formed"
    assert int(torch.where(plans.fwd.slot_src < n, plans.fwd.slot_src, 0).max()) >= 1 << 24, "25-bit ids gathered"
    del plans, G
    r = 267
    assert n * r > 1 << 32
    G = make_graph(n, r, dev, seed=6, e=4_000_000)
    graph, keep = _lib.graph_struct(G["ei"], G["et"], n, r)
    ws = _lib.plan_workspace(int(G["et"].numel()), 1, r, 16, dev)
    got = _lib.edge_weights(graph, "mean", ws)
    want = P.edge_weights(G["ei"][0], G["ei"][1], G["et"], r)
    assert torch.equal(got, want), int((got != want).sum())
    ref = torch.empty_like(G["w_s"])
    ref[torch.argsort(G["et"], stable=True)] = G["w_s"]
    assert torch.equal(got, ref.float())
    _compare(G["ei"], G["et"], n, r, 272, 64, split=0)


# ---- the module, default flags, path "auto" -----------------------------------------------------------------------------
MODULE_CASES = [("uniform", 32, (1 << 24) + 4099), ("hub", 32, (1 << 24) + 4099), ("uniform", 267, (1 << 24) + 4099),
                ("uniform", 32, (1 << 25) + 4099)]


@pytest.mark.parametrize("kind,r,n", MODULE_CASES, ids=[f"{k}-{r}rel-n{n}" for k, r, n in MODULE_CASES])
def test_module_auto_path_past_2_24(kind, r, n):
    """RGCNConv(64, 64, R) with its defaults on one GPU: both directions on the tile kernels (the edge-parallel plan holds at most
    2^24 rows), forward and every gradient against float64; a pinned path 'ep' is refused before any plan is built"""
    from scaling_rgcn_training_amd import eplan as E
    from scaling_rgcn_training_amd.conv import RGCNConv
    dev = _dev()
    d = 64
    G = make_graph(n, r, dev, seed=n + r, skew=kind == "hub")
    ei, et = G["ei"], G["et"]
    if kind == "hub":
        assert int(torch.bincount(ei[1], minlength=n).max()) > 300_000
    conv = RGCNConv(d, d, r).to(dev)
    w, root, bias = make_params(r, d, d, dev, 41)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.root.copy_(root)
        conv.bias.copy_(bias)
    assert conv.path == "auto" and conv.kernel_flags == 0
    x, dg = make_features(n, d, dev, 42), make_features(n, d, dev, 43)
    xg = x.detach().requires_grad_(True)         # (the same storage: x stays the reference's input)
    out = conv(xg, ei, et)
    plans = conv._plans(xg, ei, et)
    assert plans.fwd is not None and plans.bwd is not None and plans.ep_fwd is None and plans.ep_bwd is None, "both directions ring"
    assert plans.dw is None, "no tile-major d_weight past the descriptor's range"
    tile, chunk = conv.layout(n, int(et.numel()))
    assert E.decide_paths(ei, n, r, d, d, tile, chunk) == ("ring", "ring")
    out.backward(dg)
    del plans
    tag = f"[{kind} {r} rel n={n}]"
    R = Ref(lambda dt, a: aggregate(G, x, w, root, bias, dt, a))
    check(f"module out {tag}", out.detach(), R)
    del out, R
    R = Ref(lambda dt, a: aggregate(G, dg, w, root, None, dt, a, transposed=True))
    check(f"module d_x {tag}", xg.grad, R)
    del R
    xg.grad = None
    refs = [weight_grads(G, x, dg, dt, a) for dt, a in ((torch.float64, False), (torch.float64, True), (torch.float32, False))]
    for i, (name, got) in enumerate((("d_weight", conv.weight.grad), ("d_root", conv.root.grad), ("d_bias", conv.bias.grad))):
        R = Ref.of(refs, i)
        check(f"module {name} {tag}", got, R)
    assert bool((conv.weight.grad[r - 1] == 0).all()), "the dead relation"
    if (kind, r, n) == MODULE_CASES[0]:
        conv.path = "ep"
        with pytest.raises(ValueError, match="EP_MAX_OWNED"):
            conv(x, ei, et)
        conv.path = ("ring", "ep")
        with pytest.raises(ValueError, match="EP_MAX_OWNED"):
            conv(x, ei, et)
