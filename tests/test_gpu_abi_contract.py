"""Where the C ABI's kernels read and write (include/rgcn_mi355x.h), checked through the raw entry points.

Every operand lives inside a larger allocation whose bytes outside the operand hold a sentinel bit pattern (a NaN with a payload
of its own): guard rows before and after, and the columns between round4(width) and the row stride.  After each call the
sentinels must be intact bit for bit, the output pad columns [width, round4(width)) must be +0.0, inputs must be unchanged, and
the values inside must pass oracle/tolerance.py's criterion against the float64 oracle.  A read of a sentinel -- a gathered
padding row n_nodes, a column past round4(width), a row past the operand -- poisons the result with NaN.

Also here: the layout x entry point table (which plan each entry point walks, which it refuses), partitioned plans writing
adjacent row slices of one shared buffer, workspaces of exactly the queried size, and a hipGraph capture from a cold process.
Needs an MI355X: ``pytest -m gpu``."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import rgcn_oracle as O
from oracle.tolerance import abs_condition, assert_close, cpu32_reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0x7FC0DEAD          # a quiet NaN with a payload: neither a stored NaN nor a stored zero looks like it
G = 16                     # guard rows before every matrix (and after inputs)
G_OUT = 352                # guard rows after outputs: the last tile of a plan may reach up to `tile` rows past n_owned
WS_TAIL = 4096             # sentinel bytes after a workspace
N, E, R = 700, 7000, 5     # 700 = 10 x 64 + 60: every plan below has a partial last tile
OK, ERR_WIDTH, ERR_PLAN, ERR_LDS, ERR_WORKSPACE = 0, -2, -4, -5, -6


def r4(w):
    return (w + 3) // 4 * 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from scaling_rgcn_training_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _lib():
    from scaling_rgcn_training_amd import _lib as L
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """A [rows, ld] float32 matrix inside an allocation of sentinel bits: g0 guard rows before it, g1 after it."""

    def __init__(self, rows, ld, dev, g0=G, g1=G):
        self.rows, self.ld, self.g0 = rows, ld, g0
        self.buf = torch.full((g0 + rows + g1, ld), SENT, dtype=torch.int32, device=dev)
        self.mat = self.buf.view(torch.float32)[g0:g0 + rows]
        self.snap = None

    @property
    def ptr(self):
        return self.mat.data_ptr()

    def fill(self, data):
        """input: data [rows, w] in columns [0, w), zeros up to round4(w) (the ABI's rule), sentinels beyond"""
        w = data.shape[1]
        self.mat[:, :w] = data.to(self.mat.device, torch.float32)
        self.mat[:, w:r4(w)] = 0.0
        self.snap = self.buf.clone()
        return self

    def unchanged(self, what):
        assert torch.equal(self.buf, self.snap), f"{what}: an input was written"

    def out(self, width, what, rows=None):
        """values of the written rows [0, rows) (or the rows of a bool mask), columns [0, width); asserts the footprint"""
        b = self.buf.clone()
        inner = b[self.g0:self.g0 + self.rows]
        sel = slice(0, self.rows if rows is None else rows) if rows is None or isinstance(rows, int) else \
            torch.as_tensor(rows, device=b.device)
        written = inner[sel, :r4(width)]
        pad = written[:, width:]
        assert bool((pad == 0).all()), f"{what}: pad columns [{width}, {r4(width)}) are not +0.0"
        vals = written[:, :width].view(torch.float32).double().cpu().numpy()
        inner[sel, :r4(width)] = SENT
        bad = (b != SENT).nonzero()
        assert bad.numel() == 0, (f"{what}: {bad.shape[0]} sentinel words overwritten, first at (row, col) "
                                  f"{(int(bad[0, 0]) - self.g0, int(bad[0, 1]))} of ld {self.ld} (rows before the matrix < 0)")
        return vals


class Flat:
    """n elements (float32 or int32) with `g` sentinel words on either side"""

    def __init__(self, n, dev, dtype=torch.float32, g=256):
        self.n, self.g = n, g
        self.buf = torch.full((g + max(n, 1) + g,), SENT, dtype=torch.int32, device=dev)
        self.t = self.buf[g:g + n].view(dtype)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def out(self, what):
        assert bool((self.buf[:self.g] == SENT).all()) and bool((self.buf[self.g + self.n:] == SENT).all()), \
            f"{what}: written outside its {self.n} elements"
        return self.t.clone()


class Workspace:
    """exactly `n` bytes, then WS_TAIL sentinel bytes"""

    def __init__(self, n, dev):
        self.n = n
        self.buf = torch.full((n + WS_TAIL,), 0xA5, dtype=torch.uint8, device=dev)
        self.ptr = self.buf.data_ptr()

    def check(self, what):
        assert bool((self.buf[self.n:] == 0xA5).all()), f"{what}: written past its queried {self.n} bytes"


# ---- one graph, its oracle per width pair, its plans per geometry: shared by every case of the module ------------------------
@functools.lru_cache(None)
def graph():
    ei, et = O.synthetic_graph(N, E, R, seed=77)
    et = et.clamp(max=R - 2)                  # dead last relation
    ei[:, 10:40] = ei[:, 50:80]               # duplicate triples
    et[10:40] = et[50:80]
    ei[1, 100:180] = 5                        # a hub inside one relation: repeated destinations in one row tile
    et[100:180] = 1
    ei[1, 200] = ei[0, 200]                   # a self loop
    return ei, et


@functools.lru_cache(None)
def oracle(din, dout):
    ei, et = graph()
    w, root, _ = O.synthetic_params(R, din, dout, seed=din * 7 + dout)
    g = torch.Generator().manual_seed(din * 131 + dout)
    bias = torch.randn(dout, generator=g) * 0.1
    x = torch.randn(N, din, generator=g)
    dg = torch.randn(N, dout, generator=g)
    a = [t.numpy() for t in (x, ei, et, w, root, bias, dg)]
    ref, gr = O.rgcn_conv_segments(*a)
    c_out, c = abs_condition(*a)
    o32, g32 = cpu32_reference(*a)
    return dict(x=x, dg=dg, w=w, root=root, bias=bias, ref=ref, gr=gr, c_out=c_out, c=c, o32=o32, g32=g32)


@functools.lru_cache(None)
def plans(tile, chunk, layout, dev_index=0):
    from scaling_rgcn_training_amd import plan as P
    ei, et = graph()
    d = torch.device("cuda", dev_index)
    return P.build_graph_plans_device(ei.to(d), et.to(d), N, R, tile, chunk=chunk, split=layout)


@functools.lru_cache(None)
def packed(din, dout, transpose):
    o = oracle(din, dout)
    d = torch.device("cuda:0")
    return _lib().pack_weights(o["w"].to(d), o["root"].to(d), transpose)


def _act(z, act, f=np):
    if act == 1:
        return f.maximum(z, 0)
    if act == 2:
        return 1 / (1 + f.exp(-z))
    return z


def call_fwd(ps, din, dout, ldx, ldo, act=0, flags=0, dev=None):
    """rgcn_fwd on guarded operands -> (status, out Guarded, x Guarded)"""
    L = _lib()
    o = oracle(din, dout)
    x = Guarded(N, ldx, dev).fill(o["x"])
    out = Guarded(ps.n_owned, ldo, dev, g1=G_OUT)
    bias = Flat(dout, dev)
    bias.t.copy_(o["bias"])
    st = L.load().rgcn_fwd(C.byref(ps), x.ptr, ldx, din, packed(din, dout, False).data_ptr(), bias.ptr, out.ptr, ldo, dout, act,
                           flags, _stream())
    torch.cuda.synchronize()
    x.unchanged("rgcn_fwd x")
    bias.out("rgcn_fwd bias")
    return st, out


def check_fwd(out, din, dout, act, tag, rows=slice(None)):
    o = oracle(din, dout)
    got = out.out(dout, "rgcn_fwd " + tag)
    assert_close(got, _act(o["ref"][rows], act), o["c_out"][rows], f"abi out {tag}", cpu32=_act(o["o32"][rows].astype(np.float32), act))


def call_dx(ps, din, dout, ldg, lddx, relu_ld=None, flags=0, dev=None):
    L = _lib()
    o = oracle(din, dout)
    g = Guarded(N, ldg, dev).fill(o["dg"])
    dx = Guarded(ps.n_owned, lddx, dev, g1=G_OUT)
    rel = None
    if relu_ld is not None:
        rel = Guarded(ps.n_owned, relu_ld, dev).fill(o["x"][:ps.n_owned])
    st = L.load().rgcn_bwd_dx(C.byref(ps), g.ptr, ldg, dout, packed(din, dout, True).data_ptr(), dx.ptr, lddx, din,
                              None if rel is None else rel.ptr, 0 if rel is None else relu_ld, flags, _stream())
    torch.cuda.synchronize()
    g.unchanged("rgcn_bwd_dx g")
    if rel is not None:
        rel.unchanged("rgcn_bwd_dx relu_of")
    return st, dx


def check_dx(dx, din, dout, tag, masked=False, rows=slice(None)):
    o = oracle(din, dout)
    ref, cond, c32 = o["gr"]["x"][rows], o["c"]["x"][rows], o["g32"]["x"][rows]
    if masked:
        m = (o["x"].numpy()[rows] > 0)
        ref, cond, c32 = ref * m, cond * m, c32 * m
    assert_close(dx.out(din, "rgcn_bwd_dx " + tag), ref, cond, f"abi d_x {tag}", cpu32=c32)


def _strides(w):
    """the three row strides of a width: round4, round4 + 4, padded_width + 4"""
    return [r4(w), r4(w) + 4, _lib().padded_width(w) + 4]


def _pair(win, wout, k):
    """(ld_in, ld_out) of stride variant k, different from each other"""
    a, b = _strides(win)[k], _strides(wout)[(k + 1) % 3]
    return (a, b) if a != b else (a, b + 4)


WIDTHS = [(63, 16), (33, 7), (64, 64), (128, 100), (1, 5)]


# ---- A. strides and footprints of rgcn_fwd / rgcn_bwd_dx ---------------------------------------------------------------------
@pytest.mark.parametrize("k", range(3), ids=["round4", "round4+4", "padded+4"])
@pytest.mark.parametrize("din,dout", WIDTHS)
def test_exact_fp32_forward_and_dx_strides(dev, din, dout, k):
    """the exact-fp32 kernels (narrow: gathered width 16 / 32, wide: 64 / 128) at every stride class, input stride != output's"""
    p = plans(64, 64, 0)
    ldx, ldo = _pair(din, dout, k)
    st, out = call_fwd(_lib().plan_struct(p.fwd), din, dout, ldx, ldo, dev=dev)
    assert st == OK
    check_fwd(out, din, dout, 0, f"[{din}->{dout} ldx {ldx} ldo {ldo}]")
    ldg, lddx = _pair(dout, din, k)
    st, dx = call_dx(_lib().plan_struct(p.bwd), din, dout, ldg, lddx, dev=dev)
    assert st == OK
    check_dx(dx, din, dout, f"[{din}->{dout} ldg {ldg} lddx {lddx}]")


@pytest.mark.parametrize("act", [0, 1, 2], ids=["none", "relu", "sigmoid"])
def test_forward_activations(dev, act):
    p = plans(64, 64, 0)
    st, out = call_fwd(_lib().plan_struct(p.fwd), 63, 16, 68, 24, act=act, dev=dev)
    assert st == OK
    check_fwd(out, 63, 16, act, f"[act {act}]")


@pytest.mark.parametrize("din,dout", [(33, 7), (63, 16), (64, 64)])
def test_dx_relu_of_with_its_own_stride(dev, din, dout):
    p = plans(64, 64, 0)
    ldg, lddx, ldr = r4(dout) + 4, r4(din), _lib().padded_width(din) + 4
    st, dx = call_dx(_lib().plan_struct(p.bwd), din, dout, ldg, lddx, relu_ld=ldr, dev=dev)
    assert st == OK
    check_dx(dx, din, dout, f"[relu_of ldr {ldr}]", masked=True)


@pytest.mark.parametrize("din,dout", [(63, 16), (128, 100), (64, 64)])
def test_pointer_gather_reads_no_padding_row(dev, din, dout):
    """RGCN_FLAG_POINTER_GATHER: padding slots gather row n_nodes with a real 64-bit load unless the kernel skips it; that row is a
    NaN sentinel here"""
    L = _lib()
    p = plans(64, 64, 0)
    ldx, ldo = _pair(din, dout, 2)
    st, out = call_fwd(L.plan_struct(p.fwd), din, dout, ldx, ldo, flags=L.FLAG_POINTER_GATHER, dev=dev)
    assert st == OK
    check_fwd(out, din, dout, 0, "[pointer gather]")
    ldg, lddx = _pair(dout, din, 2)
    st, dx = call_dx(L.plan_struct(p.bwd), din, dout, ldg, lddx, flags=L.FLAG_POINTER_GATHER, dev=dev)
    assert st == OK
    check_dx(dx, din, dout, "[pointer gather]")


@pytest.mark.parametrize("layout,chunk", [(0, 128), (0, 112), (3, 128), (3, 112)])
def test_split_producers_strides(dev, layout, chunk):
    """the bf16 x 3 producer-split kernel (64 x 64, 128-slot chunks; 48 / 42 KiB ring slots) on layout-0 and layout-3 plans"""
    L = _lib()
    p = plans(128, chunk, layout)
    st, out = call_fwd(L.plan_struct(p.fwd), 64, 64, 68, 64, flags=L.FLAG_SPLIT_PRODUCERS, dev=dev)
    assert st == OK
    check_fwd(out, 64, 64, 0, f"[split layout {layout} chunk {chunk}]")
    st, dx = call_dx(L.plan_struct(p.bwd), 64, 64, 64, 68, relu_ld=72, flags=L.FLAG_SPLIT_PRODUCERS, dev=dev)
    assert st == OK
    check_dx(dx, 64, 64, f"[split layout {layout} chunk {chunk}]", masked=True)


# ---- rgcn_bwd_dw, rgcn_bwd_dw_tiles, rgcn_bwd_dw_root -------------------------------------------------------------------------
def call_dw(ps, din, dout, ldx, ldg, flags, want=(True, True, True), dev=None, ws_bytes=None):
    L = _lib()
    lib = L.load()
    o = oracle(din, dout)
    x = Guarded(N, ldx, dev).fill(o["x"])
    g = Guarded(ps.n_owned, ldg, dev).fill(o["dg"][:ps.n_owned])
    outs = [Flat(n, dev) if w else None for n, w in zip((R * din * dout, din * dout, dout), want)]
    need = lib.rgcn_bwd_dw_workspace_bytes(C.byref(ps), din, dout)
    ws = Workspace(need, dev)
    st = lib.rgcn_bwd_dw(C.byref(ps), x.ptr, ldx, din, g.ptr, ldg, dout, ws.ptr, need if ws_bytes is None else ws_bytes,
                         *[None if f is None else f.ptr for f in outs], flags, _stream())
    torch.cuda.synchronize()
    x.unchanged("rgcn_bwd_dw x")
    g.unchanged("rgcn_bwd_dw g")
    ws.check("rgcn_bwd_dw workspace")
    return st, outs, need


def check_dw(outs, din, dout, tag, names=("weight", "root", "bias")):
    o = oracle(din, dout)
    for f, nm in zip(outs, names):
        if f is None:
            continue
        shape = {"weight": (R, din, dout), "root": (din, dout), "bias": (dout,)}[nm]
        got = f.out(f"d_{nm} {tag}").view(shape).double().cpu().numpy()
        assert_close(got, o["gr"][nm], o["c"][nm], f"abi d_{nm} {tag}", cpu32=o["g32"][nm])


@pytest.mark.parametrize("mode,din,dout", [("ring", 63, 16), ("ring", 128, 100), ("ring", 1, 5), ("direct", 64, 64),
                                           ("root_only", 64, 64), ("null_weight", 33, 7), ("null_root", 33, 7),
                                           ("null_bias", 64, 64)])
def test_bwd_dw_outputs_and_workspace(dev, mode, din, dout):
    L = _lib()
    flags = {"ring": L.FLAG_DW_RING, "direct": L.FLAG_DW_DIRECT, "root_only": L.FLAG_DW_ROOT_ONLY}.get(mode, 0)
    want = {"root_only": (False, True, True), "null_weight": (False, True, True), "null_root": (True, False, True),
            "null_bias": (True, True, False)}.get(mode, (True, True, True))
    ps = L.plan_struct(plans(64, 64, 0).fwd)
    ldx, ldg = _pair(din, dout, 2)
    st, outs, need = call_dw(ps, din, dout, ldx, ldg, flags, want, dev=dev)
    assert st == OK
    check_dw(outs, din, dout, f"[{mode} {din}->{dout}]")
    st, outs, _ = call_dw(ps, din, dout, ldx, ldg, flags, want, dev=dev, ws_bytes=need - 1)
    assert st == ERR_WORKSPACE
    for f in outs:
        if f is not None:
            assert bool((f.buf == SENT).all()), "a refused call wrote its output"


@pytest.mark.parametrize("split", [False, True], ids=["exact", "bf16x3"])
@pytest.mark.parametrize("layout", [0, 5])
def test_bwd_dw_tiles_guarded(dev, layout, split):
    L = _lib()
    lib = L.load()
    from scaling_rgcn_training_amd import plan as P
    t_dw, walkers, _ = L.dw_tiles_geometry()
    pl = plans(t_dw, 64, layout).fwd
    ps = L.plan_struct(pl)
    walk = Flat(R * (walkers + 1), dev, torch.int32)
    assert lib.rgcn_dw_tiles_walk(C.byref(ps), walk.ptr, _stream()) == OK
    torch.cuda.synchronize()
    assert torch.equal(walk.out("walk_ptr").view(R, walkers + 1), P.dw_walk_table(pl, walkers))
    din = dout = 64
    o = oracle(din, dout)
    x = Guarded(N, 68, dev).fill(o["x"])
    g = Guarded(N, 64, dev).fill(o["dg"])
    dw = Flat(R * din * dout, dev)
    need = lib.rgcn_bwd_dw_tiles_workspace_bytes(R)
    ws = Workspace(need, dev)
    fl = L.FLAG_SPLIT_PRODUCERS if split else 0
    assert lib.rgcn_bwd_dw_tiles(C.byref(ps), walk.ptr, x.ptr, 68, din, g.ptr, 64, dout, ws.ptr, need - 1, dw.ptr, fl,
                                 _stream()) == ERR_WORKSPACE
    st = lib.rgcn_bwd_dw_tiles(C.byref(ps), walk.ptr, x.ptr, 68, din, g.ptr, 64, dout, ws.ptr, need, dw.ptr, fl, _stream())
    torch.cuda.synchronize()
    assert st == OK
    x.unchanged("dw_tiles x")
    g.unchanged("dw_tiles g")
    ws.check("dw_tiles workspace")
    walk.out("walk_ptr after rgcn_bwd_dw_tiles")
    check_dw([dw], din, dout, f"[tile-major layout {layout} split {split}]", names=("weight",))


@pytest.mark.parametrize("din,dout", [(63, 16), (33, 7), (1, 5), (64, 64)])
def test_bwd_dw_root_guarded(dev, din, dout):
    lib = _lib().load()
    o = oracle(din, dout)
    ldx, ldg = _pair(din, dout, 2)
    x = Guarded(N, ldx, dev).fill(o["x"])
    g = Guarded(N, ldg, dev).fill(o["dg"])
    dr, db = Flat(din * dout, dev), Flat(dout, dev)
    need = lib.rgcn_bwd_dw_root_workspace_bytes()
    ws = Workspace(need, dev)
    assert lib.rgcn_bwd_dw_root(x.ptr, ldx, din, g.ptr, ldg, dout, N, ws.ptr, need - 1, dr.ptr, db.ptr, _stream()) == ERR_WORKSPACE
    assert lib.rgcn_bwd_dw_root(x.ptr, ldx, din, g.ptr, ldg, dout, N, ws.ptr, need, dr.ptr, db.ptr, _stream()) == OK
    torch.cuda.synchronize()
    x.unchanged("dw_root x")
    g.unchanged("dw_root g")
    ws.check("dw_root workspace")
    x64, g64 = o["x"].double().numpy(), o["dg"].double().numpy()
    assert_close(dr.out("d_root").view(din, dout).double().cpu().numpy(), x64.T @ g64, np.abs(x64).T @ np.abs(g64), "abi dw_root d_root",
                 cpu32=(o["x"].t() @ o["dg"]).numpy())
    assert_close(db.out("d_bias").double().cpu().numpy(), g64.sum(0), np.abs(g64).sum(0), "abi dw_root d_bias",
                 cpu32=o["dg"].sum(0).numpy())


# ---- elementwise, edge-parallel, packing, decompositions ----------------------------------------------------------------------
@pytest.mark.parametrize("alias", [False, True], ids=["dz", "dz=da"])
@pytest.mark.parametrize("act", [1, 2], ids=["relu", "sigmoid"])
def test_act_backward_guarded(dev, act, alias):
    lib = _lib().load()
    rows, w, ld = 333, 33, 36          # (the entry point's operands are whole [rows, ld] matrices)
    gen = torch.Generator().manual_seed(act)
    z = torch.randn(rows, w, generator=gen)
    a_val = torch.relu(z) if act == 1 else torch.sigmoid(z)
    da_val = torch.randn(rows, w, generator=gen)
    a = Guarded(rows, ld, dev).fill(a_val)
    da = Guarded(rows, ld, dev).fill(da_val)
    dz = da if alias else Guarded(rows, ld, dev)
    assert lib.rgcn_act_backward(a.ptr, da.ptr, dz.ptr, rows, ld, act, _stream()) == OK
    torch.cuda.synchronize()
    a.unchanged("act_backward a")
    if not alias:
        da.unchanged("act_backward da")
    a64, d64 = a_val.double().numpy(), da_val.double().numpy()
    ref = d64 * (a64 > 0) if act == 1 else d64 * a64 * (1 - a64)
    got = dz.out(w, "act_backward dz")
    assert_close(got, ref, np.abs(ref), f"abi act_backward [{act} alias {alias}]")


@functools.lru_cache(None)
def ep_units():
    """a layout-2 plan (relation-major 64-slot units) by the builder, and its arrays on the host"""
    p = plans(64, 64, 2)
    pl = p.fwd
    host = {k: getattr(pl, k).cpu().numpy() for k in ("chunk_rel", "chunk_cnt", "slot_src", "slot_w", "slot_row")}
    return pl, host


@pytest.mark.parametrize("din,dout,split", [(33, 7, False), (63, 16, False), (128, 100, False), (64, 64, True)])
def test_ep_transform_footprint(dev, din, dout, split):
    """z rows of used row tiles: w * x[src] @ W_rel; rows of unused row tiles untouched; columns past round4(dout) untouched"""
    L = _lib()
    lib = L.load()
    pl, h = ep_units()
    o = oracle(din, dout)
    nu = pl.n_chunks
    units = L.RgcnEdgeUnits(N, nu, R, 0, pl.chunk_rel.data_ptr(), pl.chunk_cnt.data_ptr(), pl.slot_src.data_ptr(), pl.slot_w.data_ptr())
    ldx, ldz = _pair(din, dout, 2)
    x = Guarded(N, ldx, dev).fill(o["x"])
    z = Guarded(nu * 64, ldz, dev, g1=G_OUT)
    st = lib.rgcn_ep_transform(C.byref(units), x.ptr, ldx, din, packed(din, dout, False).data_ptr(), z.ptr, ldz, dout,
                               L.FLAG_SPLIT_PRODUCERS if split else 0, _stream())
    torch.cuda.synchronize()
    assert st == OK
    x.unchanged("ep_transform x")
    slot = np.arange(nu * 64)
    used = (slot % 64) < h["chunk_cnt"][slot // 64]
    got = z.out(dout, "ep_transform z", rows=used)
    rel = h["chunk_rel"][slot // 64][used]
    src = h["slot_src"][used]
    w = h["slot_w"][used].astype(np.float64)
    xe = np.vstack([o["x"].double().numpy(), np.zeros((1, din))])
    wf = np.concatenate([o["w"].double().numpy(), o["root"].double().numpy()[None]], 0)
    ref = np.zeros((len(src), dout))
    cond = np.zeros((len(src), dout))
    for r in range(R + 1):
        m = rel == r
        ref[m] = (xe[src[m]] * w[m, None]) @ wf[r]
        cond[m] = (np.abs(xe[src[m]]) * np.abs(w[m, None])) @ np.abs(wf[r])
    assert_close(got, ref, cond, f"abi ep_transform [{din}->{dout} split {split}]")


def test_ep_segment_sum_multilevel(dev):
    """two levels: weighted, indexed pieces of at most 256 rows (final_level 0), then the pieces of every segment with bias,
    ReLU and a mask (final_level 1); ldin != ldm != ldo at every level"""
    lib = _lib().load()
    w = 33
    gen = torch.Generator().manual_seed(5)
    n_in, n_out = 3000, 40
    lens = torch.randint(0, 700, (n_out,), generator=gen)
    lens[3] = 0
    lens[7] = 1
    idx = torch.randint(0, n_in, (int(lens.sum()),), generator=gen, dtype=torch.int64)
    sw = torch.randn(idx.shape[0], generator=gen)
    src = torch.randn(n_in, w, generator=gen)
    bias = torch.randn(w, generator=gen)
    mask_v = torch.randn(n_out, w, generator=gen)
    # level 1: pieces of <= 256 rows of every segment
    starts = np.concatenate([[0], np.cumsum(lens.numpy())])
    p1, seg_of_piece = [0], []
    for s in range(n_out):
        for a in range(starts[s], starts[s + 1], 256):
            p1.append(min(a + 256, starts[s + 1]))
            seg_of_piece.append(s)
    n_pc = len(p1) - 1
    p2 = np.searchsorted(np.array(seg_of_piece), np.arange(n_out + 1), side="left").astype(np.int32)
    ins = Guarded(n_in, r4(w) + 4, dev).fill(src)
    i32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int32, device=dev)
    ptr1, ptr2, idx1, w1 = i32(p1), i32(p2), i32(idx.numpy()), sw.to(dev)
    mid = Guarded(n_pc, _lib().padded_width(w) + 4, dev, g1=G_OUT)
    assert lib.rgcn_ep_segment_sum(ins.ptr, ins.ld, ptr1.data_ptr(), idx1.data_ptr(), w1.data_ptr(), n_pc, w, None, 0, None, 0, 0,
                                   mid.ptr, mid.ld, _stream()) == OK
    torch.cuda.synchronize()
    ins.unchanged("segment_sum in")
    s64, w64 = src.double().numpy(), sw.double().numpy()
    terms = s64[idx.numpy()] * w64[:, None]
    ref1 = np.stack([terms[p1[i]:p1[i + 1]].sum(0) for i in range(n_pc)])
    c1 = np.stack([np.abs(terms[p1[i]:p1[i + 1]]).sum(0) for i in range(n_pc)])
    assert_close(mid.out(w, "segment_sum level 1"), ref1, c1, "abi segment_sum level 1")
    mid.snap = mid.buf.clone()
    mask = Guarded(n_out, r4(w), dev).fill(mask_v)
    out = Guarded(n_out, r4(w) + 8, dev, g1=G_OUT)
    bd = bias.to(dev)
    assert lib.rgcn_ep_segment_sum(mid.ptr, mid.ld, ptr2.data_ptr(), None, None, n_out, w, bd.data_ptr(), 1, mask.ptr, mask.ld, 1,
                                   out.ptr, out.ld, _stream()) == OK
    torch.cuda.synchronize()
    mid.unchanged("segment_sum level-2 input")
    mask.unchanged("segment_sum mask")
    z = np.stack([terms[starts[s]:starts[s + 1]].sum(0) for s in range(n_out)]) + bias.double().numpy()
    cz = np.stack([np.abs(terms[starts[s]:starts[s + 1]]).sum(0) for s in range(n_out)]) + np.abs(bias.double().numpy())
    m = mask_v.numpy() > 0
    assert_close(out.out(w, "segment_sum level 2"), np.maximum(z, 0) * m, cz * m, "abi segment_sum level 2")


def test_eplan_segments_guarded(dev):
    lib = _lib().load()
    pl, h = ep_units()
    n_slots = int(pl.slot_row.numel())
    seg_ptr, seg_idx = Flat(N + 1, dev, torch.int32), Flat(n_slots, dev, torch.int32)
    need = lib.rgcn_plan_workspace_bytes(n_slots, 0, 1, 16)
    ws = Workspace(need, dev)
    assert lib.rgcn_eplan_segments(pl.slot_row.data_ptr(), n_slots, N, ws.ptr, need - 1, seg_ptr.ptr, seg_idx.ptr, _stream()) == ERR_WORKSPACE
    assert lib.rgcn_eplan_segments(pl.slot_row.data_ptr(), n_slots, N, ws.ptr, need, seg_ptr.ptr, seg_idx.ptr, _stream()) == OK
    torch.cuda.synchronize()
    ws.check("eplan_segments workspace")
    rows = h["slot_row"]
    real = np.nonzero(rows < N)[0]
    order = real[np.argsort(rows[real], kind="stable")]
    ptr = seg_ptr.out("seg_ptr").cpu().numpy()
    idx = seg_idx.out("seg_idx").cpu().numpy()
    assert np.array_equal(ptr, np.searchsorted(rows[order], np.arange(N + 1), side="left"))
    assert np.array_equal(idx[:ptr[N]], order)


@pytest.mark.parametrize("din,dout", [(63, 16), (64, 64)])
def test_pack_weights_guarded(dev, din, dout):
    """the three packers write exactly rgcn_packed_weight_floats floats, both orientations"""
    L = _lib()
    lib = L.load()
    o = oracle(din, dout)
    n = lib.rgcn_packed_weight_floats(R, din, dout)
    w, root = o["w"].to(dev), o["root"].to(dev)
    nb, nbases = 4 if din % 4 == 0 and dout % 4 == 0 else 1, 3
    gen = torch.Generator().manual_seed(din)
    bases = torch.randn(nbases, din, dout, generator=gen).to(dev)
    comp = torch.randn(R, nbases, generator=gen).to(dev)
    blocks = torch.randn(R, nb, din // nb, dout // nb, generator=gen).to(dev)
    for tr in (0, 1):
        f = Flat(n, dev)
        assert lib.rgcn_pack_weights(w.data_ptr(), root.data_ptr(), R, din, dout, tr, f.ptr, _stream()) == OK
        torch.cuda.synchronize()
        assert torch.equal(f.out("pack dense"), L.pack_weights(w, root, bool(tr)))
        f = Flat(n, dev)
        assert lib.rgcn_pack_weights_basis(bases.data_ptr(), comp.data_ptr(), root.data_ptr(), R, nbases, din, dout, tr, f.ptr, _stream()) == OK
        torch.cuda.synchronize()
        ref = L.pack_weights(torch.einsum("rb,bio->rio", comp.double(), bases.double()).float(), root, bool(tr))
        got = f.out("pack basis")
        nf = (R + 1) * L.padded_width(din) * L.padded_width(dout)     # the fp32 fragments (64 x 64: bf16 pieces follow, and a
        assert torch.allclose(got[:nf], ref[:nf], rtol=1e-5, atol=1e-5)   # last-bit difference may move a piece boundary)
        f = Flat(n, dev)
        assert lib.rgcn_pack_weights_block(blocks.data_ptr(), root.data_ptr(), R, nb, din, dout, tr, f.ptr, _stream()) == OK
        torch.cuda.synchronize()
        dense = torch.zeros(R, din, dout, device=dev)
        for b in range(nb):
            dense[:, b * (din // nb):(b + 1) * (din // nb), b * (dout // nb):(b + 1) * (dout // nb)] = blocks[:, b]
        assert torch.equal(f.out("pack block"), L.pack_weights(dense, root, bool(tr)))


def test_basis_and_block_backward_guarded(dev):
    lib = _lib().load()
    din, dout, nbases, nb = 64, 64, 3, 4
    gen = torch.Generator().manual_seed(9)
    dw = torch.randn(R, din, dout, generator=gen)
    bases = torch.randn(nbases, din, dout, generator=gen)
    comp = torch.randn(R, nbases, generator=gen)
    d = [t.to(dev) for t in (dw, bases, comp)]
    db, dc = Flat(nbases * din * dout, dev), Flat(R * nbases, dev)
    assert lib.rgcn_basis_backward(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), R, nbases, din, dout, db.ptr, dc.ptr, _stream()) == OK
    dblk = Flat(R * din * dout // nb, dev)
    assert lib.rgcn_block_backward(d[0].data_ptr(), R, nb, din, dout, dblk.ptr, _stream()) == OK
    torch.cuda.synchronize()
    w64, b64, c64 = dw.double().numpy(), bases.double().numpy(), comp.double().numpy()
    assert_close(db.out("d_bases").view(nbases, din, dout).double().cpu().numpy(), np.einsum("rb,rio->bio", c64, w64),
                 np.einsum("rb,rio->bio", np.abs(c64), np.abs(w64)), "abi d_bases")
    assert_close(dc.out("d_comp").view(R, nbases).double().cpu().numpy(), np.einsum("rio,bio->rb", w64, b64),
                 np.einsum("rio,bio->rb", np.abs(w64), np.abs(b64)), "abi d_comp")
    k, m = din // nb, dout // nb
    ref = np.stack([np.stack([w64[r, b * k:(b + 1) * k, b * m:(b + 1) * m] for b in range(nb)]) for r in range(R)])
    assert np.array_equal(dblk.out("d_blocks").view(R, nb, k, m).double().cpu().numpy(), ref)


# ---- the plan builder: every array with a trailing guard, workspaces of exactly the queried size --------------------------------
@pytest.mark.parametrize("tile,chunk,layout", [(64, 64, 0), (128, 112, 3), (320, 64, 5), (64, 64, 2)])
def test_plan_builder_guarded(dev, tile, chunk, layout):
    L = _lib()
    lib = L.load()
    ei, et = graph()
    eid, etd = ei.to(dev), et.to(dev)
    gs, keep = L.graph_struct(eid, etd, N, R)
    need = lib.rgcn_plan_workspace_bytes(E, N, R, (N + 15) // 16 * 16 if layout == 2 else tile)   # (layout 2: one tile)
    ws = Workspace(need, dev)
    w = Flat(E, dev)
    assert lib.rgcn_edge_weights(C.byref(gs), 0, w.ptr, ws.ptr, need, _stream()) == OK
    torch.cuda.synchronize()
    ws.check("edge_weights workspace")
    ref_ws = L.plan_workspace(E, N, R, tile, dev)
    w_ref = L.edge_weights(gs, "mean", ref_ws)
    assert torch.equal(w.out("edge weights"), w_ref)
    sizes = L.RgcnPlanSizes()
    assert lib.rgcn_plan_build_begin(C.byref(gs), w.ptr, 0, 0, N, tile, chunk, layout, ws.ptr, need - 1, C.byref(sizes),
                                     _stream()) == ERR_WORKSPACE
    assert lib.rgcn_plan_build_begin(C.byref(gs), w.ptr, 0, 0, N, tile, chunk, layout, ws.ptr, need, C.byref(sizes), _stream()) == OK
    i32 = torch.int32
    arr = {"tile_ptr": Flat(sizes.n_tiles + 1, dev, i32), "chunk_rel": Flat(sizes.n_chunks, dev, i32),
           "chunk_cnt": Flat(sizes.n_chunks, dev, i32), "chunk_tile": Flat(sizes.n_chunks, dev, i32),
           "chunk_flags": Flat(sizes.n_chunks, dev, i32), "rel_order": Flat(sizes.n_units, dev, i32),
           "slot_src": Flat(sizes.n_slots, dev, i32), "slot_w": Flat(sizes.n_slots, dev),
           "slot_row": Flat(sizes.n_slots, dev, i32), "slot_acc": Flat(sizes.n_slots, dev, i32)}
    if layout == 5:
        arr["slot_src2"] = Flat(sizes.n_chunks * 8, dev, i32)
    ps = L.RgcnPlanStruct()
    for k, f in arr.items():
        setattr(ps, k, f.ptr)
    assert lib.rgcn_plan_build_finish(C.byref(sizes), ws.ptr, need, C.byref(ps), _stream()) == OK
    torch.cuda.synchronize()
    ws.check("plan build workspace")
    ps_ref, a_ref, _ = L.plan_build(gs, w_ref, False, 0, N, tile, chunk, ref_ws, layout)
    torch.cuda.synchronize()
    assert (ps.n_units, ps.chunk_rows, ps.layout) == (ps_ref.n_units, ps_ref.chunk_rows, ps_ref.layout)
    for k, f in arr.items():
        got = f.out(f"plan array {k}")
        n = ps.n_units if k == "rel_order" else got.numel()     # (layout 5: fewer units than _begin sized rel_order for)
        assert torch.equal(got[:n], a_ref[k][:n]), k
    del keep


# ---- partitioned plans: adjacent row slices of one shared buffer -----------------------------------------------------------------
@pytest.mark.parametrize("direction", ["fwd", "dx"])
def test_partitioned_plans_write_only_their_rows(dev, direction):
    """three owned ranges [0, 192), [192, 448), [448, 700) (tile 64: the last is not whole tiles), each plan's output into its
    row slice of ONE sentinel-filled [N, ld] buffer as conv._gather_pieces lays ranks out; the ranges not yet written must
    still hold the sentinel when the next one is launched"""
    from scaling_rgcn_training_amd import plan as P
    L = _lib()
    lib = L.load()
    ei, et = graph()
    din, dout = 63, 16
    o = oracle(din, dout)
    cuts = [0, 192, 448, N]
    ranges = [((a, b), (a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
    gps = P.build_graph_plans_device(ei.to(dev), et.to(dev), N, R, 64, chunk=64, ranges=ranges)
    wout = dout if direction == "fwd" else din
    ld = r4(wout) + 4
    full = Guarded(N, ld, dev, g1=G_OUT)
    x = Guarded(N, 68, dev).fill(o["x"]) if direction == "fwd" else Guarded(N, r4(dout) + 4, dev).fill(o["dg"])
    before = full.buf.clone()
    for i, ((a, b), _) in enumerate(ranges):
        rows_after = full.buf[G + a:]
        assert bool((rows_after == SENT).all()), f"range {i}: rows past {a} were written before their launch"
        assert torch.equal(full.buf[:G + a], before[:G + a])
        if direction == "fwd":
            ps = L.plan_struct(gps[i].fwd)
            st = lib.rgcn_fwd(C.byref(ps), x.ptr, x.ld, din, packed(din, dout, False).data_ptr(), None, full.mat[a].data_ptr(), ld,
                              dout, 0, 0, _stream())
        else:
            ps = L.plan_struct(gps[i].bwd)
            st = lib.rgcn_bwd_dx(C.byref(ps), x.ptr, x.ld, dout, packed(din, dout, True).data_ptr(), full.mat[a].data_ptr(), ld,
                                 din, None, 0, 0, _stream())
        torch.cuda.synchronize()
        assert st == OK and ps.n_owned == b - a
        before = full.buf.clone()
        assert bool((full.buf[G + b:] == SENT).all()), f"range {i} [{a}, {b}) wrote rows past {b}"
    x.unchanged("partitioned input")
    got = full.out(wout, f"partitioned {direction}")
    if direction == "fwd":
        ref = o["ref"] - o["bias"].double().numpy()        # (no bias passed)
        assert_close(got, ref, o["c_out"], "abi partitioned out", cpu32=o["o32"] - o["bias"].numpy())
    else:
        assert_close(got, o["gr"]["x"], o["c"]["x"], "abi partitioned d_x", cpu32=o["g32"]["x"])


# ---- layout x entry point ---------------------------------------------------------------------------------------------------------
# Plans of every layout the builder makes (64 x 64 layer, tile 128 unless the tile-major d_weight geometry needs 320), every flag
# that selects a kernel.  Each entry: the status the entry point answers; OK results are checked against the oracle.
#   fwd / dx flags:  0, SPLIT_PRODUCERS, EXACT_FP32, POINTER_GATHER
#   bwd_dw flags:    0, DW_RING, DW_DIRECT, DW_ROOT_ONLY
#   dw_tiles flags:  0, SPLIT_PRODUCERS
_P = ERR_PLAN
LAYOUT_TABLE = {
    # (layout, chunk, tile):   fwd              bwd_dx            bwd_dw             dw_tiles
    (0, 64, 128):  ((OK, OK, OK, OK), (OK, OK, OK, OK), (OK, OK, OK, OK), (_P, _P)),
    (0, 128, 128): ((OK, OK, OK, OK), (OK, OK, OK, OK), (OK, OK, OK, OK), (_P, _P)),
    (0, 112, 128): ((OK, OK, OK, OK), (OK, OK, OK, OK), (OK, OK, OK, OK), (_P, _P)),
    (1, 128, 128): ((OK, OK, OK, OK), (OK, OK, OK, OK), (OK, OK, OK, OK), (_P, _P)),
    (2, 64, 128):  ((_P, _P, _P, _P), (_P, _P, _P, _P), (OK, OK, OK, _P), (_P, _P)),
    (3, 128, 128): ((OK, OK, OK, _P), (OK, OK, OK, _P), (_P, _P, _P, _P), (_P, _P)),
    (3, 112, 128): ((OK, OK, OK, _P), (OK, OK, OK, _P), (_P, _P, _P, _P), (_P, _P)),
    (0, 64, 320):  ((OK, OK, OK, OK), (OK, OK, OK, OK), (OK, OK, OK, OK), (OK, OK)),
    (5, 64, 320):  ((_P, _P, _P, _P), (_P, _P, _P, _P), (_P, _P, _P, _P), (OK, OK)),
}


@pytest.mark.parametrize("key", list(LAYOUT_TABLE), ids=lambda k: "layout%d-chunk%d-tile%d" % k)
def test_layout_entry_point_table(dev, key):
    L = _lib()
    lib = L.load()
    from scaling_rgcn_training_amd import plan as P
    layout, chunk, tile = key
    p = plans(tile, chunk, layout)
    pf, pb = L.plan_struct(p.fwd), L.plan_struct(p.bwd)
    assert (pf.layout, pf.chunk_rows) == (layout, chunk)
    want = LAYOUT_TABLE[key]
    got = ([], [], [], [])
    for fl in (0, L.FLAG_SPLIT_PRODUCERS, L.FLAG_EXACT_FP32, L.FLAG_POINTER_GATHER):
        st, out = call_fwd(pf, 64, 64, 68, 64, flags=fl, dev=dev)
        got[0].append(st)
        if st == OK:
            check_fwd(out, 64, 64, 0, f"[table {key} flags {fl}]")
        else:
            assert bool((out.buf == SENT).all()), "a refused rgcn_fwd wrote its output"
        st, dx = call_dx(pb, 64, 64, 64, 68, flags=fl, dev=dev)
        got[1].append(st)
        if st == OK:
            check_dx(dx, 64, 64, f"[table {key} flags {fl}]")
    for fl in (0, L.FLAG_DW_RING, L.FLAG_DW_DIRECT, L.FLAG_DW_ROOT_ONLY):
        want_out = (False, True, True) if fl == L.FLAG_DW_ROOT_ONLY else (True, True, True)
        st, outs, _ = call_dw(pf, 64, 64, 68, 64, fl, want_out, dev=dev)
        got[2].append(st)
        if st == OK:
            check_dw(outs, 64, 64, f"[table {key} flags {fl}]")
    t_dw, walkers, _ = L.dw_tiles_geometry()
    walk = torch.zeros(R, walkers + 1, dtype=torch.int32, device=dev)
    if tile == t_dw:
        walk = P.dw_walk_table(p.fwd, walkers)
    for fl in (0, L.FLAG_SPLIT_PRODUCERS):
        o = oracle(64, 64)
        x = Guarded(N, 68, dev).fill(o["x"])
        g = Guarded(N, 64, dev).fill(o["dg"])
        dw = Flat(R * 64 * 64, dev)
        need = lib.rgcn_bwd_dw_tiles_workspace_bytes(R)
        ws = Workspace(need, dev)
        st = lib.rgcn_bwd_dw_tiles(C.byref(pf), walk.data_ptr(), x.ptr, 68, 64, g.ptr, 64, 64, ws.ptr, need, dw.ptr, fl, _stream())
        torch.cuda.synchronize()
        got[3].append(st)
        if st == OK:
            check_dw([dw], 64, 64, f"[table {key} flags {fl}]", names=("weight",))
    assert tuple(tuple(g) for g in got) == want, (key, got)


# ---- C. capture into a hipGraph from a cold process -------------------------------------------------------------------------------
_CHILD = r"""
import sys
import torch
sys.path.insert(0, sys.argv[1])
from oracle import rgcn_oracle as O
from scaling_rgcn_training_amd import _lib, plan as P
from scaling_rgcn_training_amd.conv import _rows16, _round4

dev = torch.device("cuda:0")
n, e, r = 3000, 40000, 6
ei, et = O.synthetic_graph(n, e, r, seed=3)
eid, etd = ei.to(dev), et.to(dev)
gen = torch.Generator().manual_seed(0)
layers = []
# 64 x 64 on the producer-split kernel + the tile-major d_weight kernel (its root / bias by the root-only walk), and 33 -> 7 on the
# exact-fp32 kernels + the relation-major ring kernels: every instantiation these calls pick sets its LDS attribute under capture
for din, dout, tile, chunk, flags, dwt in ((64, 64, 224, 128, _lib.FLAG_SPLIT_PRODUCERS, True), (33, 7, 64, 64, 0, False)):
    pl = P.build_graph_plans_device(eid, etd, n, r, tile, chunk=chunk, dw_tiles=dwt)
    layers.append(dict(din=din, dout=dout, flags=flags, plans=pl, x=_rows16(torch.randn(n, din, generator=gen).to(dev), din),
                       g=_rows16(torch.randn(n, dout, generator=gen).to(dev), dout), w=(0.2 * torch.randn(r, din, dout, generator=gen)).to(dev),
                       root=(0.2 * torch.randn(din, dout, generator=gen)).to(dev), b=torch.randn(dout, generator=gen).to(dev)))
torch.cuda.synchronize()


def alloc():
    return [dict(out=torch.zeros(n, _round4(L["dout"]), device=dev), dx=torch.zeros(n, _round4(L["din"]), device=dev),
                 dw=torch.zeros(r, L["din"], L["dout"], device=dev), dr=torch.zeros(L["din"], L["dout"], device=dev),
                 db=torch.zeros(L["dout"], device=dev)) for L in layers]


def step(outs):
    for L, o in zip(layers, outs):
        p, din, dout, fl = L["plans"], L["din"], L["dout"], L["flags"]
        pk, pkt = _lib.pack_weights(L["w"], L["root"], False), _lib.pack_weights(L["w"], L["root"], True)
        _lib.fwd(_lib.plan_struct(p.fwd), L["x"], din, pk, L["b"], o["out"], dout, _lib.ACT_RELU, fl)
        _lib.bwd_dx(_lib.plan_struct(p.bwd), L["g"], dout, pkt, o["dx"], din, L["x"], fl)
        if p.dw is not None:
            _lib.bwd_dw_tiles(_lib.plan_struct(p.dw), p.dw_walk, L["x"], din, L["g"], dout, o["dw"], fl)
            _lib.bwd_dw(_lib.plan_struct(p.fwd), L["x"], din, L["g"], dout, None, o["dr"], o["db"], _lib.FLAG_DW_ROOT_ONLY)
        else:
            _lib.bwd_dw(_lib.plan_struct(p.fwd), L["x"], din, L["g"], dout, o["dw"], o["dr"], o["db"], _lib.FLAG_DW_RING)


graph = torch.cuda.CUDAGraph()
captured = alloc()
with torch.cuda.graph(graph):
    step(captured)
graph.replay()
torch.cuda.synchronize()
eager = alloc()
step(eager)
torch.cuda.synchronize()
for i, (a, b) in enumerate(zip(captured, eager)):
    for k in a:
        assert bool(torch.isfinite(b[k]).all()) and bool(b[k].abs().sum() > 0), (i, k)
        assert torch.equal(a[k], b[k]), ("replay differs from eager", i, k)
print("cold capture ok")
"""


def test_capture_from_a_cold_process(dev):
    """A fresh process captures a whole layer step (forward, dX, dW) through torch.cuda.graph before any eager call of those entry
    points (the first launch of a kernel instantiation sets its LDS attribute), replays it and compares with an eager run."""
    res = subprocess.run([sys.executable, "-c", _CHILD, ROOT], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "cold capture ok" in res.stdout, (res.returncode, res.stdout[-2000:], res.stderr[-4000:])


# ---- featureless layers: rgcn_featureless_fwd / _bwd on guarded operands -----------------------------------------------------------
# Tables, comp, root, bias and x_index in sentinel buffers with row stride exactly `out` (a read past the last table row is a NaN),
# out / g at three strides, every backward output subset, the workspace at exactly its queried size.  Tile 128 x out 128: the
# forward's accumulator is 66,048 B of LDS (past 64 KiB), the basis backward with B = 1 131,840 B.
FL_IN_ROWS = 300          # rows of the tables under an integer x (x values repeat; the last 10 rows are never gathered)


def _guarded_flat(t, dev, dtype=torch.float32):
    """a Flat holding t (float32 / int32 / int64), and a snapshot of its bits"""
    t = t.contiguous().view(-1)
    if dtype == torch.int64:
        f = Flat(2 * t.numel(), dev, torch.int32)
        f.t = f.buf[f.g:f.g + 2 * t.numel()].view(torch.int64)
    else:
        f = Flat(t.numel(), dev, dtype)
    f.t.copy_(t.to(dev, dtype))
    f.snap = f.buf.clone()
    return f


@functools.lru_cache(None)
def fl_operands(dout, nb, indexed):
    """float32 tables (weight or bases, comp, root, bias), g, and an integer x (None when not indexed) for the module's graph"""
    gen = torch.Generator().manual_seed(dout * 17 + nb * 3 + indexed)
    in_rows = FL_IN_ROWS if indexed else N
    w = torch.randn(nb if nb else R, in_rows, dout, generator=gen)
    comp = torch.randn(R, nb, generator=gen) if nb else None
    root = torch.randn(in_rows, dout, generator=gen)
    bias = torch.randn(dout, generator=gen)
    dg = torch.randn(N, dout, generator=gen)
    x = torch.randint(0, in_rows - 10, (N,), generator=gen) if indexed else None
    return dict(w=w, comp=comp, root=root, bias=bias, dg=dg, x=x, in_rows=in_rows)


def fl_call_fwd(ps, o, dout, nb, ldo, dev, x=None, root=True, bias=True):
    lib = _lib().load()
    ins = {"weight": _guarded_flat(o["w"], dev), "root": _guarded_flat(o["root"], dev), "bias": _guarded_flat(o["bias"], dev)}
    if nb:
        ins["comp"] = _guarded_flat(o["comp"], dev)
    x = o["x"] if x is None else x
    if x is not None:
        ins["x"] = _guarded_flat(x, dev, torch.int64)
    out = Guarded(N, ldo, dev, g1=G_OUT)
    p = lambda k: ins[k].ptr if k in ins else None
    st = lib.rgcn_featureless_fwd(C.byref(ps), p("x"), o["in_rows"], p("weight"), p("comp"), nb, p("root") if root else None,
                                  p("bias") if bias else None, out.ptr, ldo, dout, _stream())
    torch.cuda.synchronize()
    for k, f in ins.items():
        assert torch.equal(f.buf, f.snap), f"rgcn_featureless_fwd: input {k} was written"
    return st, out


WANT = ("weight", "comp", "root", "bias")


def fl_call_bwd(ps_t, o, dout, nb, ldg, dev, want=WANT, ws_bytes=None):
    """rgcn_featureless_bwd with the outputs in `want` (others NULL) -> (status, {name: values}, workspace)"""
    from scaling_rgcn_training_amd.conv import _node_index
    L = _lib()
    lib = L.load()
    in_rows = o["in_rows"]
    ins = {"weight": _guarded_flat(o["w"], dev)}
    if nb:
        ins["comp"] = _guarded_flat(o["comp"], dev)
    if o["x"] is not None:
        x64, ptr, perm = _node_index(o["x"].to(dev), in_rows)
        ins["x"] = _guarded_flat(x64, dev, torch.int64)
        ins["inv_ptr"] = _guarded_flat(ptr, dev, torch.int32)
        ins["inv_idx"] = _guarded_flat(perm, dev, torch.int32)
    g = Guarded(N, ldg, dev).fill(o["dg"])
    sizes = {"weight": o["w"].numel(), "comp": R * nb, "root": in_rows * dout, "bias": dout}
    outs = {k: Flat(sizes[k], dev) for k in want if sizes[k]}
    need = lib.rgcn_featureless_bwd_workspace_bytes(C.byref(ps_t), dout, nb, int(o["x"] is not None))
    assert need > 0
    ws = Workspace(need if ws_bytes is None else ws_bytes, dev)
    p = lambda d, k: d[k].ptr if k in d else None
    st = lib.rgcn_featureless_bwd(C.byref(ps_t), p(ins, "x"), p(ins, "inv_ptr"), p(ins, "inv_idx"), in_rows, g.ptr, ldg, dout,
                                  p(ins, "weight"), p(ins, "comp"), nb, ws.ptr, ws.n, p(outs, "weight"), p(outs, "comp"),
                                  p(outs, "root"), p(outs, "bias"), _stream())
    torch.cuda.synchronize()
    ws.check("rgcn_featureless_bwd workspace")
    g.unchanged("rgcn_featureless_bwd g")
    for k, f in ins.items():
        assert torch.equal(f.buf, f.snap), f"rgcn_featureless_bwd: input {k} was written"
    vals = {k: f.out(f"featureless d_{k}") for k, f in outs.items()}
    return st, vals, need


def _fl_ref(o, dout, x=None):
    x = o["x"] if x is None else x
    return O.featureless_reference(x, *graph(), o["w"], o["comp"], o["root"], o["bias"], o["dg"], "mean")


FL_CASES = [(16, 64, 7, 0, False), (16, 128, 5, 3, True), (48, 64, 33, 2, False), (48, 128, 24, 0, True),
            (128, 64, 128, 0, False), (128, 128, 128, 1, True), (128, 64, 1, 2, True)]


@pytest.mark.parametrize("k", range(3), ids=["round4", "round4+4", "padded+4"])
@pytest.mark.parametrize("tile,chunk,dout,nb,indexed", FL_CASES, ids=lambda v: str(v))
def test_featureless_guarded(dev, tile, chunk, dout, nb, indexed, k):
    fp = plans(tile, chunk, 0)
    ps, ps_t = _lib().plan_struct(fp.fwd), _lib().plan_struct(fp.bwd)
    assert (ps.tile, ps.chunk, ps.layout, ps_t.tile, ps_t.chunk) == (tile, chunk, 0, tile, chunk)
    assert N % tile != 0
    o = fl_operands(dout, nb, indexed)
    ref, cond = _fl_ref(o, dout)
    tag = f"tile {tile} chunk {chunk} out {dout} B {nb} x {indexed} ld {k}"
    ldo, ldg = _pair(dout, dout, k)
    st, out = fl_call_fwd(ps, o, dout, nb, ldo, dev)
    assert st == OK, tag
    assert_close(out.out(dout, "featureless out " + tag), ref["out"].numpy(), cond["out"].numpy(), "abi featureless out " + tag)
    # root and bias may be NULL
    st, out = fl_call_fwd(ps, o, dout, nb, ldo, dev, root=False, bias=False)
    assert st == OK
    xn = torch.arange(N) if o["x"] is None else o["x"]
    assert_close(out.out(dout, "featureless out no root " + tag), (ref["out"] - o["root"].double()[xn] - o["bias"].double()).numpy(),
                 cond["out"].numpy(), "abi featureless out without root / bias " + tag)
    # the backward: all outputs, then every subset with the others NULL, bit-identical
    st, full, need = fl_call_bwd(ps_t, o, dout, nb, ldg, dev)
    assert st == OK, tag
    for name in full:
        got = full[name].view(ref[name].shape).double().cpu().numpy()
        assert_close(got, ref[name].numpy(), cond[name].numpy(), f"abi featureless d_{name} {tag}")
    names = [n for n in WANT if n != "comp" or nb]
    for mask in range(1 << len(names)):
        sub = tuple(n for i, n in enumerate(names) if mask >> i & 1)
        if len(sub) == len(names):
            continue
        st, vals, _ = fl_call_bwd(ps_t, o, dout, nb, ldg, dev, want=sub)
        assert st == OK and set(vals) == set(sub), (sub, st)
        for name in sub:
            assert torch.equal(vals[name], full[name]), f"{tag}: d_{name} with only {sub} differs from the all-outputs call"
    if k == 0:
        st, _, _ = fl_call_bwd(ps_t, o, dout, nb, ldg, dev, ws_bytes=need - 1)
        assert st == ERR_WORKSPACE


@pytest.mark.parametrize("nb", [1, 2])
def test_featureless_lds_past_64k(dev, nb):
    """tile 128 x out 128: the basis backward with one basis needs 131,840 B of LDS and runs; with two, 197,632 B > 160 KiB,
    RGCN_ERR_LDS before anything is launched"""
    fp = plans(128, 64, 0)
    o = fl_operands(128, nb, False)
    st, vals, _ = fl_call_bwd(_lib().plan_struct(fp.bwd), o, 128, nb, 128, dev)
    if nb == 1:
        assert st == OK
        ref, cond = _fl_ref(o, 128)
        for name in vals:
            assert_close(vals[name].view(ref[name].shape).double().cpu().numpy(), ref[name].numpy(), cond[name].numpy(),
                         f"abi featureless d_{name} LDS 131,840 B")
    else:
        assert st == ERR_LDS
        for f in vals.values():
            assert bool((f.view(torch.int32) == SENT).all()), "a refused call wrote an output"


@pytest.mark.parametrize("nb", [0, 2])
def test_featureless_out_of_range_index_reads_zeros(dev, nb):
    """x_index entries in_rows and -1 gather zero rows (table, root) in the forward, as the header promises"""
    fp = plans(48, 64, 0)
    dout = 12
    o = fl_operands(dout, nb, True)
    x = o["x"].clone()
    x[::7] = FL_IN_ROWS
    x[3::11] = -1
    st, out = fl_call_fwd(_lib().plan_struct(fp.fwd), o, dout, nb, r4(dout), dev, x=x)
    assert st == OK
    # the reference: one zero row appended to every table, the out-of-range entries pointed at it
    z = dict(o)
    z["w"] = torch.cat([o["w"], torch.zeros(o["w"].shape[0], 1, dout)], 1)
    z["root"] = torch.cat([o["root"], torch.zeros(1, dout)])
    xr = torch.where((x < 0) | (x >= FL_IN_ROWS), torch.full_like(x, FL_IN_ROWS), x)
    ref, cond = _fl_ref(z, dout, x=xr)
    assert_close(out.out(dout, "featureless out-of-range x"), ref["out"].numpy(), cond["out"].numpy(),
                 "abi featureless out, x out of range")


# ---- max aggregation: rgcn_segment_max / rgcn_segment_max_bwd on guarded operands ---------------------------------------------
MAX_WIDTHS = [1, 7, 20, 64, 100, 128]       # lane groups of 4 / 8 / 16 / 32 per row; 1, 7 and 100 are not multiples of 4


def _max_inputs(w, seed):
    """700 rows of width w (even columns integers in -2 .. 2: ties and maxima of 0; odd columns normal), 40 segments of 0 .. 699
    gathered rows (one empty, one of a single row) with integer tie weights, cut into pieces of at most 256 rows"""
    gen = torch.Generator().manual_seed(seed)
    n_out = 40
    x = torch.randn(N, w, generator=gen)
    x[:, ::2] = torch.randint(-2, 3, (N, (w + 1) // 2), generator=gen).float()
    lens = torch.randint(0, 700, (n_out,), generator=gen)
    lens[3], lens[7] = 0, 1
    idx = torch.randint(0, N, (int(lens.sum()),), generator=gen)
    sw = torch.randint(1, 4, (idx.shape[0],), generator=gen).float()
    starts = np.concatenate([[0], np.cumsum(lens.numpy())])
    p1, seg_of_piece = [0], []
    for s in range(n_out):
        for a in range(starts[s], starts[s + 1], 256):
            p1.append(min(a + 256, starts[s + 1]))
            seg_of_piece.append(s)
    p2 = np.searchsorted(np.array(seg_of_piece), np.arange(n_out + 1), side="left")
    return x, idx, sw, starts, np.array(p1), p2


def _segmax_ref(vals, ties, ptr):
    """(max, tie weight) per segment of consecutive rows, float64 (every value an fp32 number, every tie weight a small integer)"""
    n = len(ptr) - 1
    out, out_t = np.zeros((n, vals.shape[1])), np.zeros((n, vals.shape[1]))
    for i in range(n):
        v, t = vals[ptr[i]:ptr[i + 1]], ties[ptr[i]:ptr[i + 1]]
        if v.shape[0]:
            out[i] = v.max(0)
            out_t[i] = np.where(v == out[i], t, 0).sum(0)
    return out, out_t


def _three_lds(w, k):
    """three row strides of width w, rotated by k, pairwise different"""
    a, b, c = (_strides(w)[(k + j) % 3] for j in range(3))
    b = b if b != a else b + 4
    while c in (a, b):
        c += 4
    return a, b, c


@pytest.mark.parametrize("k", range(3), ids=["round4", "round4+4", "padded+4"])
@pytest.mark.parametrize("w", MAX_WIDTHS)
def test_segment_max_guarded(dev, w, k):
    """rgcn_segment_max, two levels with seg_idx / seg_w / out_t and one level without any of them: sentinels intact, inputs
    unchanged, pad columns of out AND out_t +0.0, max and tie weight exact; an empty segment gives (0, 0); n_out = 0 writes
    nothing"""
    lib = _lib().load()
    x, idx, sw, starts, p1, p2 = _max_inputs(w, 100 * w + k)
    n_pc, n_out = len(p1) - 1, len(p2) - 1
    ld_in, ld_mid, ld_out = _three_lds(w, k)
    i32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int32, device=dev)
    ptr1, ptr2, idx1, w1 = i32(p1), i32(p2), i32(idx.numpy()), sw.to(dev)
    keep = [t.clone() for t in (ptr1, ptr2, idx1, w1)]
    ins = Guarded(N, ld_in, dev).fill(x)
    mid, mid_t = Guarded(n_pc, ld_mid, dev, g1=G_OUT), Guarded(n_pc, ld_mid, dev, g1=G_OUT)
    assert lib.rgcn_segment_max(ins.ptr, None, ld_in, ptr1.data_ptr(), idx1.data_ptr(), w1.data_ptr(), n_pc, w, mid.ptr, mid_t.ptr,
                                ld_mid, _stream()) == OK
    torch.cuda.synchronize()
    ins.unchanged("segment_max in")
    vals, ties = x.double().numpy()[idx.numpy()], np.repeat(sw.double().numpy()[:, None], w, 1)
    r1, t1 = _segmax_ref(vals, ties, p1)
    assert np.array_equal(mid.out(w, "segment_max level 1 out"), r1)
    assert np.array_equal(mid_t.out(w, "segment_max level 1 out_t"), t1)
    mid.snap, mid_t.snap = mid.buf.clone(), mid_t.buf.clone()
    out, out_t = Guarded(n_out, ld_out, dev, g1=G_OUT), Guarded(n_out, ld_out, dev, g1=G_OUT)
    assert lib.rgcn_segment_max(mid.ptr, mid_t.ptr, ld_mid, ptr2.data_ptr(), None, None, n_out, w, out.ptr, out_t.ptr, ld_out,
                                _stream()) == OK
    torch.cuda.synchronize()
    mid.unchanged("segment_max level-2 in")
    mid_t.unchanged("segment_max level-2 in_t")
    r2, t2 = _segmax_ref(vals, ties, starts)
    assert (starts[4] == starts[3]) and not r2[3].any() and not t2[3].any()                  # the empty segment
    got, got_t = out.out(w, "segment_max level 2 out"), out_t.out(w, "segment_max level 2 out_t")
    assert np.array_equal(got, r2) and np.array_equal(got_t, t2)
    assert np.array_equal(r2, _segmax_ref(r1, t1, p2)[0]) and np.array_equal(t2, _segmax_ref(r1, t1, p2)[1])      # any cut
    # one level over consecutive rows of the input itself: no seg_idx, no seg_w, and no out_t (nothing but out is written)
    rows_ptr = np.minimum(starts, N)
    ptr3 = i32(rows_ptr)
    out1 = Guarded(n_out, ld_out, dev, g1=G_OUT)
    assert lib.rgcn_segment_max(ins.ptr, None, ld_in, ptr3.data_ptr(), None, None, n_out, w, out1.ptr, None, ld_out, _stream()) == OK
    torch.cuda.synchronize()
    assert np.array_equal(out1.out(w, "segment_max one level out"), _segmax_ref(x.double().numpy(), np.ones((N, w)), rows_ptr)[0])
    # ... with seg_idx alone and out_t: every weight 1
    out2, out2_t = Guarded(n_out, ld_mid, dev, g1=G_OUT), Guarded(n_out, ld_mid, dev, g1=G_OUT)
    ptr4 = i32(starts)
    assert lib.rgcn_segment_max(ins.ptr, None, ld_in, ptr4.data_ptr(), idx1.data_ptr(), None, n_out, w, out2.ptr, out2_t.ptr, ld_mid,
                                _stream()) == OK
    torch.cuda.synchronize()
    r4, t4 = _segmax_ref(vals, np.ones_like(vals), starts)
    assert np.array_equal(out2.out(w, "segment_max one level (seg_idx) out"), r4)
    assert np.array_equal(out2_t.out(w, "segment_max one level (seg_idx) out_t"), t4)
    # n_out = 0: accepted, nothing written
    none, none_t = Guarded(4, ld_out, dev), Guarded(4, ld_out, dev)
    assert lib.rgcn_segment_max(ins.ptr, None, ld_in, ptr1.data_ptr(), None, None, 0, w, none.ptr, none_t.ptr, ld_out, _stream()) == OK
    torch.cuda.synchronize()
    none.out(w, "segment_max n_out = 0", rows=0)
    none_t.out(w, "segment_max n_out = 0 (out_t)", rows=0)
    ins.unchanged("segment_max in")
    assert all(torch.equal(a, b) for a, b in zip(keep, (ptr1, ptr2, idx1, w1)))


@pytest.mark.parametrize("k", range(3), ids=["round4", "round4+4", "padded+4"])
@pytest.mark.parametrize("w", MAX_WIDTHS)
def test_segment_max_bwd_guarded(dev, w, k):
    """rgcn_segment_max_bwd with and without seg_dh and row_w, x / h, t / dh / c each with its own stride: sentinels intact,
    inputs unchanged, pad columns of c +0.0, and c equal to where(x[src] == h[s], (w dh[d]) / (t[s] + (h[s] == 0)), 0) in fp32
    by torch on the CPU (both sides one correctly rounded product and quotient); n_rows = 0 writes nothing"""
    lib = _lib().load()
    x, idx, sw, starts, _, _ = _max_inputs(w, 100 * w + k + 50)
    n_seg, n_rows = len(starts) - 1, int(starts[-1])
    gen = torch.Generator().manual_seed(w + k)
    seg = torch.repeat_interleave(torch.arange(n_seg), torch.as_tensor(np.diff(starts)))
    hv, tv = _segmax_ref(x.double().numpy()[idx.numpy()], np.repeat(sw.double().numpy()[:, None], w, 1), starts)
    hv, tv = torch.from_numpy(hv).float(), torch.from_numpy(tv).float()
    assert bool((hv == 0).any()) and bool((tv > 1).any())
    n_dh = 64
    dhv = torch.randn(n_dh, w, generator=gen)
    seg_dh = torch.randperm(n_dh, generator=gen)[:n_seg]
    rw = torch.rand(n_rows, generator=gen) + 0.5
    ldx, ldh, ldc = _three_lds(w, k)
    lddh = ldc + 4
    i32 = lambda a: a.to(dev, torch.int32)
    src_d, seg_d, sdh_d, rw_d = i32(idx), i32(seg), i32(seg_dh), rw.to(dev)
    keep = [t.clone() for t in (src_d, seg_d, sdh_d, rw_d)]
    xg, hg, tg, dg = (Guarded(N, ldx, dev).fill(x), Guarded(n_seg, ldh, dev).fill(hv), Guarded(n_seg, ldh, dev).fill(tv),
                      Guarded(n_dh, lddh, dev).fill(dhv))
    for with_dh in (True, False):
        for with_w in (True, False):
            c = Guarded(n_rows, ldc, dev, g1=G_OUT)
            st = lib.rgcn_segment_max_bwd(xg.ptr, ldx, hg.ptr, tg.ptr, ldh, dg.ptr, lddh, src_d.data_ptr(), seg_d.data_ptr(),
                                          sdh_d.data_ptr() if with_dh else None, rw_d.data_ptr() if with_w else None, n_rows, w,
                                          c.ptr, ldc, _stream())
            torch.cuda.synchronize()
            assert st == OK
            d = dhv[seg_dh[seg] if with_dh else seg]
            num = rw[:, None] * d if with_w else d
            want = torch.where(x[idx] == hv[seg], num / (tv[seg] + (hv[seg] == 0)), torch.zeros_like(num))
            got = c.out(w, f"segment_max_bwd c [seg_dh {with_dh} row_w {with_w}]")
            assert np.array_equal(got, want.double().numpy()), int((got != want.double().numpy()).sum())
            for gd, name in ((xg, "x"), (hg, "h"), (tg, "t"), (dg, "dh")):
                gd.unchanged("segment_max_bwd " + name)
    none = Guarded(4, ldc, dev)
    assert lib.rgcn_segment_max_bwd(xg.ptr, ldx, hg.ptr, tg.ptr, ldh, dg.ptr, lddh, src_d.data_ptr(), seg_d.data_ptr(), None, None, 0, w,
                                    none.ptr, ldc, _stream()) == OK
    torch.cuda.synchronize()
    none.out(w, "segment_max_bwd n_rows = 0", rows=0)
    assert all(torch.equal(a, b) for a, b in zip(keep, (src_d, seg_d, sdh_d, rw_d)))
