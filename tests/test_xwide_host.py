"""RGCNConv wider than 128 (opt-in ``wide=True``): constructor contract, routing refusals and the C argument checks of the
rgcn_xwide_* entry points -- nothing here needs a GPU, and no call reaches one (every C call stops at an argument check).  The
arithmetic is pinned by tests/test_gpu_xwide.py."""
import ctypes

import pytest
import torch

from scaling_rgcn_training_amd import _lib, conv as conv_mod
from scaling_rgcn_training_amd.conv import RGCNConv

NULL, WIDTH, STRIDE, PLAN, LDS, WS, DEVICE, ACT = -1, -2, -3, -4, -5, -6, -7, -8
_DUMMY = (ctypes.c_int32 * 64)()       # plan arrays: host memory the argument checks see as non-NULL and never read


def test_narrow_limit_stays_without_the_flag():
    with pytest.raises(ValueError):
        RGCNConv(200, 8, 3)
    with pytest.raises(ValueError):
        RGCNConv(8, 129, 3, wide=False)
    assert RGCNConv(8, 4, 3).wide is False


def test_wide_layers_have_pygs_parameters():
    full = RGCNConv(200, 8, 3, wide=True)
    assert [k for k, _ in full.named_parameters()] == ["weight", "root", "bias"]
    assert full.weight.shape == (3, 200, 8) and full.root.shape == (200, 8) and full.bias.shape == (8,)
    assert full.comp is None and full.xwide
    basis = RGCNConv(256, 300, 5, num_bases=2, wide=True)
    assert [k for k, _ in basis.named_parameters()] == ["weight", "comp", "root", "bias"]
    assert basis.weight.shape == (2, 256, 300) and basis.comp.shape == (5, 2)
    block = RGCNConv(512, 256, 4, num_blocks=4, wide=True)
    assert block.weight.shape == (4, 4, 128, 64) and block.root.shape == (512, 256)
    bare = RGCNConv(129, 129, 2, wide=True, root_weight=False, bias=False)
    assert list(bare.state_dict().keys()) == ["weight"]
    # PyG's glorot bound
    assert float(full.weight.detach().abs().max()) <= (6.0 / 208) ** 0.5 + 1e-7
    assert RGCNConv(512, 512, 1, wide=True).weight.shape == (1, 512, 512)


@pytest.mark.parametrize("bad,good", [((513, 8), (512, 8)), ((8, 513), (8, 512)), ((0, 300), (1, 300)), ((300, 0), (300, 1)),
                                      ((513, 513), (512, 512))])
def test_widths_beyond_512_are_refused(bad, good):
    with pytest.raises(ValueError, match="1..512"):
        RGCNConv(*bad, 3, wide=True)
    layer = RGCNConv(*good, 3, wide=True)
    assert layer.weight.shape == (3, *good) and layer.xwide


def test_featureless_with_wide_is_refused():
    with pytest.raises(ValueError, match="featureless"):
        RGCNConv(1000, 200, 3, featureless=True, wide=True)
    with pytest.raises(ValueError, match="featureless"):
        RGCNConv(1000, 16, 3, featureless=True, wide=True)


def test_narrow_layer_with_wide_is_the_same_layer():
    torch.manual_seed(3)
    a = RGCNConv(64, 64, 5, wide=True)
    torch.manual_seed(3)
    b = RGCNConv(64, 64, 5, wide=False)
    assert not a.xwide and a.wide
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa.keys()) == list(sb.keys())
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    for kw in (dict(num_bases=3), dict(num_blocks=4)):
        torch.manual_seed(4)
        c = RGCNConv(64, 64, 5, wide=True, **kw)
        torch.manual_seed(4)
        d = RGCNConv(64, 64, 5, **kw)
        assert all(torch.equal(p, q) for p, q in zip(c.parameters(), d.parameters()))


def test_module_default_switches_wide_on(monkeypatch):
    monkeypatch.setattr(conv_mod, "_WIDE_DEFAULT", True)
    assert RGCNConv(255, 256, 3).xwide
    assert RGCNConv(64, 64, 3, wide=False).wide is False
    with pytest.raises(ValueError):
        RGCNConv(255, 256, 3, wide=False)
    # a featureless layer keeps its own 128-column limit under the default
    assert RGCNConv(1000, 16, 3, featureless=True).wide is False
    with pytest.raises(ValueError):
        RGCNConv(1000, 200, 3, featureless=True)
    monkeypatch.setattr(conv_mod, "_WIDE_DEFAULT", False)
    with pytest.raises(ValueError):
        RGCNConv(255, 256, 3)


def test_routing_refusals():
    ei = torch.tensor([[0, 1], [1, 2]])
    et = torch.tensor([0, 1])
    x = torch.randn(3, 200)
    layer = RGCNConv(200, 8, 3, wide=True)
    layer.dist = object()
    with pytest.raises(NotImplementedError):
        layer(x, ei, et)
    with pytest.raises(NotImplementedError):
        layer.layout(3, 2)
    layer = RGCNConv(200, 8, 3, wide=True)
    for path in ("ep", ("ring", "ep"), ("ep", "ring")):
        layer.path = path
        with pytest.raises(ValueError, match="edge-parallel"):
            layer(x, ei, et)
    layer.path = "ring"
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer(x, ei, et)


# ---- the C argument checks (no device memory, no launch) ----------------------------------------------------------------
def _plan(layout=0, chunk=64, chunk_rows=0, tile=16):
    p = ctypes.addressof(_DUMMY)
    n_tiles = (1000 + tile - 1) // tile
    return _lib.RgcnPlanStruct(1000, 1000, 3, tile, n_tiles, n_tiles, chunk, n_tiles, layout, chunk_rows,
                               p, p, p, p, p, p, p, p, p, p, p if layout == 5 else None)


def _tile_lds(tile, chunk, n):
    """LDS bytes of the forward / dX kernel (csrc/rgcn_xwide.hip tile_lds_bytes) for an output width n: a 32-column
    K-slice of `chunk` gathered rows (stride 36), a 32 x NB slice of W (stride NB + 16), the slots' destinations and the tile x NB
    accumulator, NB = 64 or 128 columns per workgroup"""
    nb = 64 if n <= 64 else 128
    return chunk * 36 * 4 + 32 * (nb + 16) * 4 + chunk * 4 + tile * nb * 4


def _refused(ps, widths, strides, pointers, lds_width=None, act=0, nbytes=None, need=None):
    """True when one of the library's argument checks certainly refuses the call (so nothing can be launched): a required pointer
    is NULL, a width is outside 1..512, a stride is not a multiple of 4 or below round4(width), the plan has NULL arrays or a
    layout other than 0, the activation code is unknown, the forward / dX accumulator does not fit 160 KiB, or the workspace is
    short of the query"""
    if any(p is None for p in pointers) or not ps.tile_ptr:
        return True
    if any(not 1 <= w <= 512 for w in widths):
        return True
    if any(ld % 4 or ld < (w + 3) // 4 * 4 for ld, w in strides):
        return True
    if ps.layout != 0 or ps.chunk_rows not in (0, ps.chunk) or act not in (0, 1, 2):
        return True
    if lds_width is not None and _tile_lds(ps.tile, ps.chunk, lds_width) > 160 * 1024:
        return True
    return nbytes is not None and nbytes < need


def _calls(ps, din=200, dout=300, ld_in=200, ld_out=300, x=True, w=True, out=True, nbytes=None, act=0, ldr=None,
           which=("fwd", "bwd_dx", "bwd_dw")):
    """status of the launching entry points named in ``which``.  Every call must stop at an argument check: the plan arrays are
    host memory, and a launch on them faults the GPU.  So each call is refused here, before it is made, unless ``_refused``
    shows the library will refuse it; and a status of RGCN_ERR_DEVICE (a machine without a gfx950 GPU) means the call passed
    every argument check, which fails the test as well."""
    lib = _lib.load()
    b, d = ctypes.byref(ps), ctypes.addressof(_DUMMY)
    need = lib.rgcn_xwide_bwd_dw_workspace_bytes(b, din, dout)
    nb = max(need, 1) - 1 if nbytes is None else nbytes
    xp, wp, op = (d if x else None), (d if w else None), (d if out else None)
    mask = d if ldr is not None else None
    calls = {
        "fwd": (_refused(ps, (din, dout), ((ld_in, din), (ld_out, dout)), (xp, wp, op), lds_width=dout, act=act),
                lambda: lib.rgcn_xwide_fwd(b, xp, ld_in, din, wp, None, op, ld_out, dout, act, None)),
        "bwd_dx": (_refused(ps, (din, dout), ((ld_out, dout), (ld_in, din)) + (((ldr, din),) if ldr is not None else ()),
                            (xp, wp, op), lds_width=din),
                   lambda: lib.rgcn_xwide_bwd_dx(b, xp, ld_out, dout, wp, op, ld_in, din, mask, ldr or 0, None)),
        "bwd_dw": (_refused(ps, (din, dout), ((ld_in, din), (ld_out, dout)), (xp, op, wp), nbytes=nb, need=need),
                   lambda: lib.rgcn_xwide_bwd_dw(b, xp, ld_in, din, op, ld_out, dout, wp, nb, d, d, d, None)),
    }
    got = {}
    for name in which:
        refused, call = calls[name]
        assert refused, f"{name}: these arguments pass every check -- the call would launch a kernel on host memory"
        got[name] = call()
        assert got[name] not in (0, DEVICE), f"{name}: status {got[name]}: the call passed every argument check"
    return got


def test_accepted_calls_stop_before_the_device():
    big = _plan(tile=32768)
    assert _calls(big) == {"fwd": LDS, "bwd_dx": LDS, "bwd_dw": WS}
    assert _calls(big, ldr=200)["bwd_dx"] == LDS
    assert _calls(big, act=2)["fwd"] == LDS
    assert _calls(big, act=3)["fwd"] == ACT


@pytest.mark.parametrize("din,dout", [(0, 300), (513, 300), (200, 0), (200, 513), (-1, 16)])
def test_width(din, dout):
    got = _calls(_plan(tile=32768), din=din, dout=dout, ld_in=1024, ld_out=1024, nbytes=1 << 40)
    assert got == {"fwd": WIDTH, "bwd_dx": WIDTH, "bwd_dw": WIDTH}
    lib = _lib.load()
    assert lib.rgcn_xwide_bwd_dw_workspace_bytes(ctypes.byref(_plan()), din, dout) == 0
    t, c = ctypes.c_int(), ctypes.c_int()
    assert lib.rgcn_xwide_geometry(1000, din, dout, ctypes.byref(t), ctypes.byref(c)) == WIDTH


@pytest.mark.parametrize("din,ld_in,dout,ld_out", [(200, 198, 300, 300), (200, 202, 300, 300), (255, 252, 8, 8),
                                                   (200, 200, 300, 296), (200, 200, 7, 6), (200, 200, 512, 510), (1, 0, 4, 4)])
def test_stride(din, ld_in, dout, ld_out):
    got = _calls(_plan(tile=32768), din=din, dout=dout, ld_in=ld_in, ld_out=ld_out, nbytes=1 << 40)
    assert got == {"fwd": STRIDE, "bwd_dx": STRIDE, "bwd_dw": STRIDE}
    # the ReLU mask of dX: stride of the input width
    assert _calls(_plan(tile=32768), ldr=198)["bwd_dx"] == STRIDE


def test_null():
    big = _plan(tile=32768)
    for kw in (dict(x=False), dict(w=False), dict(out=False)):
        got = _calls(big, nbytes=1 << 40, **kw)
        assert got["fwd"] == NULL and got["bwd_dx"] == NULL and got["bwd_dw"] == NULL, kw
    lib = _lib.load()
    d = ctypes.addressof(_DUMMY)
    assert lib.rgcn_xwide_fwd(None, d, 200, 200, d, None, d, 300, 300, 0, None) == NULL
    assert lib.rgcn_xwide_bwd_dx(None, d, 300, 300, d, d, 200, 200, None, 0, None) == NULL
    assert lib.rgcn_xwide_bwd_dw(None, d, 200, 200, d, 300, 300, d, 1 << 40, d, d, d, None) == NULL
    assert lib.rgcn_xwide_geometry(1000, 200, 300, None, None) == NULL
    empty = _lib.RgcnPlanStruct()
    assert _calls(empty, nbytes=1 << 40) == {"fwd": NULL, "bwd_dx": NULL, "bwd_dw": NULL}


@pytest.mark.parametrize("layout,chunk,chunk_rows", [(1, 128, 0), (2, 64, 0), (3, 128, 0), (5, 64, 0), (0, 128, 112), (4, 64, 0)])
def test_plan_layouts_other_than_0_are_refused(layout, chunk, chunk_rows):
    ps = _plan(layout, chunk, chunk_rows, tile=32768)
    assert _calls(ps, nbytes=1 << 40) == {"fwd": PLAN, "bwd_dx": PLAN, "bwd_dw": PLAN}
    assert _lib.load().rgcn_xwide_bwd_dw_workspace_bytes(ctypes.byref(ps), 200, 300) == 0


def test_layout_0_with_either_chunk_is_accepted():
    for chunk in (64, 128):
        assert _calls(_plan(0, chunk, chunk, tile=32768)) == {"fwd": LDS, "bwd_dx": LDS, "bwd_dw": WS}


def test_workspace():
    lib = _lib.load()
    ps = _plan()
    small = lib.rgcn_xwide_bwd_dw_workspace_bytes(ctypes.byref(ps), 16, 16)
    big = lib.rgcn_xwide_bwd_dw_workspace_bytes(ctypes.byref(ps), 512, 512)
    assert 0 < small < big and small % 256 == 0 and big % 256 == 0
    for nbytes in (big - 1, 0):
        assert _calls(ps, din=512, dout=512, ld_in=512, ld_out=512, nbytes=nbytes, which=("bwd_dw",)) == {"bwd_dw": WS}


@pytest.mark.parametrize("width", [1, 129, 255, 256, 512])
def test_geometry_fits_lds(width):
    """the geometry at every width (either side) fits both directions' kernels in 160 KiB, and an LDS-sized tile beyond it is
    what the entry points refuse"""
    lib = _lib.load()
    for n_nodes in (1, 1000, 40000, 2_100_000):
        for din, dout in ((width, width), (width, 16), (16, width), (width, 512)):
            t, c = ctypes.c_int(), ctypes.c_int()
            assert lib.rgcn_xwide_geometry(n_nodes, din, dout, ctypes.byref(t), ctypes.byref(c)) == 0
            assert t.value % 16 == 0 and 16 <= t.value <= 192 and c.value in (64, 128)
            assert _tile_lds(t.value, c.value, dout) <= 160 * 1024 and _tile_lds(t.value, c.value, din) <= 160 * 1024
            assert lib.rgcn_xwide_bwd_dw_workspace_bytes(ctypes.byref(_plan(0, c.value, 0, tile=t.value)), din, dout) > 0
    # the model above is the one the entry points check: 288 rows of 128 columns do not fit (RGCN_ERR_LDS), 256 rows...
    assert _tile_lds(288, 64, 512) > 160 * 1024 >= _tile_lds(256, 64, 512)
    ld = (width + 3) // 4 * 4
    assert _calls(_plan(tile=288), din=width, dout=512, ld_in=ld, ld_out=512, which=("fwd",)) == {"fwd": LDS}
    assert _calls(_plan(tile=288), din=512, dout=width, ld_in=512, ld_out=ld, which=("bwd_dx",)) == {"bwd_dx": LDS}
    t, c = ctypes.c_int(), ctypes.c_int()
    assert lib.rgcn_xwide_geometry(0, width, width, ctypes.byref(t), ctypes.byref(c)) == PLAN


def test_abi_version_moves_to_19():
    assert _lib.ABI_VERSION == 19 and _lib.load().rgcn_abi_version() == 19
    assert _lib.XWIDE_MAX_WIDTH == 512
