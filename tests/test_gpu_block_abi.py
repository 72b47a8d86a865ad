"""C ABI of the mini-batch block kernels (rgcn_mb_*): the size queries, every refusal code of the header's table answered before
anything is launched (workspace, arena, H, Z and every output keep their sentinel), served calls that write nothing outside their
buffers (guard words around the workspace and the arena, sentinel tails behind H, Z, dH and every output), ids out of range
found on the device, a served pass in which every leading dimension has a value of its own and the columns past ``round4(width)``
are NaN on the way in and keep their sentinel on the way out, ``d_root == NULL``, and the table of d_weight slab counts behind
``rgcn_mb_bwd_dw_workspace_bytes`` on either side of each of its clamps."""
import ctypes as C

import pytest
import torch

from tests import bipartite_reference as B
from tests import block_index_reference as X

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OK, NULL, STRIDE, PLAN, WS, GRAPH, ARG = 0, -1, -3, -4, -6, -9, -11
SENT8, SENTF = 0xA5, -77.0
NS, ND, NREL, DIN, DOUT, GUARD, TAIL = 700, 300, 3, 33, 100, 4096, 16


def _L():
    from scaling_rgcn_training_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


class Call:
    """one well-formed call of each entry point; keyword overrides swap single arguments"""

    def __init__(self):
        L = _L()
        self.L, self.lib = L, L.load()
        self.ei, self.et = B.bipartite_graph(NS, ND, NREL, seed=4)
        self.e = int(self.et.numel())
        self.dei, self.det = self.ei.to(DEV), self.et.to(DEV)
        self.sizes = (self.e, NS, ND, NREL)
        self.need_ix, self.need_ws = self.lib.rgcn_mb_index_bytes(*self.sizes), self.lib.rgcn_mb_index_workspace_bytes(*self.sizes)
        assert self.need_ix > 0 and self.need_ws > 0
        u8, f32 = dict(dtype=torch.uint8, device=DEV), dict(dtype=torch.float32, device=DEV)
        self.arena = torch.full((GUARD + self.need_ix + GUARD,), SENT8, **u8)
        self.ws = torch.full((GUARD + self.need_ws + GUARD,), SENT8, **u8)
        self.out_ix = L.RgcnMbIndex()
        self.good = L.mb_index_build(self.dei, self.det, NS, ND, NREL)      # a good index for the layer calls
        self.slots = self.good.n_slots
        self.ldi, self.ldo = (DIN + 3) // 4 * 4, (DOUT + 3) // 4 * 4
        g = torch.Generator().manual_seed(2)
        self.x = torch.zeros(NS, self.ldi)
        self.x[:, :DIN] = torch.randn(NS, DIN, generator=g)
        self.g = torch.zeros(ND, self.ldo)
        self.g[:, :DOUT] = torch.randn(ND, DOUT, generator=g)
        self.w = torch.randn(NREL, DIN, DOUT, generator=g) / 8
        self.root = torch.randn(DIN, DOUT, generator=g) / 8
        self.bias = torch.randn(DOUT, generator=g)
        self.dx_, self.dg_, self.dbias = self.x.to(DEV), self.g.to(DEV), self.bias.to(DEV)
        self.packed = L.pack_weights(self.w.to(DEV), self.root.to(DEV), False)
        self.packed_t = L.pack_weights(self.w.to(DEV), self.root.to(DEV), True)
        full = lambda rows, ld: torch.full((rows + TAIL, ld), SENTF, **f32)
        self.h, self.z, self.out = full(self.slots, self.ldi), full(self.slots, self.ldo), full(ND, self.ldo)
        self.dh, self.dx = full(self.slots, self.ldi), full(NS, self.ldi)
        self.dw, self.droot = torch.full((NREL * DIN * DOUT + TAIL,), SENTF, **f32), torch.full((DIN * DOUT + TAIL,), SENTF, **f32)
        self.need_dw = self.lib.rgcn_mb_bwd_dw_workspace_bytes(C.byref(self.good.struct), DIN, DOUT)
        self.ws_dw = torch.full((GUARD + self.need_dw + GUARD,), SENT8, **u8)

    def build(self, **o):
        a = dict(src=self.dei[0].data_ptr(), dst=self.dei[1].data_ptr(), typ=self.det.data_ptr(), e=self.e, ns=NS, nd=ND, r=NREL,
                 mean=1, arena=self.arena[GUARD:].data_ptr(), arena_bytes=self.need_ix, ws=self.ws[GUARD:].data_ptr(),
                 ws_bytes=self.need_ws, out=C.byref(self.out_ix))
        a.update(o)
        return self.lib.rgcn_mb_index_build(a["src"], 1, a["dst"], 1, a["typ"], 1, a["e"], a["ns"], a["nd"], a["r"], a["mean"],
                                            a["arena"], a["arena_bytes"], a["ws"], a["ws_bytes"], a["out"], _stream())

    def fwd(self, **o):
        a = dict(ix=C.byref(self.good.struct), x=self.dx_.data_ptr(), ldx=self.ldi, din=DIN, w=self.packed.data_ptr(),
                 bias=self.dbias.data_ptr(), h=self.h.data_ptr(), ldh=self.ldi, z=self.z.data_ptr(), ldz=self.ldo,
                 out=self.out.data_ptr(), ldo=self.ldo, dout=DOUT)
        a.update(o)
        return self.lib.rgcn_mb_fwd(a["ix"], a["x"], a["ldx"], a["din"], a["w"], a["bias"], a["h"], a["ldh"], a["z"], a["ldz"],
                                    a["out"], a["ldo"], a["dout"], _stream())

    def bwd_dx(self, **o):
        a = dict(ix=C.byref(self.good.struct), g=self.dg_.data_ptr(), ldg=self.ldo, dout=DOUT, w=self.packed_t.data_ptr(),
                 dh=self.dh.data_ptr(), lddh=self.ldi, dx=self.dx.data_ptr(), lddx=self.ldi, din=DIN)
        a.update(o)
        return self.lib.rgcn_mb_bwd_dx(a["ix"], a["g"], a["ldg"], a["dout"], a["w"], a["dh"], a["lddh"], a["dx"], a["lddx"], a["din"],
                                       _stream())

    def bwd_dw(self, **o):
        a = dict(ix=C.byref(self.good.struct), h=self.h.data_ptr(), ldh=self.ldi, din=DIN, g=self.dg_.data_ptr(), ldg=self.ldo,
                 dout=DOUT, dw=self.dw.data_ptr(), droot=self.droot.data_ptr(), ws=self.ws_dw[GUARD:].data_ptr(), ws_bytes=self.need_dw)
        a.update(o)
        return self.lib.rgcn_mb_bwd_dw(a["ix"], a["h"], a["ldh"], a["din"], a["g"], a["ldg"], a["dout"], a["dw"], a["droot"], a["ws"],
                                       a["ws_bytes"], _stream())

    def untouched(self):
        torch.cuda.synchronize()
        for t in (self.arena, self.ws, self.ws_dw):
            assert bool((t == SENT8).all()), "arena / workspace written by a refused call"
        for t in (self.h, self.z, self.out, self.dh, self.dx, self.dw, self.droot):
            assert bool((t == SENTF).all()), "output written by a refused call"
        assert self.out_ix.n_tiles == 0 and self.out_ix.tile_ptr is None, "index struct written by a refused call"

    def struct_with(self, **fields):
        s = self.L.RgcnMbIndex()
        C.memmove(C.byref(s), C.byref(self.good.struct), C.sizeof(s))
        for k, v in fields.items():
            setattr(s, k, v)
        return C.byref(s)


def test_abi_version_and_size_queries():
    L = _L()
    lib = L.load()
    assert lib.rgcn_abi_version() == 19 == L.ABI_VERSION
    for q in (lib.rgcn_mb_index_bytes, lib.rgcn_mb_index_workspace_bytes):
        assert q(-1, 10, 5, 3) == 0 and q(10, -1, 0, 3) == 0 and q(10, 10, -1, 3) == 0 and q(10, 5, 6, 3) == 0
        assert q(10, 10, 5, 0) == 0 and q(10, 10, 5, 65537) == 0 and q(10, 2 ** 31, 5, 3) == 0 and q(0xFFFF0000, 10, 5, 3) == 0
        assert q(0, 0, 0, 1) > 0 and q(0, 1, 1, 1) > 0 and q(0xFFFF0000 - 1_200_000, 100, 5, 65536) > 0
        a, b, c, d = q(1000, 500, 100, 3), q(2000, 500, 100, 3), q(2000, 900, 100, 3), q(2000, 900, 400, 3)
        assert 0 < a < b <= c < d < q(2000, 900, 400, 300)
    c = Call()
    qd = lib.rgcn_mb_bwd_dw_workspace_bytes
    assert qd(None, 8, 8) == 0 and qd(C.byref(c.good.struct), 0, 8) == 0 and qd(C.byref(c.good.struct), 8, 129) == 0
    big = c.struct_with(n_tiles=c.good.n_tiles)          # (the same index: the query depends on its counts and the widths only)
    assert qd(big, 64, 64) >= qd(big, 16, 16) >= 0 and qd(big, DIN, DOUT) == c.need_dw


def test_index_build_refusals_launch_nothing():
    c = Call()
    for o, want in (
            (dict(src=None), NULL), (dict(dst=None), NULL), (dict(typ=None), NULL), (dict(arena=None), NULL), (dict(ws=None), NULL),
            (dict(out=None), NULL),
            (dict(arena_bytes=c.need_ix - 1), WS), (dict(ws_bytes=c.need_ws - 1), WS), (dict(ws_bytes=0), WS),
            (dict(ns=2 ** 31), PLAN), (dict(ns=2 ** 31 + 5, nd=2 ** 31), PLAN), (dict(e=0xFFFF0000), PLAN), (dict(e=0xFFFF0001), PLAN),
            (dict(r=0), PLAN), (dict(r=65537), PLAN),
            (dict(e=-1), ARG), (dict(ns=-1), ARG), (dict(nd=-1), ARG), (dict(nd=NS + 1), ARG),
    ):
        assert c.build(**o) == want, o
        c.untouched()


def test_layer_refusals_launch_nothing():
    c = Call()
    for call, cases in (
            (c.fwd, ((dict(ix=None), NULL), (dict(x=None), NULL), (dict(w=None), NULL), (dict(h=None), NULL), (dict(z=None), NULL),
                     (dict(out=None), NULL), (dict(ix=c.struct_with(tile_ptr=None)), NULL), (dict(ix=c.struct_with(edge_src=None)), NULL),
                     (dict(din=0), PLAN), (dict(din=129), PLAN), (dict(dout=0), PLAN), (dict(dout=129), PLAN),
                     (dict(ix=c.struct_with(num_relations=65537)), PLAN), (dict(ix=c.struct_with(n_tiles=-1)), PLAN),
                     (dict(ix=c.struct_with(n_src=ND - 1)), ARG), (dict(ix=c.struct_with(num_edges=-1)), ARG),
                     (dict(ldx=DIN), STRIDE), (dict(ldo=DOUT - 4), STRIDE))),
            (c.bwd_dx, ((dict(ix=None), NULL), (dict(g=None), NULL), (dict(w=None), NULL), (dict(dh=None), NULL), (dict(dx=None), NULL),
                        (dict(ix=c.struct_with(src_row=None)), NULL), (dict(din=129), PLAN), (dict(dout=0), PLAN),
                        (dict(ix=c.struct_with(n_dst=NS + 1)), ARG), (dict(lddx=DIN), STRIDE))),
            (c.bwd_dw, ((dict(ix=None), NULL), (dict(h=None), NULL), (dict(g=None), NULL), (dict(ix=c.struct_with(row_dst=None)), NULL),
                        (dict(din=0), PLAN), (dict(dout=200), PLAN), (dict(ix=c.struct_with(n_dst=-1)), ARG),
                        (dict(ldg=DOUT + 1), STRIDE))
             + (((dict(ws=None), NULL), (dict(ws_bytes=c.need_dw - 1), WS)) if c.need_dw else ())),
    ):
        for o, want in cases:
            assert call(**o) == want, (call.__name__, o)
            c.untouched()


def test_served_calls_stay_inside_their_buffers():
    c = Call()
    assert c.build() == OK
    torch.cuda.synchronize()
    assert bool((c.arena[:GUARD] == SENT8).all()) and bool((c.arena[GUARD + c.need_ix:] == SENT8).all())
    assert bool((c.ws[:GUARD] == SENT8).all()) and bool((c.ws[GUARD + c.need_ws:] == SENT8).all())
    got, want = c.L.MbIndex(c.out_ix, c.arena), X.build(c.ei, c.et, NS, ND, NREL)
    for name in X.ARRAYS:
        assert torch.equal(getattr(got, name).cpu(), getattr(want, name)), name
    assert c.fwd() == OK and c.bwd_dx() == OK and c.bwd_dw() == OK
    torch.cuda.synchronize()
    for t, rows in ((c.h, c.slots), (c.z, c.slots), (c.out, ND), (c.dh, c.slots), (c.dx, NS)):
        assert bool((t[rows:] == SENTF).all()) and not bool((t[:rows] == SENTF).any())
    assert bool((c.dw[NREL * DIN * DOUT:] == SENTF).all()) and bool((c.droot[DIN * DOUT:] == SENTF).all())
    assert bool((c.ws_dw[:GUARD] == SENT8).all()) and bool((c.ws_dw[GUARD + c.need_dw:] == SENT8).all())
    # the results are the layer's
    x64, g64 = c.x[:, :DIN].double(), c.g[:, :DOUT].double()
    ref, cond, _ = B.reference(x64, x64[:ND], c.ei, c.et, c.w.double(), c.root.double(), c.bias.double(), g64)
    from oracle.tolerance import assert_close
    assert_close(c.out[:ND, :DOUT].cpu().numpy(), ref["out"], cond["out"], "rgcn_mb_fwd")
    dx, dxc = ref["x_src"].copy(), cond["x_src"].copy()
    dx[:ND] += ref["x_dst"]
    dxc[:ND] += cond["x_dst"]
    assert_close(c.dx[:NS, :DIN].cpu().numpy(), dx, dxc, "rgcn_mb_bwd_dx")
    assert_close(c.dw[:NREL * DIN * DOUT].view(NREL, DIN, DOUT).cpu().numpy(), ref["weight"], cond["weight"], "rgcn_mb_bwd_dw")
    assert_close(c.droot[:DIN * DOUT].view(DIN, DOUT).cpu().numpy(), ref["root"], cond["root"], "rgcn_mb_bwd_dw root")
    # either gradient alone; a block without destinations launches nothing
    c.dw.fill_(SENTF)
    assert c.bwd_dw(dw=None) == OK
    torch.cuda.synchronize()
    assert bool((c.dw == SENTF).all())
    empty = c.L.mb_index_build(torch.zeros(2, 0, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV), 4, 0, NREL)
    c.out.fill_(SENTF)
    assert c.fwd(ix=C.byref(empty.struct)) == OK
    torch.cuda.synchronize()
    assert bool((c.out == SENTF).all()) and (empty.n_tiles, empty.n_rows) == (0, 0)


def test_bad_ids_are_found_on_the_device():
    c = Call()
    for row, col, val in ((0, 17, NS), (0, 3, -1), (1, 900, ND), (1, 5, -4), (2, 5, NREL), (2, 6, -3), (0, 9, 2 ** 40)):
        t = torch.stack([c.ei[0], c.ei[1], c.et]).clone()
        t[row, col] = val
        d = t.to(DEV)
        assert c.build(src=d[0].data_ptr(), dst=d[1].data_ptr(), typ=d[2].data_ptr()) == GRAPH, (row, col, val)
        torch.cuda.synchronize()
        assert bool((c.arena[:GUARD] == SENT8).all()) and bool((c.arena[GUARD + c.need_ix:] == SENT8).all())
        assert bool((c.ws[:GUARD] == SENT8).all()) and bool((c.ws[GUARD + c.need_ws:] == SENT8).all())
        assert c.out_ix.tile_ptr is None
    assert c.build(nd=0, ns=NS) == GRAPH          # edges into no destination
    assert c.build() == OK


def _layer_reference(c):
    x64, g64 = c.x[:, :DIN].double(), c.g[:, :DOUT].double()
    ref, cond, _ = B.reference(x64, x64[:ND], c.ei, c.et, c.w.double(), c.root.double(), c.bias.double(), g64)
    ref["x"], cond["x"] = ref["x_src"].copy(), cond["x_src"].copy()
    ref["x"][:ND] += ref["x_dst"]
    cond["x"][:ND] += cond["x_dst"]
    return ref, cond


def test_every_leading_dimension_its_own():
    """ldx, ldh, lddh, lddx (in = 33, round4 = 36) and ldz, ldo, ldg (out = 100) all differ: a kernel that steps through one buffer
    with another's stride reads NaN or leaves sentinels inside a result"""
    from oracle.tolerance import assert_close
    c = Call()
    ldx, ldh, lddh, lddx = c.ldi + 8, c.ldi + 4, c.ldi + 12, c.ldi + 16
    ldz, ldo, ldg = c.ldo + 12, c.ldo + 4, c.ldo + 8
    assert (c.ldi, c.ldo) == (36, 100) and len({ldx, ldh, lddh, lddx}) == 4 and len({ldz, ldo, ldg}) == 3
    f32 = dict(dtype=torch.float32, device=DEV)
    x = torch.full((NS, ldx), float("nan"))
    x[:, :c.ldi] = c.x                                  # (columns 33 .. 35 are zeros, as the ABI requires)
    g = torch.full((ND, ldg), float("nan"))
    g[:, :c.ldo] = c.g
    x, g = x.to(DEV), g.to(DEV)
    full = lambda rows, ld: torch.full((rows + TAIL, ld), SENTF, **f32)
    h, z, out, dh, dx = full(c.slots, ldh), full(c.slots, ldz), full(ND, ldo), full(c.slots, lddh), full(NS, lddx)
    assert c.fwd(x=x.data_ptr(), ldx=ldx, h=h.data_ptr(), ldh=ldh, z=z.data_ptr(), ldz=ldz, out=out.data_ptr(), ldo=ldo) == OK
    assert c.bwd_dx(g=g.data_ptr(), ldg=ldg, dh=dh.data_ptr(), lddh=lddh, dx=dx.data_ptr(), lddx=lddx) == OK
    assert c.bwd_dw(h=h.data_ptr(), ldh=ldh, g=g.data_ptr(), ldg=ldg) == OK
    torch.cuda.synchronize()
    for name, t, rows, r4 in (("h", h, c.slots, c.ldi), ("z", z, c.slots, c.ldo), ("out", out, ND, c.ldo), ("dh", dh, c.slots, c.ldi),
                              ("dx", dx, NS, c.ldi)):
        assert bool((t[rows:] == SENTF).all()) and bool((t[:, r4:] == SENTF).all()), f"{name}: written outside its rows or columns"
        assert bool(torch.isfinite(t[:rows, :r4]).all()) and not bool((t[:rows, :r4] == SENTF).any()), f"{name}: NaN read or a gap left"
    assert bool((c.dw[NREL * DIN * DOUT:] == SENTF).all()) and bool((c.droot[DIN * DOUT:] == SENTF).all())
    assert bool((c.ws_dw[:GUARD] == SENT8).all()) and bool((c.ws_dw[GUARD + c.need_dw:] == SENT8).all())
    assert bool((x[:, c.ldi:] != x[:, c.ldi:]).all()) and bool((g[:, c.ldo:] != g[:, c.ldo:]).all())      # (the inputs are as they were)
    ref, cond = _layer_reference(c)
    assert_close(out[:ND, :DOUT].cpu().numpy(), ref["out"], cond["out"], "rgcn_mb_fwd, own strides")
    assert_close(dx[:NS, :DIN].cpu().numpy(), ref["x"], cond["x"], "rgcn_mb_bwd_dx, own strides")
    assert_close(c.dw[:NREL * DIN * DOUT].view(NREL, DIN, DOUT).cpu().numpy(), ref["weight"], cond["weight"], "rgcn_mb_bwd_dw, own strides")
    assert_close(c.droot[:DIN * DOUT].view(DIN, DOUT).cpu().numpy(), ref["root"], cond["root"], "rgcn_mb_bwd_dw root, own strides")


def test_d_weight_without_d_root():
    from oracle.tolerance import assert_close
    c = Call()
    assert c.fwd() == OK and c.bwd_dw(droot=None) == OK
    torch.cuda.synchronize()
    assert bool((c.droot == SENTF).all()), "d_root written though NULL was passed"
    assert bool((c.dw[NREL * DIN * DOUT:] == SENTF).all())
    assert bool((c.ws_dw[:GUARD] == SENT8).all()) and bool((c.ws_dw[GUARD + c.need_dw:] == SENT8).all())
    ref, cond = _layer_reference(c)
    assert_close(c.dw[:NREL * DIN * DOUT].view(NREL, DIN, DOUT).cpu().numpy(), ref["weight"], cond["weight"], "rgcn_mb_bwd_dw, d_root NULL")


def _slabs(n_tiles, nrel, din, dout):
    """slabs per relation of a d_weight launch: about eight tiles each, the partials at most 2^24 floats (64 MiB), at most 64, at least 1"""
    return max(1, min(-(-n_tiles // (8 * nrel)), 2 ** 24 // (nrel * din * dout), 64))


def test_the_slab_table():
    """host only: the query launches nothing, and the refused rgcn_mb_bwd_dw neither"""
    c = Call()
    qd = c.lib.rgcn_mb_bwd_dw_workspace_bytes

    def query(n_tiles, nrel, din, dout):          # (an index that states these counts: 16 n_tiles edges make room for its slots)
        return qd(c.struct_with(num_edges=16 * n_tiles, n_rows=16 * n_tiles, n_tiles=n_tiles, num_relations=nrel - 1), din, dout)

    def nbytes(slabs, nrel, din, dout):
        return nrel * slabs * din * dout * 4 if slabs > 1 else 0

    pins = (
        # about eight tiles a slab: S = 1 up to 8 nrel tiles, 2 one tile past them
        (1, 4, 16, 16, 1), (32, 4, 16, 16, 1), (33, 4, 16, 16, 2), (64, 4, 16, 16, 2), (65, 4, 16, 16, 3), (0, 4, 16, 16, 1),
        (16, 2, 1, 1, 1), (17, 2, 1, 1, 2), (8 * 601, 601, 16, 13, 1), (8 * 601 + 1, 601, 16, 13, 2),
        # the cap: 63 slabs at 8 nrel 63 tiles, 64 from one tile more, and no more than 64 ever
        (2016, 4, 33, 100, 63), (2017, 4, 33, 100, 64), (2048, 4, 33, 100, 64), (2049, 4, 33, 100, 64), (10 ** 6, 4, 33, 100, 64),
        (1026, 2, 16, 16, 64), (1008, 2, 16, 16, 63),
        # 64 MiB of partials: 2^24 // (21 * 128 * 128) = 48 where the tiles ask for 50; 47 and 48 below the clamp
        (8400, 21, 128, 128, 48), (8065, 21, 128, 128, 48), (8064, 21, 128, 128, 48), (7896, 21, 128, 128, 47),
        (8400, 21, 128, 127, 49), (8400, 21, 64, 128, 50),
        # the floor: 1,025 * 128 * 128 > 2^24 leaves room for no slab at all: one, and no workspace; 512 relations: room for 2
        (10 ** 6, 1025, 128, 128, 1), (10 ** 6, 1024, 128, 128, 1), (10 ** 6, 512, 128, 128, 2), (10 ** 6, 513, 128, 128, 1),
        (10 ** 6, 65537, 16, 16, 1), (10 ** 6, 65536, 16, 16, 1), (10 ** 6, 32768, 16, 16, 2),
    )
    for n_tiles, nrel, din, dout, slabs in pins:
        assert _slabs(n_tiles, nrel, din, dout) == slabs, (n_tiles, nrel, din, dout)
        assert query(n_tiles, nrel, din, dout) == nbytes(slabs, nrel, din, dout), (n_tiles, nrel, din, dout, slabs)
    for nrel in (2, 5, 21, 300, 1025):
        for din, dout in ((1, 1), (16, 16), (33, 100), (64, 64), (128, 128)):
            for n_tiles in (0, 1, 8 * nrel - 1, 8 * nrel, 8 * nrel + 1, 500 * nrel, 504 * nrel + 1, 512 * nrel, 512 * nrel + 1, 10 ** 6):
                assert query(n_tiles, nrel, din, dout) == nbytes(_slabs(n_tiles, nrel, din, dout), nrel, din, dout), (n_tiles, nrel, din, dout)
    assert query(33, 4, 16, 16) == 4 * 2 * 16 * 16 * 4 and query(8400, 21, 128, 128) == 21 * 48 * 128 * 128 * 4
    # a workspace one byte short at S = 64 is refused before anything is launched
    ix = c.struct_with(num_edges=16 * 2017, n_rows=c.good.n_rows, n_tiles=2017)
    need = qd(ix, DIN, DOUT)
    assert need == (NREL + 1) * 64 * DIN * DOUT * 4
    ws = torch.full((need,), SENT8, dtype=torch.uint8, device=DEV)
    assert c.bwd_dw(ix=ix, ws=ws.data_ptr(), ws_bytes=need - 1) == WS
    c.untouched()
    assert bool((ws == SENT8).all())
