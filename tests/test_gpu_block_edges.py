"""``RGCNConv.forward_block`` (csrc/rgcn_minibatch.hip) where tests/test_gpu_block_layer.py stops, against the same fp64 reference
under oracle/tolerance.py: every pair of width classes (16 / 32 / 64 / 128 per side, widths that are no multiple of 4, and the
widths on either side of a class and of a 16-byte piece), the d_weight slabs at their cap of 64, with trailing empty slabs, with
tile counts that the slab count does not divide and with either half frozen (the slab count of each case is asserted through
``rgcn_mb_bwd_dw_workspace_bytes``, and two runs must agree to the bit), a destination whose run of 4,097 edges fills a tile of
its own, and 600 relations (three trips of the relation scan, empty relations at the trips' edges)."""
import ctypes as C

import pytest
import torch

from tests import bipartite_reference as B
from tests import block_index_reference as X
from tests.test_gpu_block_layer import _block, _check, _conv, _data, _run

pytestmark = pytest.mark.gpu

# ---- A. every width class -------------------------------------------------------------------------------------------------------
NS, ND, NREL = 120, 50, 3
GRID = [(i, o) for i in (13, 29, 50, 99) for o in (13, 29, 50, 99)]          # pad to 16, 32, 64, 128: all 16 (KP, NP) pairs
BOUNDS = [(16, 17), (17, 16), (32, 33), (33, 32), (31, 32), (64, 65), (65, 64), (127, 128), (128, 127), (4, 4), (3, 5), (8, 12), (20, 28)]


def _tiny(seed, hub=300):
    """120 -> 50, three relations: a two-row hub (``hub`` edges into destination 0), relation 2 empty, destinations 45 .. 49 isolated"""
    return B.bipartite_graph(NS, ND, NREL, seed, e=400, hub=hub, dup=10)


def _layer(din, dout, ei, et, n_src, n_dst, r, aggr, tag, seed=0):
    conv = _conv(din, dout, r, seed=seed, aggr=aggr)
    x, g = _data(n_src, n_dst, din, dout, 7)
    got = _run(conv, x, _block(ei, et, n_src, n_dst), g)
    assert set(got) == {"out", "x", "weight", "root", "bias"}
    _check(conv, x, ei, et, n_dst, g, got, aggr, f"{din}x{dout} {aggr} {tag}")
    return got


@pytest.mark.parametrize("din,dout", GRID + BOUNDS)
def test_every_width_class(din, dout):
    _layer(din, dout, *_tiny(din + dout), NS, ND, NREL, "mean", "tiny")


@pytest.mark.parametrize("d", [13, 29, 50, 99])
def test_every_width_class_sum(d):
    _layer(d, d, *_tiny(d), NS, ND, NREL, "sum", "tiny")


# ---- B. d_weight slabs ------------------------------------------------------------------------------------------------------------
def _slab_bytes(block, r, aggr, din, dout):
    from scaling_rgcn_training_amd import _lib
    from scaling_rgcn_training_amd.sampling import block_index
    index = block_index(block, r, aggr)
    return index, _lib.load().rgcn_mb_bwd_dw_workspace_bytes(C.byref(index._ix.struct), din, dout)


def _occupancy(tile_ptr, slabs):
    """tiles per (relation, slab) as mb_dw_kernel cuts them: ceil(tiles / slabs) per slab from the front, the rest empty"""
    occ = []
    for t0, t1 in zip(tile_ptr[:-1], tile_ptr[1:]):
        per = (t1 - t0 + slabs - 1) // slabs
        occ.append([max(0, min(t0 + (s + 1) * per, t1) - min(t0 + s * per, t1)) for s in range(slabs)])
    return occ


def _twice(conv, x, block, g, index, **kw):
    a, b = _run(conv, x, block, g, index=index, **kw), _run(conv, x, block, g, index=index, **kw)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: two runs differ"
    return a


def _cap_block():
    n_src, n_dst = 8300, 8200
    g = torch.Generator().manual_seed(21)
    dst = torch.cat([torch.arange(n_dst), torch.randint(0, n_dst, (2 * n_dst,), generator=g)])
    ei = torch.stack([torch.randint(0, n_src, (3 * n_dst,), generator=g), dst])
    return ei, torch.zeros(3 * n_dst, dtype=torch.int64), n_src, n_dst


@pytest.mark.parametrize("aggr", ["mean", "sum"])
def test_dw_slabs_at_the_cap_of_64(aggr):
    """r = 1, 16 x 16: relation 0 and the root have 8,200 rows = 513 tiles each (no run reaches 256 edges), 1,026 tiles in all;
    ceil(1,026 / (8 * 2)) = 65 slabs uncapped, 64 with the cap; a slab is ceil(513 / 64) = 9 tiles, 57 x 9 = 513: the last seven
    slabs of either relation are empty and store zeros for the reduce"""
    ei, et, n_src, n_dst = _cap_block()
    want = X.build(ei, et, n_src, n_dst, 1, aggr)
    assert want.tile_ptr.tolist() == [0, 513, 1026] and int(want.row_cnt.max()) < X.ROW_EDGES
    assert _occupancy(want.tile_ptr.tolist(), 64) == [[9] * 57 + [0] * 7] * 2
    block = _block(ei, et, n_src, n_dst)
    index, nbytes = _slab_bytes(block, 1, aggr, 16, 16)
    assert index.n_tiles == 1026 and nbytes == 2 * 64 * 16 * 16 * 4
    conv = _conv(16, 16, 1, aggr=aggr)
    x, g = _data(n_src, n_dst, 16, 16, 7)
    _check(conv, x, ei, et, n_dst, g, _twice(conv, x, block, g, index), aggr, f"16x16 {aggr} 64 slabs")


def _skew_block():
    n_src, n_dst = 4100, 4000
    g = torch.Generator().manual_seed(22)
    dst = torch.cat([torch.arange(n_dst), torch.tensor([7]), torch.arange(272), torch.tensor([100])])
    typ = torch.cat([torch.zeros(n_dst, dtype=torch.int64), torch.tensor([1]), torch.full((273,), 2)])
    src = torch.randint(0, n_src, (int(typ.numel()),), generator=g)
    src[-1] = src[n_dst + 1 + 100]          # the duplicate of relation 2: the same (source, destination 100) again
    perm = torch.randperm(int(typ.numel()), generator=g)
    return torch.stack([src, dst])[:, perm], typ[perm], n_src, n_dst


SKEW_OCCUPANCY = [[20] * 12 + [10], [1] + [0] * 12, [2] * 8 + [1] + [0] * 4, [0] * 13, [20] * 12 + [10]]


def _skew(aggr="mean"):
    """r = 4, 64 x 64: relation 0 has 4,000 rows = 250 tiles, relation 1 one row (a tile with 15 empty slots), relation 2 272 rows
    = 17 tiles (the duplicate joins a run), relation 3 none, the root 250: 518 tiles, ceil(518 / (8 * 5)) = 13 slabs, which divide
    no relation's tiles: 250 = 12 x 20 + 10, 1 = 1 + twelve empty, 17 = 8 x 2 + 1 + four empty"""
    ei, et, n_src, n_dst = _skew_block()
    want = X.build(ei, et, n_src, n_dst, 4, aggr)
    assert want.tile_ptr.tolist() == [0, 250, 251, 268, 268, 518] and _occupancy(want.tile_ptr.tolist(), 13) == SKEW_OCCUPANCY
    block = _block(ei, et, n_src, n_dst)
    index, nbytes = _slab_bytes(block, 4, aggr, 64, 64)
    assert index.n_tiles == 518 and nbytes == 5 * 13 * 64 * 64 * 4
    return ei, et, n_src, n_dst, block, index


def test_dw_slabs_that_divide_no_relation():
    ei, et, n_src, n_dst, block, index = _skew()
    conv = _conv(64, 64, 4)
    x, g = _data(n_src, n_dst, 64, 64, 7)
    got = _twice(conv, x, block, g, index)
    _check(conv, x, ei, et, n_dst, g, got, "mean", "64x64 skew, 13 slabs")
    assert not bool(got["weight"][3].any()), "d_weight of the empty relation"


@pytest.mark.parametrize("frozen", ["root", "weight"])
def test_dw_slabs_with_a_frozen_half(frozen):
    ei, et, n_src, n_dst, block, index = _skew()
    conv = _conv(64, 64, 4)
    getattr(conv, frozen).requires_grad_(False)
    x, g = _data(n_src, n_dst, 64, 64, 7)
    got = _twice(conv, x, block, g, index)
    assert getattr(conv, frozen).grad is None and set(got) == {"out", "x", "weight", "root", "bias"} - {frozen}
    _check(conv, x, ei, et, n_dst, g, got, "mean", f"64x64 skew, 13 slabs, {frozen} frozen")


# ---- C. a destination that fills tiles; many relations ----------------------------------------------------------------------------
def _hub_block():
    """the tiny block without its hub, and a run of exactly 4,097 edges of relation 1 into destination 3, the relation's first rows
    (its edges into destinations 0 .. 3 are taken out)"""
    ei, et = _tiny(31, hub=0)
    keep = ~((et == 1) & (ei[1] <= 3))
    g = torch.Generator().manual_seed(32)
    hub = torch.stack([torch.randint(0, NS, (4097,), generator=g), torch.full((4097,), 3)])
    return torch.cat([ei[:, keep], hub], 1), torch.cat([et[keep], torch.ones(4097, dtype=torch.int64)])


@pytest.mark.parametrize("aggr", ["mean", "sum"])
@pytest.mark.parametrize("din,dout", [(29, 50), (99, 13), (17, 32)])
def test_a_run_that_fills_a_tile(din, dout, aggr):
    ei, et = _hub_block()
    want = X.build(ei, et, NS, ND, NREL, aggr)
    rows = [s for s in range(16 * want.n_tiles) if int(want.row_cnt[s]) and int(want.row_dst[s]) == 3
            and 16 * int(want.tile_ptr[1]) <= s < 16 * int(want.tile_ptr[2])]
    # 17 slots from the relation's first: 16 rows of 256 edges, a whole tile of one destination, and a row of 1 edge in the next
    # tile; for the destination sum a segment of 17 rows and the root's (and relation 0's, if any): four unrolled trips and a tail
    assert rows == list(range(16 * int(want.tile_ptr[1]), 16 * int(want.tile_ptr[1]) + 17))
    assert want.row_cnt[rows].tolist() == [256] * 16 + [1] and int(want.dst_ptr[4] - want.dst_ptr[3]) in (18, 19)
    _layer(din, dout, ei, et, NS, ND, NREL, aggr, "run of 4,097")


EMPTY = (0, 255, 256, 511, 512, 599)


def test_six_hundred_relations():
    """601 relations with the root: mb_rel_scan_kernel takes three trips of 256 with rows in each; the relations at the edges of
    the trips are empty, so ``tile_ptr`` has runs of equal entries there for the transform's tile search to step over"""
    n_src, n_dst, r = 700, 300, 600
    g = torch.Generator().manual_seed(33)
    allowed = torch.tensor([i for i in range(r) if i not in EMPTY])
    et = allowed[torch.randint(0, allowed.numel(), (3000,), generator=g)]
    et[0], et[1] = 1, 598
    ei = torch.stack([torch.randint(0, n_src, (3000,), generator=g), torch.randint(0, n_dst, (3000,), generator=g)])
    used = torch.bincount(et, minlength=r)
    assert not bool(used[list(EMPTY)].any()) and bool(used[1]) and bool(used[598])
    assert all(bool(used[lo:hi].any()) for lo, hi in ((0, 256), (256, 512), (512, 600)))
    got = _layer(16, 13, ei, et, n_src, n_dst, r, "mean", "600 relations")
    assert not bool(got["weight"][list(EMPTY)].any()), "d_weight of the empty relations"
