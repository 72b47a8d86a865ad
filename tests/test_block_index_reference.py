"""The CPU statement of a block's index (tests/block_index_reference.py) against a brute-force layer: walking the reference index
in float64 reproduces ``pyg_bipartite_loop``'s output and autograd gradients to 1e-12, and the index has the shape DESIGN.md 15
gives it -- on duplicates, a run of 600, runs of exactly 256 and 257, relations with 0 / 16 / 17 rows, isolated destinations, a
block without edges, one without destinations and one whose sources are its destinations; the same for the blocks of
``edge_cases`` (the device build's size, bit-width and pass-count boundaries), so that the enlarged reference is itself checked
without a GPU -- the one with 65,536 relations structurally (the brute-force layer loops over the relations)."""
import pytest
import torch

from tests import block_index_reference as X
from tests.bipartite_reference import pyg_bipartite_loop

CASES = X.cases()
EDGE = X.edge_cases()


def _layer(n_src, r, din, dout, seed, grid=None):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    if grid:      # multiples of 1 / grid: sums and products of a few thousand of them are exact in float64, whatever their order
        rnd = lambda *s: torch.round(torch.randn(*s, generator=g, dtype=torch.float64) * grid) / grid
    return rnd(n_src, din), rnd(r, din, dout), rnd(din, dout), rnd(dout)


@pytest.mark.parametrize("aggr", ["mean", "sum"])
@pytest.mark.parametrize("name", sorted(CASES) + sorted(k for k in EDGE if EDGE[k][4] <= 600))
def test_walking_the_index_is_the_layer(name, aggr):
    """The blocks of ``edge_cases`` take inputs on a grid of 1 / 64.  A sum over a run of 4,097 random float64 values near 1, or a
    d_root over 66,000 rows, comes out 3e-12 to 6e-12 apart between two orders of adding (measured: |value| up to 980), which says
    nothing about the index; on the grid every sum of a sum-aggregated layer is exact (9 bits a value, 4,097 terms, a second 9-bit
    factor, 66,000 rows: 47 bits), so there the two must agree to the bit, and a mean adds only the rounding of its 1 / run length."""
    edge = name not in CASES
    ei, et, n_src, n_dst, r = EDGE[name] if edge else CASES[name]
    r_used = min(r, 8) if name != "many_rel" else r
    assert not edge or (int(et.max()) < r and int(ei[0].max()) == n_src - 1 and int(ei[1].max()) == n_dst - 1)
    x, w, root, bias = _layer(n_src, r, 3, 2, 5, grid=64 if edge else None)
    g = torch.randn(n_dst, 2, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    if edge:
        g = torch.round(g * 64) / 64
    ix = X.build(ei, et, n_src, n_dst, r, aggr)
    out, grads = X.walk(ix, x, w, root, bias, g)
    leaves = [t.clone().requires_grad_(True) for t in (x, w, root, bias)]
    ref = pyg_bipartite_loop(leaves[0], leaves[0][:n_dst], ei, et, leaves[1], leaves[2], leaves[3], aggr)
    ref.backward(g)
    atol = 0.0 if edge and aggr == "sum" else 1e-12
    assert r_used and tuple(out.shape) == (n_dst, 2)
    assert torch.allclose(out, ref.detach(), rtol=0, atol=atol)
    for k, leaf in zip(("x", "weight", "root", "bias"), leaves):
        want = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
        assert torch.allclose(grads[k], want, rtol=0, atol=atol), (name, aggr, k)


def test_rows_tiles_and_lists():
    ei, et, n_src, n_dst, r = CASES["runs"]
    ix = X.build(ei, et, n_src, n_dst, r)
    cnt, dst, tp = ix.row_cnt.tolist(), ix.row_dst.tolist(), ix.tile_ptr.tolist()
    assert max(cnt) == X.ROW_EDGES and len(tp) == r + 2 and tp[-1] == ix.n_tiles and sum(c > 0 for c in cnt) == ix.n_rows
    rel0 = [(dst[s], cnt[s]) for s in range(16 * tp[0], 16 * tp[1]) if cnt[s]]
    assert rel0[:4] == [(0, 256), (0, 256), (0, 88), (1, 256)]          # the run of 600 is three rows, the run of 256 one
    rel1 = [(dst[s], cnt[s]) for s in range(16 * tp[1], 16 * tp[2]) if cnt[s]]
    assert (2, 256) in rel1 and (2, 1) in rel1                           # the run of 257: a row of 256 and a row of 1
    assert float(ix.row_scale[16 * tp[0]]) == float(torch.tensor(1.0, dtype=torch.float32) / 600)
    assert ix.dst_ptr.tolist()[-1] == ix.n_rows and ix.src_ptr.tolist()[-1] == et.numel() + n_dst
    # the root relation: one row of one pseudo edge i -> i per destination, isolated destinations included
    root = [(dst[s], cnt[s], int(ix.edge_src[ix.row_beg[s]])) for s in range(16 * tp[r], 16 * tp[r + 1]) if cnt[s]]
    assert root == [(i, 1, i) for i in range(n_dst)]
    # a destination's rows ascend by relation; a source's positions ascend
    for i in range(n_dst):
        rows = ix.dst_rows.tolist()[ix.dst_ptr[i]:ix.dst_ptr[i + 1]]
        assert rows == sorted(rows) and all(dst[s] == i for s in rows)
    ei2, et2, ns2, nd2, r2 = CASES["rel_rows"]
    tp2 = X.build(ei2, et2, ns2, nd2, r2).tile_ptr.tolist()
    assert tp2 == [0, 0, 1, 3, 3, 5]                                     # 0, 16, 17, 0 rows and the root's 20
    empty = X.build(*CASES["no_dst"])
    assert empty.n_tiles == 0 and empty.n_rows == 0 and empty.tile_ptr.tolist() == [0] * 4 and empty.src_ptr.tolist() == [0] * 5
    lone = X.build(*CASES["no_edges"])
    assert lone.n_rows == 5 and lone.n_tiles == 1 and lone.tile_ptr.tolist() == [0, 0, 0, 0, 1]


@pytest.mark.parametrize("aggr", ["mean", "sum"])
def test_structure_at_65536_relations(aggr):
    ei, et, n_src, n_dst, r = EDGE["rel65536"]
    ix = X.build(ei, et, n_src, n_dst, r, aggr)
    m = int(et.numel()) + n_dst
    # tile_ptr: the tiles of the rows per relation, counted here from the (relation, destination) runs directly
    key = torch.cat([et * n_dst + ei[1], r * n_dst + torch.arange(n_dst)])
    runs, lens = torch.unique(key, return_counts=True)
    rows = torch.zeros(r + 1, dtype=torch.int64).index_add_(0, runs // n_dst, (lens + X.ROW_EDGES - 1) // X.ROW_EDGES)
    assert sorted(torch.nonzero(rows)[:, 0].tolist()) == [0, 1, 65534, 65535, 65536]
    assert ix.n_rows == int(rows.sum()) and int((ix.row_cnt > 0).sum()) == ix.n_rows
    want = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum((rows + 15) // 16, 0)])
    assert torch.equal(ix.tile_ptr.long(), want) and ix.n_tiles == int(want[-1]) and ix.row_cnt.numel() == 16 * ix.n_tiles
    # every position lies in exactly one row, and the row is of the position's relation and destination
    live = ix.row_cnt > 0
    beg, cnt = ix.row_beg.long()[live], ix.row_cnt.long()[live]
    pos = torch.repeat_interleave(beg - torch.cumsum(cnt, 0) + cnt, cnt) + torch.arange(int(cnt.sum()))
    assert int(cnt.sum()) == m and int(cnt.max()) == X.ROW_EDGES and torch.equal(torch.sort(pos).values, torch.arange(m))
    slot_rel = torch.repeat_interleave(torch.arange(r + 1), 16 * (ix.tile_ptr[1:] - ix.tile_ptr[:-1]).long())[live]
    skey = torch.sort(key, stable=True).values
    assert torch.equal(skey[pos], torch.repeat_interleave(slot_rel * n_dst + ix.row_dst.long()[live], cnt))
    assert ix.dst_ptr.tolist()[-1] == ix.n_rows and ix.src_ptr.tolist()[-1] == m
    hub = float(ix.row_scale[0])            # (relation 0, destination 0): the hub's run of more than 600 edges
    assert hub == (float(torch.tensor(1.0) / int(lens[0])) if aggr == "mean" else 1.0) and int(lens[0]) > 600
