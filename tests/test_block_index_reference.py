"""The CPU statement of a block's index (tests/block_index_reference.py) against a brute-force layer: walking the reference index
in float64 reproduces ``pyg_bipartite_loop``'s output and autograd gradients to 1e-12, and the index has the shape DESIGN.md 15
gives it -- on duplicates, a run of 600, runs of exactly 256 and 257, relations with 0 / 16 / 17 rows, isolated destinations, a
block without edges, one without destinations and one whose sources are its destinations."""
import pytest
import torch

from tests import block_index_reference as X
from tests.bipartite_reference import pyg_bipartite_loop

CASES = X.cases()


def _layer(n_src, r, din, dout, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return rnd(n_src, din), rnd(r, din, dout), rnd(din, dout), rnd(dout)


@pytest.mark.parametrize("aggr", ["mean", "sum"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_walking_the_index_is_the_layer(name, aggr):
    ei, et, n_src, n_dst, r = CASES[name]
    r_used = min(r, 8) if name != "many_rel" else r
    x, w, root, bias = _layer(n_src, r, 3, 2, 5)
    g = torch.randn(n_dst, 2, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    ix = X.build(ei, et, n_src, n_dst, r, aggr)
    out, grads = X.walk(ix, x, w, root, bias, g)
    leaves = [t.clone().requires_grad_(True) for t in (x, w, root, bias)]
    ref = pyg_bipartite_loop(leaves[0], leaves[0][:n_dst], ei, et, leaves[1], leaves[2], leaves[3], aggr)
    ref.backward(g)
    assert r_used and tuple(out.shape) == (n_dst, 2)
    assert torch.allclose(out, ref.detach(), rtol=0, atol=1e-12)
    for k, leaf in zip(("x", "weight", "root", "bias"), leaves):
        want = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
        assert torch.allclose(grads[k], want, rtol=0, atol=1e-12), (name, aggr, k)


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
