"""The device-built index of a sampled block (rgcn_mb_index_build through sampling.block_index) against its CPU statement
(tests/block_index_reference.py): every array ``torch.equal``, on the reference's own cases, a block made by ``NeighborSampler``,
the same block with its edges permuted (the index sorts them itself), 300 relations with most of them empty, and the reference's
``edge_cases``: M = E_b + n_dst on both sides of a 2,048-key sort segment / scan block and of a four-segment sort workgroup, n_dst
and R at powers of two (one more key bit for the root relation and for the destination sort's dead key), three and four passes
of the first sort, a third pass of the source and of the destination sort, up to 513 and 65,537 relations through the relation
scan's trips of 256, and runs of exactly 1, 512, 513 and 4,097 edges."""
import pytest
import torch

from tests import block_index_reference as X
from tests import sampling_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = X.cases()
EDGE = X.edge_cases()


def _same(block, r, aggr="mean"):
    from scaling_rgcn_training_amd.sampling import Block, block_index
    ei, et, n_src, n_dst = block[:4]
    got = block_index(Block(ei.to(DEV), et.to(DEV), n_src, n_dst, None), r, aggr)
    want = X.build(ei.cpu(), et.cpu(), n_src, n_dst, r, aggr)
    torch.cuda.synchronize()
    assert (got.n_rows, got.n_tiles, got.n_src, got.n_dst, got.num_edges) == (want.n_rows, want.n_tiles, n_src, n_dst, int(et.numel()))
    for name in X.ARRAYS:
        g, w = getattr(got, name).cpu(), getattr(want, name)
        assert g.dtype == w.dtype and torch.equal(g, w), name
    return got


@pytest.mark.parametrize("aggr", ["mean", "sum"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_index_equals_the_reference(name, aggr):
    ei, et, n_src, n_dst, r = CASES[name]
    _same((ei, et, n_src, n_dst), r, aggr)


@pytest.mark.parametrize("aggr", ["mean", "sum"])
@pytest.mark.parametrize("name", sorted(EDGE))
def test_index_equals_the_reference_at_the_edges(name, aggr):
    ei, et, n_src, n_dst, r = EDGE[name]      # (the arithmetic that puts each block on its boundary: X.edge_cases)
    got = _same((ei, et, n_src, n_dst), r, aggr)
    if name.startswith("m"):
        assert got.num_edges + got.n_dst == int(name[1:])
    if name == "runs_1_512_513_4097":         # relation 1: rows (1), (256, 256), (256, 256, 1), 16 x (256) + (1), in that order
        t = got.tile_ptr.tolist()
        assert got.row_cnt[16 * t[1]:16 * t[2]].tolist() == [1, 256, 256, 256, 256, 1] + [256] * 16 + [1] + [0] * 9


def test_sampled_block_and_its_permutation():
    from scaling_rgcn_training_amd.sampling import NeighborSampler
    n, e, r = 2000, 20000, 5
    ei, et = R.hub_graph(n, e, r, seed=9, hub_edges=1400)
    sampler = NeighborSampler(ei.to(DEV), et.to(DEV), n, r)
    g = torch.Generator().manual_seed(1)
    seeds = torch.cat([torch.tensor([0]), 1 + torch.randperm(n - 1, generator=g)[:63]])
    blocks = sampler.sample(seeds.to(DEV), (5, -1), 2)
    for b in blocks:
        _same((b.edge_index, b.edge_type, b.n_src, b.n_dst), r)
        perm = torch.randperm(int(b.edge_type.numel()), generator=g).to(DEV)
        _same((b.edge_index[:, perm], b.edge_type[perm], b.n_src, b.n_dst), r)
    # the hub's run of more than 256 edges is there: the case is not vacuous
    b1 = blocks[1]
    key = b1.edge_index[1] * r + b1.edge_type
    assert int(torch.bincount(key).max()) > X.ROW_EDGES


def test_strided_rows_and_bad_ids():
    from scaling_rgcn_training_amd.sampling import Block, block_index
    ei, et, n_src, n_dst, r = CASES["square"]
    t = torch.stack([ei[0], ei[1], et], 1).to(DEV)              # [E, 3]: its columns are strided views
    got = block_index(Block(t[:, :2].t(), t[:, 2], n_src, n_dst, None), r)
    want = X.build(ei, et, n_src, n_dst, r)
    for name in X.ARRAYS:
        assert torch.equal(getattr(got, name).cpu(), getattr(want, name)), name
    for row, val in ((0, n_src), (1, n_dst), (1, -1), (2, r), (2, -2)):
        bad = torch.stack([ei[0], ei[1], et]).clone()
        bad[row, 7] = val
        with pytest.raises(ValueError):
            block_index(Block(bad[:2].to(DEV), bad[2].to(DEV), n_src, n_dst, None), r)
