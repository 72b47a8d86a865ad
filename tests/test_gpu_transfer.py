"""``rgcn_tr_block_labels`` / ``rgcn_tr_gather`` (csrc/rgcn_transfer.hip) and ``transfer.summary_labels`` /
``TransferredEmbedding`` against the numpy twin of tests/transfer_reference.py, BIT FOR BIT: the labels are integer sums and one
correctly rounded quotient, the gather moves table rows, computes draws in integers and adds in a fixed order -- nothing here has
a tolerance.  Shapes are the smallest that reach every path: widths 1 and 3 (element path), 4 (one 16-byte piece), 63 (element
path with a tail), 64 (16 lanes per row), 100 (25 lanes, two rows per wave), 260 (65 pieces: a second pass), 600 nodes (more than
one workgroup at every width)."""
import os

import numpy as np
import pytest
import torch

from tests import transfer_reference as R
from tests.conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TEST_NT = os.path.join(GOLDEN_DIR, "TEST", "TEST_complete.nt")
WIDTHS = (1, 3, 4, 63, 64, 100, 260)
N = 600


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what=""):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), (what, int((g != w).sum()), "elements differ")


# ---- labels --------------------------------------------------------------------------------------------------------------------
def _label_case(name):
    """(block, num_blocks, train_idx, y) as numpy int64"""
    g = np.random.default_rng(3)
    if name == "one-node":
        return np.zeros(1, np.int64), 1, np.zeros(1, np.int64), np.array([[1, 0, 2]], np.int64)
    if name in ("empty-blocks-c1", "empty-blocks-c4", "empty-blocks-c7"):
        c = int(name[-1])
        ids = np.array([b for b in range(37) if b not in (0, 17, 36)])            # three blocks without a node
        block = ids[g.integers(0, len(ids), 1000)]
        idx = g.permutation(1000)[:300]
        return block, 37, idx, (g.random((300, c)) < 0.4).astype(np.int64)
    if name == "no-training-rows":
        return g.integers(0, 37, 1000), 37, np.zeros(0, np.int64), np.zeros((0, 4), np.int64)
    if name == "labelled-in-one-block":
        block = g.integers(0, 37, 1000)
        idx = np.nonzero(block == 5)[0]
        return block, 37, idx, (g.random((len(idx), 4)) < 0.5).astype(np.int64)
    if name == "one-block-5000":
        idx = g.permutation(5000)[:700]
        return np.zeros(5000, np.int64), 1, idx, (g.random((700, 4)) < 0.3).astype(np.int64)
    if name == "few-blocks-interleaved":                                          # more distinct ids per wave than are combined
        return g.integers(0, 12, 3000), 12, g.permutation(3000)[:500], (g.random((500, 4)) < 0.3).astype(np.int64)
    if name == "sorted-blocks":              # whole chunks of one id, the id changing inside a wave's range and inside a chunk
        block = np.sort(np.concatenate([g.integers(0, 12, 2900), np.full(1500, 5)]))
        return block, 12, g.permutation(4400)[:500], (g.random((500, 4)) < 0.3).astype(np.int64)
    assert name == "counts-above-one"
    return g.integers(0, 37, 1000), 37, g.permutation(1000)[:400], g.integers(0, 5, (400, 7))


LABEL_CASES = ("one-node", "empty-blocks-c1", "empty-blocks-c4", "empty-blocks-c7", "no-training-rows", "labelled-in-one-block",
               "one-block-5000", "few-blocks-interleaved", "sorted-blocks", "counts-above-one")


@pytest.mark.parametrize("name", LABEL_CASES)
def test_block_labels_equal_the_twin(name):
    from scaling_rgcn_training_amd import _lib, transfer as T
    block, nb, idx, y = _label_case(name)
    size_w, ysum_w, nz_w = R.block_labels(block, nb, idx, y)
    tb, ti, ty = (torch.from_numpy(a).to(DEV) for a in (block, idx, y))
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    size, y_sum, nonzero = _lib.tr_block_labels(tb, nb, ti, ty, bad)
    assert size.dtype == torch.int32 and np.array_equal(size.cpu().numpy(), size_w)
    assert np.array_equal(nonzero.cpu().numpy(), nz_w)
    _same(y_sum, ysum_w, name)
    assert int(bad.item()) == 0
    x, ys, size2 = T.summary_labels(tb, nb, ti, ty)
    xw, yw, _ = R.summary_labels(block, nb, idx, y)
    assert x.dtype == torch.int64 and np.array_equal(x.cpu().numpy(), xw) and torch.equal(size2, size)
    assert ys.shape == (len(xw), y.shape[1])
    _same(ys, yw, name)
    if name.startswith("empty-blocks"):
        assert size_w[[0, 17, 36]].tolist() == [0, 0, 0] and not ysum_w[[0, 17, 36]].any()
    if name == "one-block-5000":
        assert size_w.tolist() == [5000]


def test_labels_equal_dataset_add_summary_on_the_golden_graph():
    from scaling_rgcn_training_amd import graphs as G, transfer as T
    from scaling_rgcn_training_amd.summaries import Partition
    data = G.Dataset(TEST_NT)
    data.init_dataset()
    td = data.orgGraph.training_data
    for ids in ([0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2], [0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3], list(range(12))):
        block, nb = torch.tensor(ids), max(ids) + 1
        sg = data.add_summary(partition=Partition(block, nb, 1, (nb,), False))
        x, y, size = T.summary_labels(block.to(DEV), nb, td.x_train.to(DEV), td.y_train.to(DEV))
        assert torch.equal(x.cpu(), sg.training_data.x_train)
        _same(y, sg.training_data.y_train)
        assert size.tolist() == np.bincount(ids, minlength=nb).tolist()


def test_labels_with_ids_out_of_range():
    from scaling_rgcn_training_amd import _lib, transfer as T
    block, nb, idx, y = _label_case("empty-blocks-c4")
    good = R.block_labels(block, nb, idx, y)
    for what, bit in (("block", _lib.TR_BAD_BLOCK), ("train", _lib.TR_BAD_NODE), ("both", _lib.TR_BAD_BLOCK | _lib.TR_BAD_NODE)):
        b2, i2 = block.copy(), idx.copy()
        free = np.setdiff1d(np.arange(1000), idx)              # nodes without a label: their loss changes a size, no label
        if what in ("block", "both"):
            b2[free[0]], b2[free[1]], b2[free[2]] = -1, nb, 2 ** 40
        if what in ("train", "both"):
            i2[7], i2[8], i2[9] = -5, 1000, 2 ** 33
        want = R.block_labels(b2, nb, i2, y)
        tb, ti, ty = (torch.from_numpy(a).to(DEV) for a in (b2, i2, y))
        bad = torch.zeros(1, dtype=torch.int32, device=DEV)
        size, y_sum, nonzero = _lib.tr_block_labels(tb, nb, ti, ty, bad)
        assert int(bad.item()) == bit
        assert np.array_equal(size.cpu().numpy(), want[0]) and np.array_equal(nonzero.cpu().numpy(), want[2])
        _same(y_sum, want[1], what)
        if what == "train":                                    # the rows of the good training nodes are what they were
            touched = np.unique(block[idx[[7, 8, 9]]])
            keep = np.setdiff1d(np.arange(nb), touched)
            _same(y_sum[torch.from_numpy(keep).to(DEV)], good[1][keep], what)
        with pytest.raises(IndexError):
            T.summary_labels(tb, nb, ti, ty)


# ---- gather --------------------------------------------------------------------------------------------------------------------
def _tables(s, e, layout="plain", seed=0):
    """S device tables of 37 + s rows: plain, a row-strided view (ld = e + 4 or e + 1), or a base 4 bytes off 16-byte alignment"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(s):
        t = torch.randn(37 + i, e, generator=g)
        if layout == "plain":
            d = t.to(DEV)
        elif layout in ("padded", "odd"):
            ld = e + (4 if layout == "padded" else 1)
            d = torch.full((37 + i, ld), 777.0, device=DEV)[:, :e]
            d.copy_(t)
        else:
            buf = torch.full(((37 + i) * e + 1,), 777.0, device=DEV)
            d = buf[1:].view(37 + i, e)
            d.copy_(t)
            assert d.data_ptr() % 16 == 4
        out.append(d)
    return out


def _maps(s, n, unmapped, seed=1):
    g = np.random.default_rng(seed)
    maps = []
    for i in range(s):
        m = g.integers(0, 37 + i, n)
        if unmapped == "some":
            m[g.random(n) < 0.3] = -1
        elif unmapped == "all":
            m[:] = -1
        maps.append(m.astype(np.int64))
    return maps


def _node_lists(n):
    g = np.random.default_rng(2)
    return {"all": None, "repeats": np.concatenate([g.integers(0, n, n // 2), [n - 1, 0, 0, n - 1]]).astype(np.int64),
            "empty": np.zeros(0, np.int64)}


def _check_all_modes(tables, maps, nodes_np, seed, what):
    from scaling_rgcn_training_amd import transfer as T
    n = maps[0].shape[0]
    host_tables = [t.cpu().numpy() for t in tables]
    ps = R.pieces(host_tables, maps, n, nodes_np, seed)
    dmaps = [torch.from_numpy(m).to(DEV) for m in maps]
    nodes = None if nodes_np is None else torch.from_numpy(nodes_np).to(DEV)
    for mode in R.MODES:
        te = T.TransferredEmbedding(tables, dmaps, n, mode, seed)
        got = te.materialize() if nodes is None else te.rows(nodes)
        _same(got, R.combine(ps, mode), (what, mode))
        te.check()
    return ps


@pytest.mark.parametrize("e", WIDTHS)
@pytest.mark.parametrize("s", (1, 3, 16))
def test_gather_equals_the_twin(s, e):
    tables = _tables(s, e)
    for unmapped in ("none", "some", "all"):
        maps = _maps(s, N, unmapped)
        for name, nodes in _node_lists(N).items():
            ps = _check_all_modes(tables, maps, nodes, 11, (s, e, unmapped, name))
            if unmapped == "none" and nodes is not None and len(nodes):       # mapped pieces are index_select
                for i in range(s):
                    want = tables[i].index_select(0, torch.from_numpy(maps[i][nodes]).to(DEV))
                    _same(want, ps[i])


@pytest.mark.parametrize("layout", ("padded", "odd", "offset"))
@pytest.mark.parametrize("e", WIDTHS)
def test_gather_from_strided_and_misaligned_tables(e, layout):
    tables = _tables(3, e, layout)
    maps = _maps(3, N, "some")
    for name, nodes in _node_lists(N).items():
        _check_all_modes(tables, maps, nodes, 5, (e, layout, name))


@pytest.mark.parametrize("mode", R.MODES)
def test_rows_equal_materialize_and_sum_is_left_to_right(mode):
    from scaling_rgcn_training_amd import transfer as T
    tables, maps = _tables(3, 64), _maps(3, N, "some")
    dmaps = [torch.from_numpy(m).to(DEV) for m in maps]
    te = T.TransferredEmbedding(tables, dmaps, N, mode, seed=4)
    full = te.materialize()
    nodes = torch.from_numpy(_node_lists(N)["repeats"]).to(DEV)
    part = te.rows(nodes)
    assert torch.equal(part, full[:, nodes] if mode == "stack" else full[nodes])
    # the draw does not depend on the mode, and SUM is the left-to-right torch sum of the planes
    stack = T.TransferredEmbedding(tables, dmaps, N, "stack", seed=4).materialize()
    want = {"stack": stack, "concat": torch.cat(list(stack), dim=-1), "sum": sum(list(stack))}[mode]
    assert torch.equal(full, want)
    other = T.TransferredEmbedding(tables, dmaps, N, mode, seed=5).materialize()
    mapped = torch.from_numpy(np.stack(maps) >= 0).to(DEV)
    if mode == "stack":
        assert torch.equal(other[mapped], full[mapped]) and not torch.equal(other, full)      # the seed moves the fills alone
    te.check()


def test_tricks_equal_the_string_keyed_ones():
    """all nodes mapped: transfer.* on a string-keyed graph (its map comes from graphs.transfer_index), and on the same summaries
    with org_block, equal graphs.* exactly"""
    from scaling_rgcn_training_amd import graphs as G, transfer as T
    from scaling_rgcn_training_amd.summaries import Partition
    data = G.Dataset(TEST_NT)
    data.init_dataset()
    g = torch.Generator().manual_seed(0)
    for ids in ([0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2], [0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3], list(range(12))):
        nb = max(ids) + 1
        sg = data.add_summary(partition=Partition(torch.tensor(ids), nb, 1, (nb,), False))
        sg.embedding = torch.randn(nb, 20, generator=g)
    org = data.orgGraph
    pairs = ((T.stack_embeddings, G.stack_embeddings), (T.concat_embeddings, G.concat_embeddings), (T.sum_embeddings, G.sum_embeddings))
    for ours, theirs in pairs:
        want = theirs(org, data.sumGraphs, 20)
        got = ours(org, data.sumGraphs, 20)
        assert got.device.type == "cuda"
        _same(got, want, ours.__name__)
    for sg in data.sumGraphs:                                  # the tensor form of the same maps, tables already on the GPU
        sg.org_block = G.transfer_index(org, sg).to(DEV)
        sg.embedding = sg.embedding.to(DEV)
        sg.orgNode2sumNode_dict = None
    for ours, theirs in pairs:
        got = ours(org, data.sumGraphs, 20)
        ref = torch.stack([sg.embedding[sg.org_block] for sg in data.sumGraphs])
        want = {"stack_embeddings": ref, "concat_embeddings": torch.cat(list(ref), -1), "sum_embeddings": sum(list(ref))}[ours.__name__]
        assert torch.equal(got, want)


def test_gather_with_ids_out_of_range():
    from scaling_rgcn_training_amd import _lib, transfer as T
    tables, maps = _tables(3, 64), _maps(3, N, "some")
    nodes = _node_lists(N)["repeats"].copy()
    clean = R.pieces([t.cpu().numpy() for t in tables], maps, N, nodes, 9)
    maps[1][nodes[3]], maps[2][nodes[5]] = -2, 37 + 2                 # one below -1, one just past its table
    nodes[10], nodes[11], nodes[12] = -1, N, 2 ** 35
    want = R.pieces([t.cpu().numpy() for t in tables], maps, N, nodes, 9)
    assert not want[1][3].any() and not want[2][5].any() and not want[0][10].any() and not want[2][12].any()
    hit = np.isin(nodes, [nodes[3], nodes[5]]) | (np.arange(len(nodes)) >= 10) & (np.arange(len(nodes)) <= 12)
    assert all(np.array_equal(w[~hit], c[~hit]) for w, c in zip(want, clean))      # the other pieces are what they were
    dmaps = [torch.from_numpy(m).to(DEV) for m in maps]
    for mode in R.MODES:
        te = T.TransferredEmbedding(tables, dmaps, N, mode, seed=9)
        _same(te.rows(torch.from_numpy(nodes).to(DEV)), R.combine(want, mode), mode)
        assert int(te._bad.item()) == _lib.TR_BAD_NODE | _lib.TR_BAD_MAP
        with pytest.raises(IndexError):
            te.check()
        te.check()                                                        # the word was cleared
        _same(te.materialize(), R.gather([t.cpu().numpy() for t in tables], maps, N, None, mode, 9), mode)
        assert int(te._bad.item()) == _lib.TR_BAD_MAP
        with pytest.raises(IndexError):
            te.check()


def test_gather_past_4_gib():
    """CONCAT of two 64-wide tables over 2^23 + 5 nodes is 4 GiB + 2,560 bytes: the last five rows lie past 2^32 bytes, so a row
    offset computed in 32 bits would wrap onto the first rows"""
    from scaling_rgcn_training_amd import transfer as T
    n = 2 ** 23 + 5
    g = torch.Generator(device=DEV).manual_seed(0)
    tables = [torch.randn(1000, 64, device=DEV, generator=g) for _ in range(2)]
    maps = [torch.randint(0, 1000, (n,), device=DEV, generator=g) for _ in range(2)]
    loose = torch.tensor([0, 1, 4097, 2 ** 22, 2 ** 23 - 1, 2 ** 23, 2 ** 23 + 2, n - 1], device=DEV)
    maps[0][loose] = -1
    maps[1][loose[::2]] = -1
    te = T.TransferredEmbedding(tables, maps, n, "concat", seed=3)
    out = te.materialize()
    assert out.shape == (n, 128) and out.numel() * 4 > 2 ** 32
    te.check()
    for lo in range(0, n, 2 ** 21):
        hi = min(n, lo + 2 ** 21)
        want = torch.cat([t[m[lo:hi].clamp(min=0)] for t, m in zip(tables, maps)], dim=1)
        keep = torch.stack([m[lo:hi] >= 0 for m in maps], 1).repeat_interleave(64, dim=1)
        assert torch.equal(torch.where(keep, out[lo:hi], want), want), lo
    host_maps = [m[loose].cpu().numpy() for m in maps]
    idx = loose.cpu().numpy()
    for s in range(2):
        fill = R.draw(3, s, idx, 64)
        got = out[loose, 64 * s:64 * (s + 1)].cpu().numpy()
        rows = host_maps[s] == -1
        assert rows.any() and np.array_equal(got[rows].view(np.uint32), fill[rows].view(np.uint32))
    _same(te.rows(loose), out[loose])


def test_gather_replays_from_a_captured_graph():
    from scaling_rgcn_training_amd import transfer as T
    tables, maps = _tables(3, 64), _maps(3, N, "some")
    dmaps = [torch.from_numpy(m).to(DEV) for m in maps]
    nodes = torch.from_numpy(_node_lists(N)["repeats"]).to(DEV)
    te = T.TransferredEmbedding(tables, dmaps, N, "stack", seed=2)
    eager_full, eager_rows = te.materialize(), te.rows(nodes)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        te.rows(nodes)                                                    # warm-up
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            full, rows = te.materialize(), te.rows(nodes)
    torch.cuda.current_stream(DEV).wait_stream(side)
    for _ in range(2):
        full.fill_(-1.0)
        rows.fill_(-1.0)
        graph.replay()
        assert torch.equal(full, eager_full) and torch.equal(rows, eager_rows)
    te.check()
