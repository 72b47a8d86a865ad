"""The host side of the summary -> original pipeline on tensors (scaling_rgcn_training_amd/transfer.py, tensor_data.py, the
argument checks of csrc/rgcn_transfer.hip) and the numpy twin the GPU tests compare against (tests/transfer_reference.py):
everything here is answered before a kernel is launched, so it runs without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from scaling_rgcn_training_amd import _lib
from scaling_rgcn_training_amd import graphs as G
from scaling_rgcn_training_amd import tensor_data as D
from scaling_rgcn_training_amd import transfer as T
from scaling_rgcn_training_amd.summaries import Partition
from tests import transfer_reference as R
from tests.conftest import GOLDEN_DIR

TEST_NT = os.path.join(GOLDEN_DIR, "TEST", "TEST_complete.nt")
NULL, STRIDE, PLAN, WS, ARG = -1, -3, -4, -6, -11
_BUF = (ctypes.c_float * 1024)()


def _p():
    a = ctypes.addressof(_BUF)
    return a + (-a % 16)            # a 16-byte aligned host address the checks see as non-NULL and never read


# ---- the twin's labels are make_training_data's -----------------------------------------------------------------------------------
def test_twin_labels_equal_make_training_data():
    data = G.Dataset(TEST_NT)
    data.init_dataset()
    org, td = data.orgGraph, data.orgGraph.training_data
    n = org.num_nodes
    assert n == 12 and td.x_train.tolist() == [6] and td.x_val.tolist() == [7] and td.x_test.tolist() == [5]
    hand = ([0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2],       # block 1: the training node, both held-out nodes, two unlabelled ones
            [0, 1, 0, 1, 0, 2, 2, 2, 1, 0, 3, 3],       # block 2: the three labelled nodes alone
            [0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3],       # block 2: the training node and unlabelled ones; block 1 / 3: held-out ones
            list(range(n)))                             # every node its own block
    for ids in hand:
        block, nb = torch.tensor(ids), max(ids) + 1
        if nb == 3:                          # a block that mixes training, held-out and unlabelled nodes
            held, train = set(td.x_val.tolist()) | set(td.x_test.tolist()), set(td.x_train.tolist())
            kinds = {"train" if i in train else "held" if i in held else "none" for i, b in enumerate(ids) if b == 1}
            assert len(kinds) == 3
        data.sumGraphs = [G.summary_graph(org, Partition(block, nb, 1, (nb,), False), f"hand{nb}")]
        data.make_training_data()
        std = data.sumGraphs[0].training_data
        x, y, size = R.summary_labels(block.numpy(), nb, td.x_train.numpy(), td.y_train.numpy())
        assert np.array_equal(x, std.x_train.numpy())
        assert y.dtype == np.float32 and std.y_train.dtype == torch.float32
        assert np.array_equal(y.view(np.uint32), std.y_train.numpy().view(np.uint32))
        assert np.array_equal(size, np.bincount(block.numpy(), minlength=nb))
        assert len(x) > 0 and (nb == n or np.any((y > 0) & (y < 1)))      # fractions, not only 0 / 1


def test_twin_labels_edge_cases():
    block = np.array([0, 0, 2, 2, 2, 5], dtype=np.int64)                  # blocks 1, 3, 4 are empty
    y = np.array([[3, 0], [0, 0], [1, 2]], dtype=np.int64)
    size, y_sum, nonzero = R.block_labels(block, 6, np.array([0, 4, 2]), y)
    assert size.tolist() == [2, 0, 3, 0, 0, 1] and nonzero.tolist() == [1, 0, 1, 0, 0, 0]
    assert y_sum[0].tolist() == [1.5, 0.0] and y_sum[2].tolist() == [np.float32(1 / 3), np.float32(2 / 3)]
    assert np.all(y_sum[[1, 3, 4, 5]] == 0)
    # ids out of range are skipped, the other rows stay
    size2, y_sum2, _ = R.block_labels(np.array([0, 0, 2, 2, 2, 9]), 6, np.array([0, 4, 2, 77, -1]), np.vstack([y, y[:2]]))
    assert size2.tolist() == [2, 0, 3, 0, 0, 0] and np.array_equal(y_sum2, y_sum)
    size3, y_sum3, nz3 = R.block_labels(block, 6, np.zeros(0, dtype=np.int64), np.zeros((0, 2), dtype=np.int64))
    assert np.array_equal(size3, size) and not y_sum3.any() and not nz3.any()


# ---- the twin's draw --------------------------------------------------------------------------------------------------------------
def test_twin_draw_is_a_function_of_seed_table_node_and_column():
    nodes = np.array([0, 1, 5, 5, 2 ** 31 - 2, 123456789])
    base = R.draw(7, 2, nodes, 16)
    assert base.dtype == np.float32 and base.shape == (6, 16)
    assert np.all(base >= 0) and np.all(base < 1)
    assert np.array_equal(base[2], base[3])                                  # the same node twice: the same row
    assert len(np.unique(base[[0, 1, 2, 4, 5]])) == 5 * 16                   # it changes with node and column
    assert not np.array_equal(base, R.draw(8, 2, nodes, 16)) and not np.array_equal(base, R.draw(7, 3, nodes, 16))
    # nothing else: not the position in the list, not the list's length; the counter is node * width + column
    assert np.array_equal(R.draw(7, 2, nodes[::-1], 16)[::-1], base)
    assert np.array_equal(R.draw(7, 2, nodes[4:5], 16)[0], base[4])
    assert np.array_equal(R.draw(7, 2, np.array([0]), 32)[0, 16:], R.draw(7, 2, np.array([1]), 16)[0])
    # one value by hand, in Python integers
    m64 = (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m64
        return z ^ (z >> 31)

    key = mix((7 + 0x9E3779B97F4A7C15 * 3) & m64)
    want = (mix((key + 123456789 * 16 + 11) & m64) >> 40) * 2.0 ** -24
    assert float(base[5, 11]) == want
    # uniform enough: the mean of 64k draws
    big = R.draw(0, 0, np.arange(4096), 16)
    assert abs(float(big.mean()) - 0.5) < 0.01 and float(big.max()) > 0.999 and float(big.min()) < 0.001


def test_twin_gather_modes():
    g = np.random.default_rng(0)
    tables = [g.standard_normal((5, 3)).astype(np.float32) for _ in range(3)]
    maps = [np.array([0, -1, 4, 2]), np.array([-1, -1, 1, 9]), np.array([3, 3, -2, 0])]       # 9 and -2: out of range
    nodes = np.array([3, 0, 0, 7, 2])                                                           # 7: out of range
    ps = R.pieces(tables, maps, 4, nodes, 5)
    assert np.array_equal(ps[0][0], tables[0][2]) and np.array_equal(ps[0][1], tables[0][0]) and not ps[0][3].any()
    assert not ps[1][0].any() and not ps[2][4].any()                                            # bad map values: zeros
    assert np.array_equal(ps[1][1], R.draw(5, 1, [0], 3)[0]) and np.array_equal(ps[1][1], ps[1][2])
    st, cc, sm = (R.gather(tables, maps, 4, nodes, m, 5) for m in R.MODES)
    assert st.shape == (3, 5, 3) and cc.shape == (5, 9) and sm.shape == (5, 3)
    assert np.array_equal(cc, np.concatenate(list(st), 1)) and np.array_equal(sm, (st[0] + st[1]) + st[2])
    full = R.gather(tables, maps, 4, None, "stack", 5)
    assert np.array_equal(full[:, [3, 0, 0, 2]], st[:, [0, 1, 2, 4]])


# ---- the Python layer's refusals ----------------------------------------------------------------------------------------------------
def test_summary_labels_refusals():
    block, idx, y = torch.zeros(6, dtype=torch.int64), torch.tensor([0, 2]), torch.ones(2, 3, dtype=torch.int64)
    for args in ((block.int(), 2, idx, y), (block.reshape(2, 3), 2, idx, y), (block, 0, idx, y), (block, True, idx, y), (block, 2.0, idx, y),
                 (block, 2, idx.int(), y), (block, 2, idx, y.float()), (block, 2, idx, y[:1]), (block, 2, idx, y[:, :0]),
                 (block, 2, idx, y.reshape(-1)), (block.numpy(), 2, idx, y)):
        with pytest.raises(ValueError):
            T.summary_labels(*args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # a missing GPU is an error, never a torch formulation
        T.summary_labels(block, 2, idx, y)


def test_transferred_embedding_refusals():
    t, m = torch.zeros(4, 8), torch.zeros(10, dtype=torch.int64)
    ok = dict(tables=[t, t], maps=[m, m], num_nodes=10)
    for kw in (dict(mode="mean"), dict(tables=[t]), dict(tables=[], maps=[]), dict(tables=[t] * 17, maps=[m] * 17), dict(num_nodes=11),
               dict(num_nodes=-1), dict(num_nodes=True), dict(seed=-1), dict(seed=2 ** 63), dict(seed=1.0),
               dict(tables=[t, torch.zeros(4, 7)]), dict(tables=[t, t.double()]), dict(tables=[t, t[0]]), dict(tables=[t, torch.zeros(4, 0)]),
               dict(tables=[t, torch.zeros(8, 4).t()]), dict(tables=[t, t[:1].expand(4, 8)]), dict(maps=[m, m.int()]),
               dict(maps=[m, m.reshape(2, 5)]), dict(tables=t, maps=m), dict(tables=[t, t.numpy()])):
        args = dict(ok)
        args.update(kw)
        with pytest.raises(ValueError):
            T.TransferredEmbedding(**args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.TransferredEmbedding(**ok)
    assert T.TransferredEmbedding.__init__.__defaults__ == ("stack", 0)


class _Bag:
    pass


def test_embedding_tricks_refusals():
    org, sg = _Bag(), _Bag()
    org.num_nodes, sg.org_block, sg.embedding = 10, torch.zeros(10, dtype=torch.int64), None
    for trick in (T.stack_embeddings, T.concat_embeddings, T.sum_embeddings):
        with pytest.raises(ValueError, match="at least one"):
            trick(org, [], 8)
        with pytest.raises(ValueError, match="trained"):
            trick(org, [sg], 8)
    sg.embedding = torch.zeros(3, 4)
    with pytest.raises(ValueError, match="trained"):
        T.sum_embeddings(org, [sg], 8)


def test_tensor_dataset_refusals_and_layout():
    ei, et = torch.tensor([[0, 1, 2, 3], [1, 2, 3, 0]]), torch.tensor([0, 1, 2, 4])
    lab_idx = torch.tensor([0, 1, 2, 3, 4, 5, 6, 7, 8, 9])
    labels = torch.eye(3, dtype=torch.int64)[torch.arange(10) % 3]
    ok = dict(edge_index=ei, edge_type=et, num_nodes=12, num_relations=5, labelled_idx=lab_idx, labels=labels)
    pos = torch.arange(10)
    for kw in (dict(edge_index=ei.int()), dict(edge_type=et[:3]), dict(num_nodes=3), dict(num_relations=4), dict(num_nodes=0),
               dict(labelled_idx=lab_idx.int()), dict(labels=labels.float()), dict(labels=labels[:9]), dict(labels=labels[:, :0]),
               dict(labelled_idx=lab_idx + 3), dict(labelled_idx=lab_idx - 1), dict(labels=-labels), dict(seed=1.5),
               dict(split=(pos[:6], pos[6:8])), dict(split=(pos[:6], pos[6:8], pos[8:] + 1)), dict(split=(pos[:6], pos[6:8], pos[8:].int())),
               dict(split="60/20/20")):
        args = dict(ok)
        args.update(kw)
        with pytest.raises(ValueError):
            D.TensorDataset(**args)
    data = D.TensorDataset(**ok)
    org, td = data.orgGraph, data.orgGraph.training_data
    assert data.num_classes == 3 and data.sumGraphs == [] and org.num_nodes == 12 and org.embedding is None
    assert len(org.relations.keys()) == 3 and 2 * len(org.relations) + 1 >= 5 + 1      # what Trainer sizes the models with
    assert (td.x_train.numel(), td.x_val.numel(), td.x_test.numel()) == (6, 2, 2)
    assert sorted(torch.cat([td.x_train, td.x_val, td.x_test]).tolist()) == lab_idx.tolist()
    assert torch.equal(td.y_train, labels[td.x_train]) and td.y_train.dtype == torch.int64
    again = D.TensorDataset(**ok).orgGraph.training_data
    assert torch.equal(again.x_train, td.x_train) and not torch.equal(D.TensorDataset(**ok, seed=2).orgGraph.training_data.x_train, td.x_train)
    given = D.TensorDataset(**ok, split=(pos[4:], pos[:2], pos[2:4])).orgGraph.training_data
    assert given.x_train.tolist() == [4, 5, 6, 7, 8, 9] and given.x_val.tolist() == [0, 1] and torch.equal(given.y_test, labels[2:4])
    with pytest.raises(RuntimeError, match="no CPU path"):            # summaries are made on the GPU
        data.add_summary(k=1)
    with pytest.raises(ValueError):
        data.add_summary(partition=object())
    with pytest.raises(ValueError):
        data.add_summary(partition=Partition(torch.zeros(12, dtype=torch.int64), 1, 1, (1,), True), dedup=1)


# ---- the C ABI's refusals and workspace query: no launch, no device ------------------------------------------------------------------
def test_tr_block_labels_refusals():
    lib, p = _lib.load(), _p()
    need = lib.rgcn_tr_block_labels_workspace_bytes(100, 7, 10, 3)
    assert need == 256 and lib.rgcn_tr_block_labels_workspace_bytes(100, 70, 10, 3) == 1024      # B x C int32, 256-byte pieces

    def call(block=p, n=100, nb=7, idx=p, y=p, ldy=3, l=10, c=3, size=p, ysum=p, ld=3, nz=p, ws=p, nbytes=need):
        return lib.rgcn_tr_block_labels(block, n, nb, idx, y, ldy, l, c, size, ysum, ld, nz, None, ws, nbytes, None)

    assert call(size=None) == NULL and call(ysum=None) == NULL and call(nz=None) == NULL and call(ws=None) == NULL
    assert call(block=None) == NULL and call(idx=None) == NULL and call(y=None) == NULL
    assert call(nb=0) == ARG and call(c=0) == ARG and call(n=-1) == ARG and call(l=-1) == ARG and call(ld=2) == ARG and call(ldy=2) == ARG
    assert call(n=2 ** 31) == PLAN and call(nb=2 ** 31) == PLAN and call(l=2 ** 31) == PLAN and call(c=65537, ld=65537, ldy=65537) == PLAN
    assert call(nbytes=need - 1) == WS and call(nbytes=0) == WS
    for args in ((100, 0, 10, 3), (100, 7, 10, 0), (-1, 7, 10, 3), (100, 7, -1, 3), (2 ** 31, 7, 10, 3), (100, 2 ** 31, 10, 3), (100, 7, 10, 65537)):
        assert lib.rgcn_tr_block_labels_workspace_bytes(*args) == 0, args


def test_tr_gather_refusals():
    lib, p = _lib.load(), _p()

    def call(s=2, e=8, ld=8, rows=5, n=10, nodes=None, m=10, mode=0, seed=0, out=p, ld_out=None, plane=None, tab=p, mp=p, arrays=True):
        k = max(s, 1)
        tabs, mps = (ctypes.c_void_p * k)(*[tab] * k), (ctypes.c_void_p * k)(*[mp] * k)
        lds, rws = (ctypes.c_int32 * k)(*[ld] * k), (ctypes.c_int64 * k)(*[rows] * k)
        row = s * e if mode == 1 else e
        ld_out = row if ld_out is None else ld_out
        plane = m * ld_out if plane is None else plane
        if not arrays:
            tabs = None
        return lib.rgcn_tr_gather(tabs, lds, rws, mps, s, e, n, nodes, m, mode, seed, out, ld_out, plane, None, None)

    assert call(arrays=False) == NULL and call(tab=None) == NULL and call(mp=None) == NULL and call(out=None) == NULL
    assert call(s=0) == ARG and call(s=17) == ARG and call(e=0) == ARG and call(e=-4) == ARG
    assert call(mode=3) == ARG and call(mode=-1) == ARG and call(seed=-1) == ARG and call(n=-1) == ARG and call(m=-1) == ARG
    assert call(m=9) == ARG                                        # all nodes in order: n_out is num_nodes
    assert call(rows=-1) == ARG
    assert call(ld=7) == STRIDE and call(ld_out=7) == STRIDE and call(mode=1, ld_out=15) == STRIDE and call(plane=79) == STRIDE
    assert call(n=2 ** 31, m=2 ** 31) == PLAN and call(nodes=p, m=2 ** 31) == PLAN
    assert call(nodes=p, m=0) == 0 and call(n=0, m=0, mp=None, out=None) == 0          # nothing to do: no launch
    assert call(rows=0, tab=None, nodes=p, m=0) == 0
