"""Host side of the GPU summaries: every refusal of summaries.node_partition / quotient_graph is raised before the HIP library
is touched, and graphs.summary_graph / Dataset.add_summary assemble a trainable summary graph from a partition (here the
oracle's: tests/summary_reference.py).  CPU only."""
import os

import pytest
import torch

from scaling_rgcn_training_amd import _lib, graphs as G, summaries as S
from tests import summary_reference as R
from tests.conftest import GOLDEN_DIR

TEST_NT = os.path.join(GOLDEN_DIR, "TEST", "TEST_complete.nt")


@pytest.fixture
def no_library(monkeypatch):
    """any attempt to reach the library fails the test"""
    def boom(*a, **k):
        raise AssertionError("the HIP library was touched")
    monkeypatch.setattr(_lib, "load", boom)


def _graph(e=6, n=5, r=3):
    return R.random_graph(n, e, r, seed=0)


def test_partition_refusals(no_library):
    ei, et = _graph()
    ok = dict(num_nodes=5, num_relations=3)
    part = lambda *a, **k: S.node_partition(*a, **{**ok, **k})
    # a well-formed call on CPU tensors: there is no CPU path
    with pytest.raises(RuntimeError, match="no CPU path"):
        part(ei, et)
    with pytest.raises(RuntimeError, match="no CPU path"):
        part(ei, et, k=None, direction="in_out", initial=torch.zeros(5, dtype=torch.int64))
    bad = [
        dict(direction="both"), dict(direction=None), dict(k=0), dict(k=-1), dict(k=1.5), dict(k=True), dict(max_rounds=0),
        dict(num_nodes=0), dict(num_nodes=2 ** 31), dict(num_nodes=5.0), dict(num_relations=0), dict(num_relations=65537),
        dict(num_nodes=4),                      # node id 4 out of range (the graph below uses it)
        dict(num_relations=2),                  # relation id 2 out of range
        dict(initial=torch.zeros(4, dtype=torch.int64)), dict(initial=torch.zeros(5, dtype=torch.int32)),
        dict(initial=torch.zeros(5, 1, dtype=torch.int64)), dict(initial=torch.tensor([0, 0, -1, 0, 0])),
        dict(initial=torch.tensor([0, 0, 2 ** 31 - 1, 0, 0])), dict(initial=[0] * 5), dict(_route=3),
    ]
    ei[0, 0], et[0] = 4, 2
    for kw in bad:
        with pytest.raises(ValueError):
            part(ei, et, **kw)
    neg = ei.clone()
    neg[1, 2] = -1
    for a, b in ((neg, et), (ei, -et - 1), (ei.int(), et), (ei, et.int()), (ei.float(), et), (ei[0], et), (ei.t(), et),
                 (ei[:, :5], et), (ei, et[:, None]), (ei.tolist(), et)):
        with pytest.raises(ValueError):
            part(a, b)


def test_partition_size_limits(no_library):
    """the u32 counts of the sort: 0xFFFF0000 keys, one per edge, two for in_out -- checked on shapes alone (meta tensors)"""
    big = S.MAX_KEYS + 1
    ei, et = torch.empty(2, big, dtype=torch.int64, device="meta"), torch.empty(big, dtype=torch.int64, device="meta")
    with pytest.raises(ValueError, match="keys"):
        S.node_partition(ei, et, 10, 3, direction="out")
    half = S.MAX_KEYS // 2 + 1
    ei, et = torch.empty(2, half, dtype=torch.int64, device="meta"), torch.empty(half, dtype=torch.int64, device="meta")
    with pytest.raises(ValueError, match="keys"):
        S.node_partition(ei, et, 10, 3, direction="in_out")
    with pytest.raises(ValueError, match="keys"):
        S.quotient_graph(torch.empty(2, big, dtype=torch.int64, device="meta"), torch.empty(big, dtype=torch.int64, device="meta"),
                         torch.zeros(10, dtype=torch.int64), 1)
    assert S.MAX_KEYS == _lib.SUMMARY_MAX_KEYS and S.MAX_RELATIONS == _lib.SUMMARY_MAX_RELATIONS
    assert tuple(_lib.SUMMARY_DIRECTIONS) == S.DIRECTIONS and list(_lib.SUMMARY_DIRECTIONS.values()) == [0, 1, 2]


def test_quotient_refusals(no_library):
    ei, et = _graph()
    block = torch.tensor([0, 1, 0, 2, 1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.quotient_graph(ei, et, block, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.quotient_graph(ei, et, block, 3, dedup=False)
    for b, nb in ((block, 2), (block, 0), (block, 2 ** 31), (block.int(), 3), (block[:4], 3), (-block, 3), (block[:, None], 3),
                  (block.tolist(), 3), (block, 3.0)):
        with pytest.raises(ValueError):
            S.quotient_graph(ei, et, b, nb)
    for a, t in ((ei.int(), et), (ei, et[:-1]), (ei + 5, et), (ei, et - 1), (ei, et + 65536)):
        with pytest.raises(ValueError):
            S.quotient_graph(a, t, block, 3)
    with pytest.raises(ValueError):
        S.quotient_graph(ei, et, block, 3, _route=-1)


# ---- graphs.summary_graph / Dataset.add_summary with the oracle's partition -----------------------------------------------------
@pytest.fixture(scope="module")
def dataset():
    data = G.Dataset(TEST_NT)                     # no summary files, no map files
    data.init_dataset()
    assert data.sumGraphs == [] and data.orgGraph.training_data.x_train.numel() > 0
    org = data.orgGraph
    td = org.training_data
    parts = {}
    for k, d in ((1, "in_out"), (2, "out")):
        parts[k, d] = R.node_partition(td.edge_index, td.edge_type, org.num_nodes, 2 * len(org.relations), k=k, direction=d)
        data.add_summary(k=k, direction=d, partition=parts[k, d])
    return data, parts


def test_summary_graph_maps_and_relations(dataset):
    data, parts = dataset
    org = data.orgGraph
    assert len(data.sumGraphs) == 2
    for sg, p in zip(data.sumGraphs, parts.values()):
        assert sg.num_nodes == p.num_blocks and sg.nodes == [f"<b{i}>" for i in range(p.num_blocks)]
        assert sg.node_to_enum == {n: i for i, n in enumerate(sg.nodes)}
        assert sg.relations == org.relations and sg.relations is not org.relations
        # both maps, both ways
        assert set(sg.orgNode2sumNode_dict) == set(org.nodes)
        for node, i in org.node_to_enum.items():
            s = sg.orgNode2sumNode_dict[node]
            assert s == f"<b{int(p.block[i])}>" and node in sg.sumNode2orgNode_dict[s]
        assert sorted(n for v in sg.sumNode2orgNode_dict.values() for n in v) == sorted(org.nodes)
        assert all(v for v in sg.sumNode2orgNode_dict.values())            # canonical ids: no empty block
        # one summary edge per original edge, in the original's relation ids
        td, otd = sg.training_data, org.training_data
        assert torch.equal(td.edge_index, p.block[otd.edge_index]) and torch.equal(td.edge_type, otd.edge_type)
        assert td.edge_index.dtype == torch.int64 and td.edge_index.is_contiguous()
        # transfer_index finds every original node
        idx = G.transfer_index(org, sg)
        assert torch.equal(idx, p.block)
    assert data.sumGraphs[0].name.endswith("_bisim_k1_in_out") and data.sumGraphs[1].name.endswith("_bisim_k2_out")


def test_training_data_of_generated_summaries(dataset):
    data, _ = dataset
    nc = data.num_classes
    for sg in data.sumGraphs:
        td = sg.training_data
        assert td.x_train.numel() > 0 and td.y_train.shape == (td.x_train.numel(), nc)
        assert int(td.x_train.max()) < sg.num_nodes
        assert torch.all(td.y_train.sum(1) > 0)
        assert len(sg.relations) == len(data.orgGraph.relations)             # make_training_data's own assertion
    # the original's split is what the file-based dataset gives
    t = os.path.join(GOLDEN_DIR, "TEST")
    ref = G.Dataset(TEST_NT, os.path.join(t, "attr", "sum"), os.path.join(t, "attr", "map"))
    ref.init_dataset()
    assert len(ref.sumGraphs) == 3
    for k in ("x_train", "y_train", "x_val", "x_test"):
        assert torch.equal(getattr(ref.orgGraph.training_data, k), getattr(data.orgGraph.training_data, k))


def test_summary_graph_refuses_a_partition_of_another_graph(dataset):
    data, parts = dataset
    p = parts[1, "in_out"]
    with pytest.raises(ValueError):
        G.summary_graph(data.orgGraph, p._replace(block=p.block[:-1]), "x")
    with pytest.raises(RuntimeError, match="no CPU path"):                   # the deduplicated form is made on the GPU
        G.summary_graph(data.orgGraph, p, "x", dedup=True)
    with pytest.raises(RuntimeError, match="init_dataset"):
        G.Dataset(TEST_NT).add_summary(partition=p)
