"""The reference's experiment on a graph that exists only as tensors (scaling_rgcn_training_amd/tensor_data.py, transfer.py;
DESIGN.md 19): ``TensorDataset.add_summary`` -> ``Trainer.train_summaries`` -> ``Trainer.train_original`` with the three embedding
tricks, against the string-keyed ``graphs.Dataset`` path on the same graph given names, on 2,000 nodes / 20,000 edges / 8 relations
/ 4 classes."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
N, E, R, C, L = 2000, 20000, 8, 4, 600
EMB, HIDDEN = 16, 16


def _graph():
    g = torch.Generator().manual_seed(0)
    # few distinct neighbourhoods, so that k = 1 and k = 2 give summaries much smaller than the graph
    kind = torch.randint(0, 12, (N,), generator=g)
    src = torch.randint(0, N, (E,), generator=g)
    dst = torch.randint(0, N, (E,), generator=g)
    et = (kind[src] + kind[dst]) % R
    labelled = torch.randperm(N, generator=g)[:L]
    labels = torch.zeros(L, C, dtype=torch.int64)
    labels[torch.arange(L), kind[labelled] % C] = 1
    labels[torch.arange(40), (kind[labelled[:40]] + 1) % C] = 1         # some rows carry two classes
    return torch.stack([src, dst]), et, labelled, labels


def _named_dataset(ei, et, labelled, labels):
    """the same graph as a string-keyed graphs.Dataset: node i is <n000i>, relation pair p is <p{p}>, class c is <c{c}>"""
    from scaling_rgcn_training_amd import graphs as G
    from scaling_rgcn_training_amd.data import Data
    names = [f"<n{i:05d}>" for i in range(N)]
    org2type = {names[int(i)]: {f"<c{c}>" for c in torch.nonzero(row).flatten().tolist()} for i, row in zip(labelled, labels)}
    ds = G.Dataset(None)
    graph = G.Graph("named", org2type)
    graph.nodes, graph.node_to_enum, graph.num_nodes, graph.num_edges = names, {n: i for i, n in enumerate(names)}, N, E
    graph.relations = {f"<p{p}>": p for p in range(R // 2)}
    graph.training_data = Data(edge_index=ei.clone())
    graph.training_data.edge_type = et.clone()
    ds.orgGraph, ds.enum_classes, ds.num_classes = graph, {f"<c{c}>": c for c in range(C)}, C
    ds.make_training_data()
    return ds


@pytest.fixture(scope="module")
def datasets():
    from scaling_rgcn_training_amd.tensor_data import TensorDataset
    ei, et, labelled, labels = _graph()
    named = _named_dataset(ei, et, labelled, labels)
    # the named dataset's split (sklearn's), as positions into labelled_idx
    pos = torch.full((N,), -1, dtype=torch.int64)
    pos[labelled] = torch.arange(L)
    ntd = named.orgGraph.training_data
    split = tuple(pos[x].to(DEV) for x in (ntd.x_train, ntd.x_val, ntd.x_test))
    tensor = TensorDataset(ei.to(DEV), et.to(DEV), N, R, labelled.to(DEV), labels.to(DEV), split=split)
    for k in (1, 2):
        named.add_summary(k=k, direction="out", device=DEV)
        tensor.add_summary(k=k, direction="out")
    return named, tensor


def test_tensor_dataset_equals_the_string_keyed_one(datasets):
    named, tensor = datasets
    ntd, ttd = named.orgGraph.training_data, tensor.orgGraph.training_data
    for key in ("x_train", "y_train", "x_val", "y_val", "x_test", "y_test"):
        assert torch.equal(getattr(ttd, key).cpu(), getattr(ntd, key)), key
    assert len(tensor.sumGraphs) == len(named.sumGraphs) == 2 and tensor.num_classes == named.num_classes
    assert 2 * len(tensor.orgGraph.relations.keys()) + 1 == 2 * len(named.orgGraph.relations.keys()) + 1 == R + 1
    assert tensor.sumGraphs[0].num_nodes < N // 4                              # k = 1: blocks of several nodes
    for sg_t, sg_n in zip(tensor.sumGraphs, named.sumGraphs):
        t, n = sg_t.training_data, sg_n.training_data
        assert sg_t.num_nodes == sg_n.num_nodes <= N
        assert torch.equal(t.edge_index.cpu(), n.edge_index) and torch.equal(t.edge_type.cpu(), n.edge_type)
        assert torch.equal(t.x_train.cpu(), n.x_train) and t.x_train.numel() > 0
        assert t.y_train.dtype == n.y_train.dtype == torch.float32
        assert np.array_equal(t.y_train.cpu().numpy().view(np.uint32), n.y_train.numpy().view(np.uint32))
        assert sg_t is not tensor.sumGraphs[0] or bool(((t.y_train > 0) & (t.y_train < 1)).any())      # fractions, not 0 / 1 alone
        assert int(sg_t.block_size.sum()) == N and sg_t.org_block.shape == (N,)
        assert sg_t.relations == tensor.orgGraph.relations and sg_t.relations is not tensor.orgGraph.relations


def _models():
    from scaling_rgcn_training_amd import layers, transfer as T
    return {"sum": (layers.Emb_Layers, T.sum_embeddings), "stack": (layers.Emb_ATT_Layers, T.stack_embeddings),
            "concat": (layers.Emb_MLP_Layers, T.concat_embeddings)}


@pytest.mark.parametrize("mode", ("sum", "stack", "concat"))
def test_the_experiment_runs_on_tensors(datasets, mode):
    from scaling_rgcn_training_amd.trainer import Trainer
    _, tensor = datasets
    torch.manual_seed(0)
    trainer = Trainer(tensor, HIDDEN, 5, EMB, 0.01, 0.0005, verbose=False, hipgraph=False)
    configs = {"dataset": "SYNTH", "num_sums": len(tensor.sumGraphs), "e_trans": True, "e_freeze": False, "w_trans": True, "w_grad": True}
    trainer.train_summaries(configs)
    for sg in tensor.sumGraphs:
        assert sg.embedding.shape == (sg.num_nodes, EMB) and sg.embedding.device.type == "cuda"
    layer_cls, trick = _models()[mode]
    acc, loss, f1_w, f1_m, test_acc, test_f1_w, test_f1_m, model = trainer.train_original(layer_cls, trick, configs, "transfer")
    losses = loss["loss"]
    print(mode, "losses", losses, "test accuracy", test_acc)
    assert len(losses) == 5 and all(math.isfinite(v) for v in losses)
    assert losses[-1] < losses[0]
    table = model.embedding_table()
    assert table.device.type == "cuda" and table.shape[-2] == N


@pytest.mark.parametrize("mode", ("sum", "stack", "concat"))
def test_rows_feed_mini_batches_without_the_table(datasets, mode):
    """eval mode: forward_blocks_from_rows on te.rows(src_nodes) is forward_blocks after load_embedding(te.materialize()), bit for bit"""
    from scaling_rgcn_training_amd import transfer as T
    from scaling_rgcn_training_amd.sampling import NeighborSampler
    from scaling_rgcn_training_amd.trainer import do_nothing
    _, tensor = datasets
    g = torch.Generator().manual_seed(1)
    for sg in tensor.sumGraphs:
        sg.embedding = torch.randn(sg.num_nodes, EMB, generator=g).to(DEV)
    org, td = tensor.orgGraph, tensor.orgGraph.training_data
    block = tensor.sumGraphs[1].org_block.clone()
    block[torch.randperm(N, generator=g)[:500].to(DEV)] = -1             # a quarter of the nodes has no summary node: fills
    tensor.sumGraphs[1].org_block, kept = block, tensor.sumGraphs[1].org_block
    try:
        te = T.transferred_embedding(org, tensor.sumGraphs, EMB, mode, seed=6)
    finally:
        tensor.sumGraphs[1].org_block = kept
    layer_cls, _ = _models()[mode]
    torch.manual_seed(0)
    model = layer_cls(R + 1, HIDDEN, C, N, EMB, len(tensor.sumGraphs)).to(DEV)
    model.load_embedding(te.materialize(), freeze=True)
    model = model.to(DEV).eval()
    sampler = NeighborSampler(td.edge_index, td.edge_type, N, R + 1)
    blocks = sampler.sample(td.x_train[:64], [5, 5], seed=3)
    with torch.no_grad():
        want = model.forward_blocks(blocks, do_nothing)
        got = model.forward_blocks_from_rows(blocks, do_nothing, te.rows(blocks[0].src_nodes))
    te.check()
    assert want.shape == (64, C) and torch.equal(got, want)
