"""``TensorDataset``: the dataset ``Trainer`` reads, for a graph that exists only as tensors.

``graphs.Dataset`` keys everything on node-name strings (``nodes``, ``node_to_enum``, ``org2type_dict``); a synthetic graph, or one
ingested elsewhere, has none.  ``TensorDataset`` holds the int64 COO the layer takes, the labelled node ids and their multi-hot
rows, and makes its summaries on the GPU: ``add_summary`` is ``summaries.node_partition`` -> ``summaries.quotient_graph`` ->
``transfer.summary_labels``, with no per-node Python on the way.  Together with ``transfer.stack_embeddings`` /
``concat_embeddings`` / ``sum_embeddings`` the reference's experiment runs as it does on a string-keyed dataset::

    data = TensorDataset(edge_index, edge_type, num_nodes, num_relations, labelled_idx, labels)
    data.add_summary(k=1)
    trainer = Trainer(data, hidden_l, epochs, emb_dim, lr, weight_d)
    trainer.train_summaries(configs)
    trainer.train_original(Emb_ATT_Layers, transfer.stack_embeddings, configs, exp)

``relations``: ``Trainer`` sizes its models with ``2 * len(graph.relations.keys()) + 1`` relations (a string-keyed graph has R
predicates and 2 R edge types: forward and inverse).  A tensor graph has ``num_relations`` edge types as they are, so ``relations``
is a dict of ``ceil(num_relations / 2)`` entries and the models get ``2 ceil(num_relations / 2) + 1 >= num_relations + 1`` relation
weights.  The surplus weights see no edge: they are dead relations, which the layer handles (tests/test_gpu_parity.py).

Mini-batches: a FROZEN transferred embedding never has to exist as a table.  With ``te = transfer.transferred_embedding(org,
data.sumGraphs, emb_dim, mode)``, ``model.forward_blocks_from_rows(blocks, act, te.rows(blocks[0].src_nodes))`` equals
``model.forward_blocks(blocks, act)`` after ``model.load_embedding(te.materialize())`` bit for bit, and reads ``[S, n_src, E]``
instead of ``[S, N, E]``.  (Not wired into the models or ``Trainer.train_minibatch``.)
"""
from __future__ import annotations

from typing import List, Optional

import torch
from torch import Tensor

from . import summaries
from .data import Data
from .transfer import summary_labels


class TensorGraph:
    """What ``Trainer`` reads of a graph: ``num_nodes``, ``relations``, ``training_data``, ``embedding``.  A summary graph also has
    ``org_block`` (int64 ``[N]``: the summary node of every original node) and ``block_size`` (int32: nodes per block)."""

    def __init__(self, name: str, num_nodes: int, relations: dict, training_data: Data) -> None:
        self.name, self.num_nodes, self.relations, self.training_data = name, num_nodes, relations, training_data
        self.num_edges = int(training_data.edge_type.shape[0])
        self.embedding: Optional[Tensor] = None
        self.org_block: Optional[Tensor] = None
        self.block_size: Optional[Tensor] = None


def _positions(name: str, t, n: int, device) -> Tensor:
    if not torch.is_tensor(t) or t.dtype != torch.int64 or t.dim() != 1:
        raise ValueError(f"split: {name} must be an int64 vector of positions into labelled_idx")
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= n):
        raise ValueError(f"split: {name} holds positions outside [0, {n})")
    return t.to(device)


class TensorDataset:
    """``edge_index`` int64 ``[2, E]`` / ``edge_type`` int64 ``[E]`` with ids in ``[0, num_nodes)`` / ``[0, num_relations)``, on the
    GPU; ``labelled_idx`` int64 ``[L]`` distinct node ids and ``labels`` int64 ``[L, C]`` their multi-hot rows, on the same device.
    ``split``: ``(train, val, test)`` int64 vectors of POSITIONS into ``labelled_idx``; None: 60 / 20 / 20 of
    ``torch.randperm(L, generator=manual_seed(seed))``.  Exposes ``orgGraph``, ``sumGraphs`` and ``num_classes``."""

    def __init__(self, edge_index: Tensor, edge_type: Tensor, num_nodes: int, num_relations: int, labelled_idx: Tensor, labels: Tensor,
                 *, split=None, seed: int = 1, name: str = "tensor_graph") -> None:
        summaries._check_coo(edge_index, edge_type, num_nodes, num_relations)
        dev = edge_index.device
        if not torch.is_tensor(labelled_idx) or labelled_idx.dtype != torch.int64 or labelled_idx.dim() != 1:
            raise ValueError("labelled_idx must be an int64 vector of node ids")
        n_lab = int(labelled_idx.shape[0])
        if not torch.is_tensor(labels) or labels.dtype != torch.int64 or labels.dim() != 2 or labels.shape[0] != n_lab or labels.shape[1] < 1:
            raise ValueError(f"labels must be int64 [{n_lab}, C] multi-hot rows with C >= 1")
        if labelled_idx.device != dev or labels.device != dev:
            raise ValueError(f"labelled_idx and labels must live on the graph's device ({dev})")
        if n_lab and (int(labelled_idx.min()) < 0 or int(labelled_idx.max()) >= num_nodes):
            raise ValueError(f"labelled_idx holds node ids outside [0, {num_nodes})")
        if n_lab and int(labels.min()) < 0:
            raise ValueError("labels must be non-negative counts")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"seed must be an int (got {seed!r})")
        if split is None:
            perm = torch.randperm(n_lab, generator=torch.Generator().manual_seed(seed)).to(dev)
            n_test = -(-n_lab // 5)
            n_val = -(-(n_lab - n_test) // 4)
            train, val, test = perm[n_test + n_val:], perm[n_test:n_test + n_val], perm[:n_test]
        else:
            if not isinstance(split, (list, tuple)) or len(split) != 3:
                raise ValueError("split must be (train, val, test): three int64 vectors of positions into labelled_idx")
            train, val, test = (_positions(nm, t, n_lab, dev) for nm, t in zip(("train", "val", "test"), split))
        td = Data(edge_index=edge_index)
        td.edge_type = edge_type
        td.x_train, td.x_val, td.x_test = labelled_idx[train], labelled_idx[val], labelled_idx[test]
        td.y_train, td.y_val, td.y_test = labels[train], labels[val], labels[test]
        self.num_relations = num_relations
        self.num_classes = int(labels.shape[1])
        self.orgGraph = TensorGraph(name, num_nodes, {i: i for i in range((num_relations + 1) // 2)}, td)
        self.sumGraphs: List[TensorGraph] = []

    def add_summary(self, k: Optional[int] = 1, direction: str = "out", *, partition=None, dedup: bool = False) -> TensorGraph:
        """Append the k-bisimulation summary of the original graph (``summaries.node_partition``; ``k=None``: the fixpoint), or the
        summary of a ``partition`` the caller made: its quotient graph (one summary edge per original edge, or with ``dedup`` the
        distinct triples), the fractional labels of its blocks, and ``org_block`` for the embedding transfer."""
        if not isinstance(dedup, bool):
            raise ValueError(f"dedup must be a bool (got {dedup!r})")
        org, td = self.orgGraph, self.orgGraph.training_data
        if partition is None:
            partition = summaries.node_partition(td.edge_index, td.edge_type, org.num_nodes, self.num_relations, k=k, direction=direction)
            label = f"bisim_k{'fix' if k is None else k}_{direction}"
        else:
            if not hasattr(partition, "block") or not hasattr(partition, "num_blocks"):
                raise ValueError("partition must be a summaries.Partition (block, num_blocks)")
            label = "partition"
        block, nb = partition.block, int(partition.num_blocks)
        ei, et, _ = summaries.quotient_graph(td.edge_index, td.edge_type, block, nb, dedup=dedup)
        x, y, size = summary_labels(block, nb, td.x_train, td.y_train)
        std = Data(edge_index=ei)
        std.edge_type = et
        std.x_train, std.y_train = x, y
        sg = TensorGraph(f"{org.name}_{label}", nb, dict(org.relations), std)
        sg.org_block, sg.block_size = block, size
        self.sumGraphs.append(sg)
        return sg
