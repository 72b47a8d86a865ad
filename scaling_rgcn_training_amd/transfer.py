"""From a node partition to a trained original-graph model on tensors alone (csrc/rgcn_transfer.hip): the
fractional labels of a summary graph and the embedding every original node takes over from its summary nodes, without node
names, dicts or per-node Python.

* ``summary_labels``: what ``graphs.Dataset.make_training_data`` stores on a summary graph -- per block the label counts of its
  TRAINING nodes over the number of all its nodes -- from ``Partition.block`` and the training rows.
* ``TransferredEmbedding``: the reference's embedding tricks (model/embeddingTricks.py; ``graphs.get_tensor_list``) as one
  gather: a mapped node takes the row of its summary node, an unmapped node a uniform draw in [0, 1) that is a pure function of
  ``(seed, summary, node, column)``.  ``materialize()`` writes the whole ``[S, N, E]`` / ``[N, S E]`` / ``[N, E]`` tensor,
  ``rows(nodes)`` the rows of a node list -- the same bits, so a frozen transferred embedding composes with mini-batches
  without the table ever existing: ``model.forward_blocks_from_rows(blocks, act, te.rows(blocks[0].src_nodes))``.
* ``stack_embeddings`` / ``concat_embeddings`` / ``sum_embeddings``: the callables ``Trainer.train_original`` takes, for
  ``tensor_data.TensorGraph`` summaries (``org_block``) and for string-keyed ``graphs.Graph`` ones alike.

There is no CPU path: every argument is checked on the host, then the HIP library does the work.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib

MODES = tuple(_lib.TR_MODES)
MAX_SUMMARIES = _lib.TR_MAX_TABLES
MAX_IDS = 2 ** 31 - 1        # nodes, blocks and training rows are counted in int32 on the device
_NO_CPU = "runs only on an MI355X (ROCm 'cuda' device); there is no CPU fallback"


def _check_ids(what: str, name: str, t, device=None) -> None:
    if not torch.is_tensor(t) or t.dtype != torch.int64 or t.dim() != 1:
        raise ValueError(f"{what}: {name} must be an int64 vector (got {type(t).__name__ if not torch.is_tensor(t) else (t.dtype, tuple(t.shape))})")
    if device is not None and t.device != device:
        raise ValueError(f"{what}: {name} lives on {t.device}, not on {device}")


def _check_count(what: str, name: str, value, low: int, high: int) -> None:
    if isinstance(value, bool) or not isinstance(value, int) or not low <= value <= high:
        raise ValueError(f"{what}: {name} must be an int in {low} .. {high} (got {value!r})")


def _bad_ids(what: str, word: int) -> IndexError:
    names = [n for bit, n in ((_lib.TR_BAD_BLOCK, "a block id outside [0, num_blocks)"),
                              (_lib.TR_BAD_NODE, "a node id outside [0, num_nodes)"),
                              (_lib.TR_BAD_MAP, "a map value below -1 or past its table")) if word & bit]
    return IndexError(f"{what}: " + " and ".join(names) + " (such entries were not used as addresses and contributed nothing)")


def summary_labels(block: Tensor, num_blocks: int, train_idx: Tensor, y_train: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """``(x_train_sum, y_train_sum, size)`` of the partition ``block`` (int64 ``[N]``, ids in ``[0, num_blocks)``): ``size`` int32
    ``[B]`` counts the nodes of every block, ``x_train_sum`` holds the ascending block ids whose label row is not all zero and
    ``y_train_sum`` float32 ``[len, C]`` their rows ``sum of y_train over the block's training nodes / max(1, size)`` -- the double
    quotient rounded to float32, ``make_training_data``'s values bit for bit.  ``train_idx`` int64 ``[L]`` (distinct node ids),
    ``y_train`` int64 ``[L, C]`` (multi-hot rows or counts).  Validation and test nodes contribute nothing because they are not
    passed.  ONE read-back (the number of non-zero rows, with the word that flags ids out of range: ``IndexError``)."""
    what = "summary_labels"
    _check_ids(what, "block", block)
    _check_count(what, "num_blocks", num_blocks, 1, MAX_IDS)
    _check_ids(what, "train_idx", train_idx, block.device)
    if not torch.is_tensor(y_train) or y_train.dtype != torch.int64 or y_train.dim() != 2 or y_train.shape[0] != train_idx.shape[0] \
            or y_train.shape[1] < 1:
        raise ValueError(f"{what}: y_train must be int64 [{int(train_idx.shape[0])}, C] with C >= 1")
    if y_train.device != block.device:
        raise ValueError(f"{what}: y_train lives on {y_train.device}, not on {block.device}")
    if block.shape[0] > MAX_IDS or train_idx.shape[0] > MAX_IDS or y_train.shape[1] > 65536:
        raise ValueError(f"{what}: at most 2^31 - 1 nodes and training rows and 65536 classes")
    if block.device.type != "cuda":
        raise RuntimeError(f"{what} {_NO_CPU}")
    dev = block.device
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    size, y_sum, nonzero = _lib.tr_block_labels(block.contiguous(), num_blocks, train_idx.contiguous(), y_train.contiguous(), bad)
    count, word = torch.cat([nonzero.sum(dtype=torch.int32).reshape(1), bad]).tolist()
    if word:
        raise _bad_ids(what, word)
    # a stable sort puts the flagged blocks first and keeps them ascending: no second synchronisation
    x = torch.argsort(nonzero, descending=True, stable=True)[:count]
    return x, y_sum.index_select(0, x), size


class TransferredEmbedding:
    """``tables``: S (1 .. 16) fp32 ``[B_s, E]`` device tensors with a contiguous last dimension (row-strided views are taken as
    they are); ``maps``: S int64 ``[num_nodes]`` tensors, the row of every node in its table or -1 where it is not mapped;
    ``mode``: ``"stack"`` ``[S, M, E]``, ``"concat"`` ``[M, S E]`` or ``"sum"`` ``[M, E]`` (``((0 + t_0) + t_1) + ...`` in fp32:
    Python's ``sum(list)``).  Calls are asynchronous; ids out of range give zeros and are reported by ``check()``."""

    def __init__(self, tables: Sequence[Tensor], maps: Sequence[Tensor], num_nodes: int, mode: str = "stack", seed: int = 0) -> None:
        what = "TransferredEmbedding"
        if mode not in MODES:
            raise ValueError(f"{what}: mode must be one of {MODES} (got {mode!r})")
        if not isinstance(tables, (list, tuple)) or not isinstance(maps, (list, tuple)) or len(tables) != len(maps):
            raise ValueError(f"{what}: tables and maps must be lists of one length")
        if not 1 <= len(tables) <= MAX_SUMMARIES:
            raise ValueError(f"{what}: 1 .. {MAX_SUMMARIES} summaries (got {len(tables)})")
        _check_count(what, "num_nodes", num_nodes, 0, MAX_IDS)
        _check_count(what, "seed", seed, 0, 2 ** 63 - 1)
        for t in tables:
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] < 1:
                raise ValueError(f"{what}: every table must be a float32 [rows, E] tensor with E >= 1")
            if t.shape[1] != tables[0].shape[1]:
                raise ValueError(f"{what}: the tables have widths {[int(u.shape[1]) for u in tables]}, they must share one")
            if t.shape[1] > 1 and t.stride(1) != 1:
                raise ValueError(f"{what}: the last dimension of a table must be contiguous (strides {t.stride()})")
            if t.shape[0] > 1 and t.stride(0) < t.shape[1]:
                raise ValueError(f"{what}: the rows of a table must not overlap (strides {t.stride()})")
            if t.device != tables[0].device:
                raise ValueError(f"{what}: the tables live on {t.device} and {tables[0].device}")
        dev = tables[0].device
        for m in maps:
            _check_ids(what, "a map", m, dev)
            if m.shape[0] != num_nodes:
                raise ValueError(f"{what}: a map holds {int(m.shape[0])} entries for {num_nodes} nodes")
        if dev.type != "cuda":
            raise RuntimeError(f"{what} {_NO_CPU}")
        self.tables = [t.detach() for t in tables]
        self.maps = [m.contiguous() for m in maps]
        self.num_nodes, self.mode, self.seed = num_nodes, mode, seed
        self.num_summaries, self.emb_dim, self.device = len(tables), int(tables[0].shape[1]), dev
        self._bad = torch.zeros(1, dtype=torch.int32, device=dev)

    def _gather(self, nodes: Optional[Tensor], m: int) -> Tensor:
        s, e = self.num_summaries, self.emb_dim
        shape = {"stack": (s, m, e), "concat": (m, s * e), "sum": (m, e)}[self.mode]
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        _lib.tr_gather(self.tables, self.maps, self.num_nodes, e, nodes, _lib.TR_MODES[self.mode], self.seed, out, self._bad)
        return out

    def materialize(self) -> Tensor:
        """the tensor of all ``num_nodes`` nodes in order"""
        return self._gather(None, self.num_nodes)

    def rows(self, nodes: Tensor) -> Tensor:
        """the tensor of the nodes ``nodes`` (int64 ``[M]``, repeats allowed): ``materialize()`` indexed by ``nodes`` along the
        node axis, bit for bit, fills included -- without the full tensor"""
        _check_ids("TransferredEmbedding.rows", "nodes", nodes, self.device)
        return self._gather(nodes.contiguous(), int(nodes.shape[0]))

    def check(self) -> None:
        """Raise if a call since the last ``check()`` met an id out of range.  Reads one word back: SYNCHRONISES."""
        word = int(self._bad.item())
        if word:
            self._bad.zero_()
            raise _bad_ids("TransferredEmbedding", word)


# ---- the embedding tricks Trainer.train_original takes ---------------------------------------------------------------------------
def _node_map(graph, sum_graph, device) -> Tensor:
    """int64 [N] on ``device``: ``sum_graph.org_block`` where the summary was made from tensors, else the map of the two
    string-keyed node dicts (``graphs.transfer_index``: per-node Python, the only kind of map such a graph has)"""
    block = getattr(sum_graph, "org_block", None)
    if block is None:
        from .graphs import transfer_index
        block = transfer_index(graph, sum_graph)
    return block.to(device)


def transferred_embedding(graph, sum_graphs, emb_dim: int, mode: str, seed: int = 0) -> TransferredEmbedding:
    """the ``TransferredEmbedding`` of ``graph`` over the trained ``sum_graphs`` (their ``embedding`` tables, moved to the GPU
    where they are not there yet)"""
    if len(sum_graphs) == 0:
        raise ValueError("embedding transfer needs at least one summary graph")
    tables: List[Tensor] = []
    for sg in sum_graphs:
        emb = getattr(sg, "embedding", None)
        if not torch.is_tensor(emb) or emb.dim() != 2 or emb.shape[1] != emb_dim:
            raise ValueError(f"every summary graph needs a trained [rows, {emb_dim}] embedding "
                             f"(got {tuple(emb.shape) if torch.is_tensor(emb) else type(emb).__name__})")
        emb = emb.detach()
        tables.append(emb if emb.device.type == "cuda" else emb.to("cuda"))
    dev = tables[0].device
    maps = [_node_map(graph, sg, dev) for sg in sum_graphs]
    return TransferredEmbedding([t.to(dev) for t in tables], maps, int(graph.num_nodes), mode, seed)


def _trick(graph, sum_graphs, emb_dim: int, mode: str) -> Tensor:
    te = transferred_embedding(graph, sum_graphs, emb_dim, mode)
    out = te.materialize()
    te.check()
    return out


def stack_embeddings(graph, sum_graphs, emb_dim: int) -> Tensor:
    """``[S, N, emb]`` on the GPU (``Emb_ATT_Layers``)"""
    return _trick(graph, sum_graphs, emb_dim, "stack")


def concat_embeddings(graph, sum_graphs, emb_dim: int) -> Tensor:
    """``[N, S emb]`` on the GPU (``Emb_MLP_Layers``)"""
    return _trick(graph, sum_graphs, emb_dim, "concat")


def sum_embeddings(graph, sum_graphs, emb_dim: int) -> Tensor:
    """``[N, emb]`` on the GPU (``Emb_Layers``)"""
    return _trick(graph, sum_graphs, emb_dim, "sum")
