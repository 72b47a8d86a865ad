"""Neighbour sampling on the GPU (csrc/rgcn_sample.hip): fan-out sampling of in-edges into the layered bipartite
blocks a mini-batch step walks -- what PyG's ``NeighborLoader`` / DGL's ``sample_neighbors`` do on the host.

``NeighborSampler`` builds the in-edge index of a graph once (edges sorted stably by destination); ``sample(seeds, fanouts,
seed)`` returns one ``Block`` per model layer, sampled from the last layer back: ``blocks[-1]`` has the seeds as destinations,
``blocks[i]`` the source nodes of ``blocks[i + 1]``.  A block's ``src_nodes`` start with its destinations, so a layer runs as
``conv((x, x[:block.n_dst]), block.edge_index, block.edge_type)`` with ``x`` the rows ``src_nodes`` of its input.

A layer's fan-out is one int for all in-edges of a destination, or one int PER RELATION (a list / tuple: RGCNConv normalises per
(destination, relation), so a pooled draw starves the rare relations of a hub).

The choice of a destination's in-edges is a pure function of ``(seed, layer, global node id)`` -- and of the relation, with
per-relation fan-outs -- (a counter-based generator and Floyd's k-subset algorithm): it depends neither on the other nodes of the
batch nor on launch geometry, and two calls return equal tensors.  There is no CPU path: every argument is checked on the host, then the HIP library does the work.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

import torch
from torch import Tensor

from .summaries import _check_coo, _need_gpu

MAX_FANOUT = 256


class Block(NamedTuple):
    edge_index: Tensor      # int64 [2, E_b]: positions in src_nodes (row 0) and among the destinations (row 1)
    edge_type: Tensor       # int64 [E_b]
    n_src: int
    n_dst: int
    src_nodes: Tensor       # int64 [n_src] global node ids; src_nodes[:n_dst] are the destinations


class BlockIndex:
    """The index one mini-batch layer walks straight from a ``Block`` (csrc/rgcn_minibatch.hip): the block's edges
    plus one root pseudo edge per destination, sorted by (relation, destination), cut into rows of at most 256 edges that lie
    relation-major in tiles of 16, with the destination-major list of rows and the source-major list of (row, scale).  One index
    serves ``RGCNConv.forward_block``'s forward, dX and d_weight; it is built once per (block, aggregation) by ``block_index``
    and owns its arrays."""

    def __init__(self, lib_index, aggr: str):
        self._ix = lib_index
        self.aggr = aggr
        self.n_src, self.n_dst, self.num_edges = lib_index.n_src, lib_index.n_dst, lib_index.num_edges
        self.num_relations, self.n_rows, self.n_tiles = lib_index.num_relations, lib_index.n_rows, lib_index.n_tiles
        self.device = lib_index.arena.device

    def __getattr__(self, name):      # tile_ptr, row_beg, row_cnt, row_dst, row_scale, edge_src, dst_ptr, dst_rows, src_ptr, ...
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self._ix, name)


def check_block(block, num_relations: int, aggr: str = "mean") -> None:
    """what ``block_index`` refuses on the host, before the library is loaded"""
    if aggr not in ("mean", "sum", "add"):
        raise ValueError(f"block_index aggregates by mean / sum (got {aggr!r})")
    if isinstance(num_relations, bool) or not isinstance(num_relations, int) or num_relations < 1:
        raise ValueError(f"num_relations must be an int >= 1 (got {num_relations!r})")
    ei, et = block.edge_index, block.edge_type
    if not torch.is_tensor(ei) or not torch.is_tensor(et) or ei.dim() != 2 or ei.shape[0] != 2 or et.dim() != 1 \
            or ei.shape[1] != et.shape[0]:
        raise ValueError("a block holds edge_index [2, E_b] and edge_type [E_b]")
    if ei.dtype != torch.int64 or et.dtype != torch.int64:
        raise ValueError(f"edge_index and edge_type must be int64 (got {ei.dtype}, {et.dtype})")
    if block.n_src < 0 or block.n_dst < 0 or block.n_dst > block.n_src:
        raise ValueError(f"a block's destinations are its first source rows: n_dst ({block.n_dst}) must lie in [0, n_src = {block.n_src}]")
    if et.shape[0] and block.n_dst == 0:
        raise ValueError(f"edge_index out of range: {int(et.shape[0])} edges into 0 destinations")
    _need_gpu(ei, "block_index")
    if et.device != ei.device:
        raise RuntimeError(f"block_index: edge_type ({et.device}) must be on the device of edge_index ({ei.device})")


def block_index(block: Block, num_relations: int, aggr: str = "mean") -> BlockIndex:
    """Build the ``BlockIndex`` of ``block`` on its device: three radix sorts and one host synchronisation.  No order is required
    of the block's edges; an id out of range raises (found on the device)."""
    check_block(block, num_relations, aggr)
    from . import _lib
    aggr = "sum" if aggr == "add" else aggr
    try:
        ix = _lib.mb_index_build(block.edge_index, block.edge_type, block.n_src, block.n_dst, num_relations, mean=aggr == "mean")
    except _lib.RgcnLibraryError as err:
        if getattr(err, "status", 0) == _lib.ERR_GRAPH:
            raise ValueError(f"edge_index / edge_type out of range: sources must lie in [0, {block.n_src}), destinations in "
                             f"[0, {block.n_dst}), relations in [0, {num_relations})") from err
        raise
    return BlockIndex(ix, aggr)


def check_fanouts(fanouts, num_relations: Optional[int] = None) -> list:
    """a non-empty sequence with one entry per layer: an int in {-1} u [1, 256] (one fan-out for all in-edges of a destination), or
    a list / tuple of ints in {-1, 0} u [1, 256], one per relation (its length is checked against
    ``num_relations`` where that is given).  Returns a list whose sequence entries are lists."""
    if isinstance(fanouts, (str, bytes)) or not isinstance(fanouts, Sequence) or len(fanouts) == 0:
        raise ValueError(f"fanouts must be a non-empty sequence, one entry per layer (got {fanouts!r})")
    out = []
    for k in fanouts:
        if isinstance(k, (list, tuple)):
            if len(k) == 0 or (num_relations is not None and len(k) != num_relations):
                raise ValueError(f"a per-relation fan-out takes one int per relation"
                                 + (f" ({num_relations})" if num_relations is not None else "") + f", got {len(k)} entries")
            for kt in k:
                if isinstance(kt, bool) or not isinstance(kt, int) or not (-1 <= kt <= MAX_FANOUT):
                    raise ValueError(f"a per-relation fan-out entry must be -1 (the whole run), 0 (nothing of that relation) or "
                                     f"an int in 1 .. {MAX_FANOUT} (got {kt!r})")
            out.append(list(k))
            continue
        if isinstance(k, bool) or not isinstance(k, int) or not (k == -1 or 1 <= k <= MAX_FANOUT):
            raise ValueError(f"a fan-out must be -1 (all in-edges), an int in 1 .. {MAX_FANOUT}, or a list / tuple with one "
                             f"such int (or 0) per relation (got {k!r})")
        out.append(k)
    return out


def check_seeds(seeds, num_nodes: int) -> None:
    """int64 [n], unique, in [0, num_nodes): one reduction where the seeds live"""
    if not torch.is_tensor(seeds) or seeds.dim() != 1 or seeds.dtype != torch.int64:
        raise ValueError("seeds must be a 1-d int64 tensor")
    if seeds.numel():
        s = torch.sort(seeds).values
        lo, hi, repeats = torch.stack([s[0], s[-1], (s[1:] == s[:-1]).sum()]).tolist()
        if lo < 0 or hi >= num_nodes:
            raise ValueError(f"seeds must lie in [0, {num_nodes}) (got [{lo}, {hi}])")
        if repeats:
            raise ValueError("seeds must be unique")


def check_sample_seed(seed) -> int:
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 63:
        raise ValueError(f"seed must be an int in [0, 2^63) (got {seed!r})")
    return seed


class NeighborSampler:
    """``NeighborSampler(edge_index [2, E], edge_type [E], num_nodes, num_relations)`` on GPU tensors (``edge_index`` may be the
    strided rows of a transposed [E, 3] tensor).  Builds the index once and owns its arrays (12 bytes per edge, 8 per node)."""

    def __init__(self, edge_index: Tensor, edge_type: Tensor, num_nodes: int, num_relations: int):
        from . import _lib
        _check_coo(edge_index, edge_type, num_nodes, num_relations)
        _need_gpu(edge_index, "NeighborSampler")
        self.num_nodes, self.num_relations = num_nodes, num_relations
        self.num_edges = int(edge_type.shape[0])
        self.device = edge_index.device
        graph, keep = _lib.graph_struct(edge_index, edge_type, num_nodes, num_relations)
        self._index, self._arrays = _lib.sample_index_build(graph, self.device)
        del keep
        # the relation index is built from the caller's edges on the first per-relation hop: until then the sampler
        # holds references to them and nothing more
        self._edges = (edge_index, edge_type)
        self._rel_index = self._rel_arrays = None
        # node id -> position in the block being built; all "none" (-1) between hops, which reset only what they wrote
        self._map = torch.full((num_nodes,), -1, dtype=torch.int32, device=self.device)

    def _relation_index(self):
        if self._rel_index is None:
            from . import _lib
            graph, keep = _lib.graph_struct(self._edges[0], self._edges[1], self.num_nodes, self.num_relations)
            self._rel_index, self._rel_arrays = _lib.sample_rel_index_build(graph, self.device)
            del keep
        return self._rel_index

    def sample(self, seeds: Tensor, fanouts: Sequence, seed: int = 0) -> List[Block]:
        """``blocks[0 .. L-1]``, ``fanouts[i]`` belonging to model layer ``i``: an int (at most that many in-edges per destination,
        all relations pooled) or a list / tuple of ``num_relations`` ints (at most ``fanouts[i][t]`` in-edges per destination AND
        relation ``t``; -1 all, 0 none).  The two may be mixed across layers.  One host synchronisation per layer."""
        from . import _lib
        fanouts = check_fanouts(fanouts, getattr(self, "num_relations", None))
        seed = check_sample_seed(seed)
        check_seeds(seeds, self.num_nodes)
        dst = seeds.to(self.device).contiguous()
        blocks = []
        for i in reversed(range(len(fanouts))):
            if isinstance(fanouts[i], list):
                ei, et, src_nodes = _lib.sample_hop_rel(self._relation_index(), dst, fanouts[i], seed, i, self._map)
            else:
                ei, et, src_nodes = _lib.sample_hop(self._index, dst, fanouts[i], seed, i, self._map)
            blocks.append(Block(ei, et, int(src_nodes.shape[0]), int(dst.shape[0]), src_nodes))
            dst = src_nodes
        return blocks[::-1]
