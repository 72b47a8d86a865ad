"""Attribute-summary generation: every node is mapped to the 128-bit MurmurHash3 of its sorted
set of outgoing / incoming / incoming+outgoing predicates; the summary graph replaces every node by its hash and the
map file records ``<hash> <isSummaryOf> node``.  Contract: /root/reference/graphs/createAttributeSum.py:6-67
(``create_sum_map`` / ``write_sum_map_files``), whose hash is ``mmh3.hash128`` -- a C extension that is not in this
image; here it is ``csrc/murmur3_x64_128.c`` (plain C, built into ``librgcn_host.so``).  Integer / byte work: results
are bit-exact and pinned by the reference's shipped ``graphs/TEST/attr`` files (tests/test_summaries.py).

``legacy=True`` reproduces those shipped files byte for byte: they were written by an earlier version of the
reference script that neither lower-cased the terms nor skipped ``rdf:type`` when collecting predicate sets (the
hash-named ids in them are murmur3 of e.g. ``<...#isAbout>`` with its capital A and of the rdf:type predicate alone).
The default follows the script as it is in the reference today (lower-cased, rdf:type excluded from the sets).

``node_partition`` / ``quotient_graph`` are the integer form of the same step, on the GPU (csrc/rgcn_summary.hip):
k rounds of partition refinement over the int64 COO the layer takes -- round 1 from the trivial partition is the attribute
summary over relation ids, rounds 2 .. k the k-bisimulation -- and the quotient graph of a partition.  There is no CPU path:
every argument is checked on the host, then the HIP library does the work.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import defaultdict
from typing import Dict, Iterable, List, NamedTuple, Optional, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.path.join(_HERE, "librgcn_host.so")
RDF_TYPE = "<http://www.w3.org/1999/02/22-rdf-syntax-ns#type>"
LITERAL_KEY = "http://example.org/literal"
_host = None


def _lib():
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise RuntimeError(f"{HOST_LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        _host = C.CDLL(HOST_LIB_PATH)
        _host.rgcn_murmur3_x64_128.restype = None
        _host.rgcn_murmur3_x64_128.argtypes = [C.c_char_p, C.c_int64, C.c_uint32, C.POINTER(C.c_uint64 * 2)]
    return _host


def hash128(key: bytes, seed: int = 0) -> int:
    """``mmh3.hash128(key, seed)``: MurmurHash3 x64 128, unsigned, little-endian (h1 | h2 << 64)."""
    out = (C.c_uint64 * 2)()
    _lib().rgcn_murmur3_x64_128(key, len(key), seed, C.byref(out))
    return int(out[0]) | (int(out[1]) << 64)


def _split(triple: str, lower: bool):
    parts = triple[:-2].split(" ", maxsplit=2)
    if parts == [""]:
        return None
    return tuple(p.lower() for p in parts) if lower else tuple(parts)


def property_hashes(triples: Iterable[str], legacy: bool = False) -> Tuple[Dict[str, int], Dict[str, int], Dict[str, int]]:
    """(outgoing, incoming, incoming + outgoing) hash per entity -- createAttributeSum.py:7-38"""
    outgoing, incoming = defaultdict(set), defaultdict(set)
    for t in triples:
        spo = _split(t, lower=not legacy)
        if spo is None:
            continue
        s, p, o = spo
        if legacy or p != RDF_TYPE:
            outgoing[s].add(p)
            if o.startswith('"'):
                incoming[LITERAL_KEY].add(p)
            else:
                incoming[o].add(p)
    h = lambda ps: hash128(",".join(sorted(ps)).encode("utf8"))
    out_h = {k: h(v) for k, v in outgoing.items()}
    in_h = {k: h(v) for k, v in incoming.items()}
    both = {e: in_h.get(e, 0) + out_h.get(e, 0) for e in set(in_h) | set(out_h)}
    return out_h, in_h, both


def write_sum_map_files(hashes: Dict[str, int], triples: List[str], sum_path: str, map_path: str, legacy: bool = False) -> None:
    """createAttributeSum.py:44-67: the summary graph (every term replaced by its hash, '0' when it has none) and the
    map file (insertion order of first appearance, last assignment wins -- a Python dict, as in the reference)."""
    mapping: Dict[str, object] = {}
    with open(sum_path, "w") as f:
        for t in triples:
            spo = _split(t, lower=not legacy)
            if spo is None:
                continue
            s, p, o = spo
            if o.startswith('"') and LITERAL_KEY in hashes:
                obj = hashes[LITERAL_KEY]
            else:
                obj = hashes[o] if o in hashes else "0"
            sub = hashes[s] if s in hashes else "0"
            mapping[s] = sub
            mapping[o] = obj
            f.write(f"<{sub}> {p} <{obj}> .\n")
    with open(map_path, "w") as m:
        for o_node, s_node in mapping.items():
            m.write(f"<{s_node}> <isSummaryOf> {o_node} .\n")


def create_sum_map(path: str, sum_path: str, map_path: str, dataset: str, legacy: bool = False) -> None:
    """``create_sum_map`` of the reference (main.py:39 ``-create_attr_sum``): writes
    ``{sum_path}{dataset}_sum_{out,in,in_out}.nt`` and ``{map_path}{dataset}_map_{out,in,in_out}.nt``."""
    with open(path, "r") as f:
        triples = f.read().splitlines()
    out_h, in_h, both = property_hashes(triples, legacy)
    for name, h in (("out", out_h), ("in", in_h), ("in_out", both)):
        write_sum_map_files(h, triples, f"{sum_path}{dataset}_sum_{name}.nt", f"{map_path}{dataset}_map_{name}.nt", legacy)


# ---- node partitions and quotient graphs on the GPU (csrc/rgcn_summary.hip) ------------------------------------------------
DIRECTIONS = ("out", "in", "in_out")
MAX_NODES = 2 ** 31 - 1        # node and block ids are int32 on the device
MAX_RELATIONS = 65536
MAX_KEYS = 0xFFFF0000          # edges (both ends of every edge for "in_out") one call sorts, counted in u32


class Partition(NamedTuple):
    block: "torch.Tensor"      # int64 [N] on the device: canonical block id of every node (ordered by smallest member)
    num_blocks: int
    rounds: int                # refinement rounds actually run
    counts: Tuple[int, ...]    # number of blocks after every round
    converged: bool            # the last round changed nothing (refinement only splits: an unchanged count is the fixpoint)


def _check_coo(edge_index, edge_type, num_nodes: int, num_relations: Optional[int], keys_per_edge: int = 1):
    """Shapes, dtypes, limits and id ranges of an int64 COO; returns (E, largest edge type or -1).  Raises before anything
    reaches the library.  The range checks read the tensors where they live."""
    import torch
    if not (torch.is_tensor(edge_index) and torch.is_tensor(edge_type)):
        raise ValueError("edge_index and edge_type must be tensors")
    if edge_index.dtype != torch.int64 or edge_type.dtype != torch.int64:
        raise ValueError(f"edge_index and edge_type must be int64 (got {edge_index.dtype}, {edge_type.dtype})")
    if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_type.dim() != 1 or edge_type.shape[0] != edge_index.shape[1]:
        raise ValueError(f"edge_index must be [2, E] and edge_type [E] (got {tuple(edge_index.shape)}, {tuple(edge_type.shape)})")
    if edge_index.device != edge_type.device:
        raise ValueError("edge_index and edge_type must live on one device")
    if isinstance(num_nodes, bool) or not isinstance(num_nodes, int) or not 1 <= num_nodes <= MAX_NODES:
        raise ValueError(f"num_nodes must be an int in 1 .. 2^31 - 1 (got {num_nodes!r})")
    if num_relations is not None and (isinstance(num_relations, bool) or not isinstance(num_relations, int)
                                      or not 1 <= num_relations <= MAX_RELATIONS):
        raise ValueError(f"num_relations must be an int in 1 .. {MAX_RELATIONS} (got {num_relations!r})")
    e = int(edge_type.shape[0])
    if e * keys_per_edge > MAX_KEYS:
        raise ValueError(f"{e} edges ({keys_per_edge} key(s) each) pass the {MAX_KEYS} keys one call sorts")
    tmax = -1
    if e:
        lo, hi = int(edge_index.min()), int(edge_index.max())
        if lo < 0 or hi >= num_nodes:
            raise ValueError(f"edge_index holds node ids in [{lo}, {hi}], outside [0, {num_nodes})")
        tlo, tmax = int(edge_type.min()), int(edge_type.max())
        top = MAX_RELATIONS if num_relations is None else num_relations
        if tlo < 0 or tmax >= top:
            raise ValueError(f"edge_type holds relation ids in [{tlo}, {tmax}], outside [0, {top})")
    return e, tmax


def _check_block(block, num_nodes: int, device, what: str) -> int:
    """an int64 [N] block vector on ``device`` with ids in [0, 2^31 - 1); returns its largest id"""
    import torch
    if not torch.is_tensor(block) or block.dtype != torch.int64 or block.dim() != 1 or block.shape[0] != num_nodes:
        raise ValueError(f"{what} must be an int64 tensor of shape [{num_nodes}]")
    if block.device != device:
        raise ValueError(f"{what} must live on the graph's device ({device})")
    lo, hi = int(block.min()), int(block.max())
    if lo < 0 or hi >= MAX_NODES:
        raise ValueError(f"{what} holds block ids in [{lo}, {hi}], outside [0, 2^31 - 1)")
    return hi


def _need_gpu(t, what: str) -> None:
    if t.device.type != "cuda":
        raise RuntimeError(f"{what}: the graph must live on the GPU (tensors are on {t.device}); there is no CPU path")


def node_partition(edge_index, edge_type, num_nodes: int, num_relations: int, *, k: Optional[int] = 1, direction: str = "out",
                   initial=None, max_rounds: int = 64, _route: int = 0) -> Partition:
    """k rounds of partition refinement of the nodes (``k=None``: until nothing changes, at most ``max_rounds`` rounds).

    A round maps a partition b to b': two nodes share a block of b' iff they share one of b AND have the same SET S(i):
    ``"out"``: {(type_e, b[dst_e]) : src_e = i}; ``"in"``: {(type_e, b[src_e]) : dst_e = i}; ``"in_out"``: both, every element
    tagged with its direction.  Duplicate edges and their order do not matter, self-loops are ordinary edges.  After every round
    the ids are 0 .. B - 1 in the order of the smallest node of every block.  ``initial`` (int64 [N], default: one block) is
    only ever refined.  The loop stops at the first round that leaves B unchanged (``converged``).  ``edge_index`` may be
    strided (rows of a transposed [E, 3] tensor).  ``_route``: 0 lets the library choose between its one-sort and two-sort
    key routes, 1 / 2 pin one (tests)."""
    import torch
    from . import _lib
    if direction not in DIRECTIONS:
        raise ValueError(f"direction must be one of {DIRECTIONS} (got {direction!r})")
    if k is not None and (isinstance(k, bool) or not isinstance(k, int) or k < 1):
        raise ValueError(f"k must be None or an int >= 1 (got {k!r})")
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, int) or max_rounds < 1:
        raise ValueError(f"max_rounds must be an int >= 1 (got {max_rounds!r})")
    if _route not in (0, 1, 2):
        raise ValueError(f"_route must be 0, 1 or 2 (got {_route!r})")
    e, _ = _check_coo(edge_index, edge_type, num_nodes, num_relations, 2 if direction == "in_out" else 1)
    dev = edge_index.device
    top = 0 if initial is None else _check_block(initial, num_nodes, dev, "initial")
    _need_gpu(edge_index, "node_partition")

    d = _lib.SUMMARY_DIRECTIONS[direction]
    graph, keep = _lib.graph_struct(edge_index, edge_type, num_nodes, num_relations)
    ws = _lib.summary_workspace(e, num_nodes, d, dev)
    cur = torch.zeros(num_nodes, dtype=torch.int32, device=dev) if initial is None else initial.to(torch.int32)
    nxt = torch.empty_like(cur)
    nb = 1
    if initial is not None:      # an edge-less round numbers the caller's blocks canonically and counts them
        no_edges = _lib.RgcnGraphStruct(None, None, None, 1, 1, 1, 0, num_nodes, num_relations)
        nb = _lib.summary_round(no_edges, d, cur, top + 1, nxt, ws)
        cur, nxt = nxt, cur
    counts, converged = [], False
    for _ in range(k if k is not None else max_rounds):
        new = _lib.summary_round(graph, d, cur, nb, nxt, ws, _route)
        cur, nxt = nxt, cur
        counts.append(new)
        converged = new == nb
        nb = new
        if converged:
            break
    del keep
    return Partition(cur.long(), nb, len(counts), tuple(counts), converged)


def quotient_graph(edge_index, edge_type, block, num_blocks: int, *, dedup: bool = True, _route: int = 0):
    """The graph of the blocks: ``(edge_index_s [2, E_s], edge_type_s [E_s], multiplicity [E_s])``, int64, on the device.
    ``dedup=True``: the distinct ``(block[src], type, block[dst])`` triples sorted by (type, dst block, src block), each with the
    number of edges behind it.  ``dedup=False``: ``block[edge_index]`` -- one summary edge per original edge in the original
    order, what the reference's summary files hold -- with multiplicity 1."""
    import torch
    from . import _lib
    if not torch.is_tensor(block) or block.dim() != 1:
        raise ValueError("block must be an int64 tensor of shape [N]")
    n = int(block.shape[0])
    if isinstance(num_blocks, bool) or not isinstance(num_blocks, int) or not 1 <= num_blocks <= MAX_NODES:
        raise ValueError(f"num_blocks must be an int in 1 .. 2^31 - 1 (got {num_blocks!r})")
    if _route not in (0, 1, 2):
        raise ValueError(f"_route must be 0, 1 or 2 (got {_route!r})")
    e, tmax = _check_coo(edge_index, edge_type, n, None)
    dev = edge_index.device
    if _check_block(block, n, dev, "block") >= num_blocks:
        raise ValueError(f"block holds ids outside [0, {num_blocks})")
    _need_gpu(edge_index, "quotient_graph")
    if not dedup:
        return block[edge_index], edge_type.clone(), torch.ones(e, dtype=torch.int64, device=dev)
    graph, keep = _lib.graph_struct(edge_index, edge_type, n, tmax + 1 if e else 1)
    ws = _lib.summary_workspace(e, n, _lib.SUMMARY_DIRECTIONS["out"], dev)
    out = _lib.summary_quotient(graph, block.to(torch.int32), num_blocks, ws, _route)
    del keep
    return out
