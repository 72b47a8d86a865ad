"""The oracle of scaling_rgcn_training_amd.summaries.node_partition / quotient_graph: the same semantics with Python sets and
tuples -- no hashing, no sorting of packed keys, nothing shared with the kernels.  CPU only.

One round maps a partition b to b': nodes share a block of b' iff they share one of b and have the same SET
  out:    {(type_e, b[dst_e]) : src_e = i}
  in:     {(type_e, b[src_e]) : dst_e = i}
  in_out: {(0, type_e, b[dst_e]) : src_e = i} | {(1, type_e, b[src_e]) : dst_e = i}
Blocks are numbered 0 .. B - 1 by their smallest node.  The loop stops after the first round that leaves the number of blocks
unchanged (refinement only splits, so nothing changed).

``node_partition_sparse`` is the same oracle for graphs of 2^24 nodes and a few thousand edges, where one set per node is too
much: sets only for the nodes that own an edge, still from the semantics above and with nothing of the kernels in it."""
from collections import Counter, namedtuple

import numpy as np
import torch

Partition = namedtuple("Partition", "block num_blocks rounds counts converged")


def canonical(labels):
    """ids 0 .. B - 1 in the order of first appearance = order of the smallest node of every block"""
    ids = {}
    return [ids.setdefault(lab, len(ids)) for lab in labels], len(ids)


def refine_once(src, dst, typ, n, block, direction):
    sets = [set() for _ in range(n)]
    for s, d, t in zip(src, dst, typ):
        if direction == "out":
            sets[s].add((t, block[d]))
        elif direction == "in":
            sets[d].add((t, block[s]))
        else:
            sets[s].add((0, t, block[d]))
            sets[d].add((1, t, block[s]))
    return canonical([(block[i], frozenset(sets[i])) for i in range(n)])


def node_partition(edge_index, edge_type, num_nodes, num_relations=None, *, k=1, direction="out", initial=None, max_rounds=64):
    assert direction in ("out", "in", "in_out") and (k is None or k >= 1)
    src, dst, typ = edge_index[0].tolist(), edge_index[1].tolist(), edge_type.tolist()
    block, nb = canonical([0] * num_nodes if initial is None else initial.tolist())
    counts, converged = [], False
    for _ in range(k if k is not None else max_rounds):
        block, new = refine_once(src, dst, typ, num_nodes, block, direction)
        counts.append(new)
        converged = new == nb
        nb = new
        if converged:
            break
    return Partition(torch.tensor(block, dtype=torch.int64), nb, len(counts), tuple(counts), converged)


def canonical_array(labels):
    """``canonical`` for a numpy int64 array: the distinct labels numbered by the position of their first occurrence"""
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(order.shape[0])
    return rank[inverse.reshape(-1)], int(order.shape[0])


def refine_once_sparse(src, dst, typ, block, direction):
    """``refine_once`` with a set only for the nodes that own an edge: every distinct set gets a small id (the empty set 0), a
    node's label is the pair (block, set id) written as one integer"""
    bs, bd = block[src].tolist(), block[dst].tolist()
    sets = {}
    for e, (s, d, t) in enumerate(zip(src.tolist(), dst.tolist(), typ.tolist())):
        if direction == "out":
            sets.setdefault(s, set()).add((t, bd[e]))
        elif direction == "in":
            sets.setdefault(d, set()).add((t, bs[e]))
        else:
            sets.setdefault(s, set()).add((0, t, bd[e]))
            sets.setdefault(d, set()).add((1, t, bs[e]))
    set_ids = {frozenset(): 0}
    set_id = np.zeros(block.shape[0], dtype=np.int64)
    for node, elements in sets.items():
        set_id[node] = set_ids.setdefault(frozenset(elements), len(set_ids))
    assert int(block.max()) < (1 << 62) // len(set_ids)
    return canonical_array(block * len(set_ids) + set_id)


def node_partition_sparse(edge_index, edge_type, num_nodes, num_relations=None, *, k=1, direction="out", initial=None,
                          max_rounds=64):
    """``node_partition`` for graphs of many nodes and few edges (2^24 nodes, some thousand edges): the same rounds, one Python
    set per node that owns an edge instead of one per node, the numbering in numpy.  tests/test_summary_reference.py holds the
    two equal."""
    assert direction in ("out", "in", "in_out") and (k is None or k >= 1)
    src, dst, typ = edge_index[0].numpy(), edge_index[1].numpy(), edge_type.numpy()
    block, nb = canonical_array(np.zeros(num_nodes, dtype=np.int64) if initial is None else initial.numpy().astype(np.int64))
    counts, converged = [], False
    for _ in range(k if k is not None else max_rounds):
        block, new = refine_once_sparse(src, dst, typ, block, direction)
        counts.append(new)
        converged = new == nb
        nb = new
        if converged:
            break
    return Partition(torch.from_numpy(block.astype(np.int64)), nb, len(counts), tuple(counts), converged)


def quotient_graph(edge_index, edge_type, block):
    """distinct (block[src], type, block[dst]) with multiplicities, sorted by (type, dst block, src block)"""
    b = block.tolist()
    c = Counter((t, b[d], b[s]) for s, d, t in zip(edge_index[0].tolist(), edge_index[1].tolist(), edge_type.tolist()))
    keys = sorted(c)
    ei = torch.tensor([[k[2] for k in keys], [k[1] for k in keys]], dtype=torch.int64).reshape(2, -1)
    return ei, torch.tensor([k[0] for k in keys], dtype=torch.int64), torch.tensor([c[k] for k in keys], dtype=torch.int64)


def path_graph(n):
    """0 -> 1 -> ... -> n - 1, one relation"""
    return torch.stack([torch.arange(n - 1), torch.arange(1, n)]), torch.zeros(n - 1, dtype=torch.int64)


def random_graph(n, e, r, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, n, (2, e), generator=g), torch.randint(0, r, (e,), generator=g)


def hub_graph(deg=5000, lead=37):
    """Three hubs with `deg` leaves each (relation 0, hub -> leaf): H1 and H2 differ in ONE leaf, H3 has exactly H1's leaves with
    every seventh edge doubled.  `lead` edges on owners in front of the hubs push the hubs' key runs off every wave (64) and
    workgroup (256) boundary of the sorted keys.  `initial`: the hubs and the lead owners share block 0, every leaf has a block
    of its own.  After one "out" round H1 and H3 share a block and H2 does not: a partial sum dropped or counted twice where a
    run crosses a wave changes a hub's signature.  Returns (edge_index, edge_type, N, initial, (H1, H2, H3))."""
    h1, h2, h3 = lead, lead + 1, lead + 2           # node ids: lead owners 0 .. lead - 1, then the hubs, then the leaves
    leaf0 = lead + 3
    n = leaf0 + deg + 1
    leaves1 = list(range(leaf0, leaf0 + deg))
    leaves2 = leaves1[:-1] + [leaf0 + deg]          # one leaf swapped
    src = list(range(lead)) + [h1] * deg + [h2] * deg + [h3] * deg + [h3] * len(leaves1[::7])
    dst = [leaf0 + i for i in range(lead)] + leaves1 + leaves2 + leaves1 + leaves1[::7]
    perm = torch.randperm(len(src), generator=torch.Generator().manual_seed(11))
    ei = torch.tensor([src, dst], dtype=torch.int64)[:, perm]
    initial = torch.zeros(n, dtype=torch.int64)
    initial[leaf0:] = torch.arange(1, deg + 2)
    return ei, torch.zeros(ei.shape[1], dtype=torch.int64), n, initial, (h1, h2, h3)
