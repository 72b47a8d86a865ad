"""Reference of neighbour sampling with one fan-out PER RELATION, written from its specification and independent of
csrc/rgcn_sample.hip: the relation index (edges sorted stably by (destination, relation), cut into runs), Floyd's k-subset of a run
on the generator keyed by (seed, hop, destination, relation) in Python integers (``floyd_rel``), the blocks and the multi-layer
driver in torch on the device of the tensors given (the CPU in the tests).  The generator, ``Block`` and the test graphs are those
of tests/sampling_reference.py; int entries of ``fanouts`` go to its ``sample_block``.

``vectorised=True`` replaces the per-unit Python loop by the same draws in torch int64 arithmetic, Floyd's j loop over all sampled
units at once, each with its own k: the form tools/sampling_rel_timing.py times on the GPU against the HIP hop.
tests/test_sampling_rel_reference.py holds the two forms equal.
"""
from typing import List, NamedTuple, Sequence

import torch

from tests.sampling_reference import MAX_FANOUT, Block, Index, _lsr, _mix_t, _s64, hop_key, hub_graph, mix, sample_block

REL_MUL = 0xD1B54A32D192ED03

__all__ = ["RelIndex", "build_rel_index", "floyd_rel", "floyd_rel_torch", "sample_block_rel", "sample_rel", "Block", "hub_graph", "mix",
           "hop_key"]


class RelIndex(NamedTuple):
    run_ptr: torch.Tensor         # int64 [N + 1]: the runs of node v are run_ptr[v] .. run_ptr[v + 1], ascending in relation
    run_beg: torch.Tensor         # int64 [num_runs + 1]: the positions of run q in the sorted edge list
    run_type: torch.Tensor        # int64 [num_runs]
    src: torch.Tensor             # int64 [E]: sources of the edges sorted stably by (destination, relation)
    num_nodes: int
    num_relations: int
    num_runs: int


def build_rel_index(edge_index: torch.Tensor, edge_type: torch.Tensor, num_nodes: int, num_relations: int) -> RelIndex:
    dev = edge_type.device
    key = edge_index[1].long() * num_relations + edge_type.long()
    order = torch.sort(key, stable=True).indices
    key = key[order]
    e = int(key.shape[0])
    head = torch.ones(e, dtype=torch.bool, device=dev)
    head[1:] = key[1:] != key[:-1]
    first = torch.nonzero(head).flatten()
    run_beg = torch.cat([first, torch.tensor([e], dtype=torch.int64, device=dev)])
    run_key = key[first]
    run_ptr = torch.zeros(num_nodes + 1, dtype=torch.int64, device=dev)
    run_ptr[1:] = torch.cumsum(torch.bincount(run_key // num_relations, minlength=num_nodes), 0)
    return RelIndex(run_ptr, run_beg, run_key % num_relations, edge_index[0].long()[order], num_nodes, num_relations,
                    int(first.shape[0]))


# ---- the generator, keyed per relation as well ---------------------------------------------------------------------------------
def rel_key(seed: int, hop: int, v: int, t: int) -> int:
    return mix(mix(hop_key(seed, hop) + v) + REL_MUL * (t + 1))


def floyd_rel(d: int, k: int, seed: int, hop: int, v: int, t: int) -> List[int]:
    """the ascending k-subset of 0 .. d-1 the run of destination ``v`` (global id) and relation ``t`` takes in hop ``hop`` (d > k >= 1)"""
    kv, chosen = rel_key(seed, hop, v, t), set()
    for j in range(d - k, d):
        r = mix(kv + j)
        x = ((r >> 32) * (j + 1)) >> 32
        chosen.add(j if x in chosen else x)
    return sorted(chosen)


def floyd_rel_torch(d: torch.Tensor, k: torch.Tensor, seed: int, hop: int, v: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """[n, max k] : row i holds ``floyd_rel(d[i], k[i], ..., v[i], t[i])`` in its first k[i] columns, then a filler past every position"""
    big = 1 << 62
    kv = _mix_t(_mix_t(v + _s64(hop_key(seed, hop))) + (t + 1) * _s64(REL_MUL))
    kmax = int(k.max())
    chosen = torch.full((int(d.shape[0]), kmax), big, dtype=torch.int64, device=d.device)
    for s in range(kmax):
        live = k > s
        j = d - k + s
        r = _mix_t(kv + j)
        dr = _lsr(_lsr(r, 32) * (j + 1), 32)
        hit = (chosen == dr[:, None]).any(1)
        chosen[:, s] = torch.where(live, torch.where(hit, j, dr), torch.full_like(j, big))
    return chosen.sort(1).values


# ---- blocks, layers ----------------------------------------------------------------------------------------------------------------
def check_rel_fanout(k: Sequence[int], num_relations: int) -> None:
    assert len(k) == num_relations and all(isinstance(x, int) and (-1 <= x <= MAX_FANOUT) for x in k)


def sample_block_rel(index: RelIndex, dst_nodes: torch.Tensor, k: Sequence[int], seed: int, hop: int,
                     vectorised: bool = False) -> Block:
    check_rel_fanout(k, index.num_relations)
    dev = index.run_ptr.device
    n_dst = int(dst_nodes.shape[0])
    fan = torch.tensor(list(k), dtype=torch.int64, device=dev)
    # units: the runs of the destinations, by destination position, then relation
    first_run = index.run_ptr[dst_nodes]
    n_run = index.run_ptr[dst_nodes + 1] - first_run
    uoff = torch.cumsum(n_run, 0) - n_run
    udst = torch.repeat_interleave(torch.arange(n_dst, device=dev), n_run)
    n_units = int(udst.shape[0])
    q = first_run[udst] + torch.arange(n_units, device=dev) - uoff[udst]
    begin = index.run_beg[q]
    d = index.run_beg[q + 1] - begin
    t = index.run_type[q]
    ku = fan[t]
    cnt = torch.where(ku < 0, d, torch.minimum(d, ku))
    eoff = torch.cumsum(cnt, 0) - cnt
    unit = torch.repeat_interleave(torch.arange(n_units, device=dev), cnt)
    pos = torch.arange(int(unit.shape[0]), device=dev) - eoff[unit]      # units taken whole: every edge of the run, in order
    sampled = torch.nonzero((ku > 0) & (d > ku)).flatten()
    if sampled.numel():
        ds, ks, vs, ts = d[sampled], ku[sampled], dst_nodes[udst[sampled]], t[sampled]
        if vectorised:
            chosen = floyd_rel_torch(ds, ks, seed, hop, vs, ts)
            keep = torch.arange(chosen.shape[1], device=dev)[None, :] < ks[:, None]
            flat = chosen[keep]                                         # (row-major: unit by unit, ascending)
        else:
            flat = torch.tensor([p for di, ki, vi, ti in zip(ds.tolist(), ks.tolist(), vs.tolist(), ts.tolist())
                                 for p in floyd_rel(di, ki, seed, hop, vi, ti)], dtype=torch.int64, device=dev)
        where_e = torch.repeat_interleave(eoff[sampled], ks) + (torch.arange(int(flat.shape[0]), device=dev)
                                                                - torch.repeat_interleave(torch.cumsum(ks, 0) - ks, ks))
        pos[where_e] = flat
    g = begin[unit] + pos
    s = index.src[g]
    where = torch.full((index.num_nodes,), -1, dtype=torch.int64, device=dev)
    where[dst_nodes] = torch.arange(n_dst, device=dev)
    new = torch.unique(s[where[s] < 0])      # (sorted ascending)
    where[new] = n_dst + torch.arange(int(new.shape[0]), device=dev)
    src_nodes = torch.cat([dst_nodes, new])
    return Block(torch.stack([where[s], udst[unit]]), t[unit], int(src_nodes.shape[0]), n_dst, src_nodes)


def sample_rel(index: Index, rel_index: RelIndex, seeds: torch.Tensor, fanouts: Sequence, seed: int = 0,
               vectorised: bool = False) -> List[Block]:
    """blocks[0 .. L-1]; fanouts[i] (an int: tests/sampling_reference.sample_block on ``index``; a sequence: one fan-out per
    relation, on ``rel_index``) and hop = i belong to model layer i; sampled from the last layer back"""
    blocks, dst = [], seeds
    for i in reversed(range(len(fanouts))):
        if isinstance(fanouts[i], int):
            b = sample_block(index, dst, fanouts[i], seed, i, vectorised)
        else:
            b = sample_block_rel(rel_index, dst, fanouts[i], seed, i, vectorised)
        blocks.append(b)
        dst = b.src_nodes
    return blocks[::-1]

