"""Reference of the neighbour sampler, written from its specification and independent of csrc/rgcn_sample.hip:
the counter-based draw and Floyd's k-subset in Python integers (``floyd``), the in-edge index, the blocks and the multi-layer
driver in torch on the device of the tensors given (the CPU in the tests).

``vectorised=True`` replaces the per-destination Python loop by the same draws in torch int64 arithmetic (wrapping multiplies,
logical shifts spelled out), Floyd's j loop over all sampled destinations at once: the form tools/sampling_timing.py times on the
GPU against the HIP hop.  tests/test_sampling_reference.py holds the two forms equal.
"""
from typing import List, NamedTuple, Sequence

import torch

M64 = (1 << 64) - 1
C1, C2, GOLDEN = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB, 0x9E3779B97F4A7C15
MAX_FANOUT = 256


class Block(NamedTuple):
    edge_index: torch.Tensor      # int64 [2, E_b]: positions in src_nodes (row 0) and in the destinations (row 1)
    edge_type: torch.Tensor       # int64 [E_b]
    n_src: int
    n_dst: int
    src_nodes: torch.Tensor       # int64 [n_src]: global ids; the first n_dst are the destinations


class Index(NamedTuple):
    ptr: torch.Tensor             # int64 [N + 1]
    src: torch.Tensor             # int64 [E]: sources of the edges sorted stably by destination
    type: torch.Tensor            # int64 [E]
    num_nodes: int


# ---- the generator, in Python integers ---------------------------------------------------------------------------------
def mix(z: int) -> int:
    z &= M64
    z ^= z >> 30
    z = (z * C1) & M64
    z ^= z >> 27
    z = (z * C2) & M64
    z ^= z >> 31
    return z


def hop_key(seed: int, hop: int) -> int:
    return mix(seed + GOLDEN * (hop + 1))


def draw(key: int, v: int, j: int) -> int:
    r = mix(mix(key + v) + j)
    return ((r >> 32) * (j + 1)) >> 32


def floyd(d: int, k: int, seed: int, hop: int, v: int) -> List[int]:
    """the ascending k-subset of 0 .. d-1 destination ``v`` (global id) takes in hop ``hop`` (d > k >= 1)"""
    key, chosen = hop_key(seed, hop), set()
    for j in range(d - k, d):
        t = draw(key, v, j)
        chosen.add(j if t in chosen else t)
    return sorted(chosen)


# ---- the same draws in torch int64 (two's complement: multiplies wrap, >> is arithmetic and is masked) -------------------------
def _s64(c: int) -> int:
    return c - (1 << 64) if c >= (1 << 63) else c


def _lsr(z: torch.Tensor, s: int) -> torch.Tensor:
    return (z >> s) & ((1 << (64 - s)) - 1)


def _mix_t(z: torch.Tensor) -> torch.Tensor:
    z = z ^ _lsr(z, 30)
    z = z * _s64(C1)
    z = z ^ _lsr(z, 27)
    z = z * _s64(C2)
    return z ^ _lsr(z, 31)


def floyd_torch(d: torch.Tensor, k: int, seed: int, hop: int, v: torch.Tensor) -> torch.Tensor:
    """[n, k] ascending positions: ``floyd`` for every (d[i], v[i]) at once"""
    kv = _mix_t(v + _s64(hop_key(seed, hop)))
    chosen = torch.full((int(d.shape[0]), k), -1, dtype=torch.int64, device=d.device)
    for t in range(k):
        j = d - k + t
        r = _mix_t(kv + j)
        dr = _lsr(_lsr(r, 32) * (j + 1), 32)
        hit = (chosen == dr[:, None]).any(1)
        chosen[:, t] = torch.where(hit, j, dr)
    return chosen.sort(1).values


# ---- index, blocks, layers ---------------------------------------------------------------------------------------------------
def build_index(edge_index: torch.Tensor, edge_type: torch.Tensor, num_nodes: int) -> Index:
    dst = edge_index[1].long()
    order = torch.sort(dst, stable=True).indices
    ptr = torch.zeros(num_nodes + 1, dtype=torch.int64, device=dst.device)
    ptr[1:] = torch.cumsum(torch.bincount(dst, minlength=num_nodes), 0)
    return Index(ptr, edge_index[0].long()[order], edge_type.long()[order], num_nodes)


def sample_block(index: Index, dst_nodes: torch.Tensor, k: int, seed: int, hop: int, vectorised: bool = False) -> Block:
    assert k == -1 or 1 <= k <= MAX_FANOUT
    dev = index.ptr.device
    n_dst = int(dst_nodes.shape[0])
    begin = index.ptr[dst_nodes]
    deg = index.ptr[dst_nodes + 1] - begin
    cnt = deg if k == -1 else deg.clamp(max=k)
    off = torch.cumsum(cnt, 0) - cnt
    owner = torch.repeat_interleave(torch.arange(n_dst, device=dev), cnt)
    pos = torch.arange(int(owner.shape[0]), device=dev) - off[owner]      # take-all destinations: every in-edge, in order
    if k != -1:
        sampled = torch.nonzero(deg > k).flatten()
        if sampled.numel():
            if vectorised:
                chosen = floyd_torch(deg[sampled], k, seed, hop, dst_nodes[sampled])
            else:
                chosen = torch.tensor([floyd(d, k, seed, hop, v) for d, v in zip(deg[sampled].tolist(), dst_nodes[sampled].tolist())],
                                      dtype=torch.int64, device=dev)
            pos[(off[sampled][:, None] + torch.arange(k, device=dev)).flatten()] = chosen.flatten()
    g = begin[owner] + pos
    s, t = index.src[g], index.type[g]
    where = torch.full((index.num_nodes,), -1, dtype=torch.int64, device=dev)
    where[dst_nodes] = torch.arange(n_dst, device=dev)
    new = torch.unique(s[where[s] < 0])      # (sorted ascending)
    where[new] = n_dst + torch.arange(int(new.shape[0]), device=dev)
    src_nodes = torch.cat([dst_nodes, new])
    return Block(torch.stack([where[s], owner]), t, int(src_nodes.shape[0]), n_dst, src_nodes)


def sample(index: Index, seeds: torch.Tensor, fanouts: Sequence[int], seed: int = 0, vectorised: bool = False) -> List[Block]:
    """blocks[0 .. L-1]; fanouts[i] and hop = i belong to model layer i; sampled from the last layer back"""
    blocks, dst = [], seeds
    for i in reversed(range(len(fanouts))):
        b = sample_block(index, dst, fanouts[i], seed, i, vectorised)
        blocks.append(b)
        dst = b.src_nodes
    return blocks[::-1]


# ---- test graphs -----------------------------------------------------------------------------------------------------------
def hub_graph(n: int, e: int, num_rel: int, seed: int, hub_edges: int = 0, empty_rel: bool = True):
    """random (edge_index [2, E], edge_type [E]): node 0 a hub of ``hub_edges`` in-edges, self loops, repeated triples, the last
    relation empty, the last 3 nodes without in-edges"""
    g = torch.Generator().manual_seed(seed)
    top = max(n - 3, 1)
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, top, (e,), generator=g)
    typ = torch.randint(0, max(num_rel - 1, 1) if empty_rel else num_rel, (e,), generator=g)
    if hub_edges:
        dst[torch.randperm(e, generator=g)[:hub_edges]] = 0
    m = min(e // 10, 50)
    if m:
        src[:m] = dst[:m]                                    # self loops
        src[m:2 * m], dst[m:2 * m], typ[m:2 * m] = src[2 * m:3 * m], dst[2 * m:3 * m], typ[2 * m:3 * m]      # repeated triples
    return torch.stack([src, dst]), typ


def triples(edge_index: torch.Tensor, edge_type: torch.Tensor) -> torch.Tensor:
    """[E, 3] (src, type, dst) rows sorted lexicographically: a multiset of triples in canonical form"""
    t = torch.stack([edge_index[0], edge_type, edge_index[1]], 1)
    for c in (2, 1, 0):
        t = t[torch.sort(t[:, c], stable=True).indices]
    return t
