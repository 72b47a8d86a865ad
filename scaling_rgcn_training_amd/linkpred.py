"""Link prediction on the R-GCN encoder: the ``DistMult`` decoder, ``corrupt`` negatives and filtered ``ranks`` on
the kernels of csrc/rgcn_linkpred.hip, with the plumbing both frameworks' examples have around them (PyG ``rgcn_link_pred.py``,
DGL ``link.py``): ``with_inverse_edges`` for the encoder's graph, ``FilterIndex`` for the known triples, ``metrics`` for MRR and
Hits@k.  The encoder is any model that returns ``z [N, dim]``, e.g. ``Emb_Layers(2 R, hidden, dim, N, emb)`` with
``activation=do_nothing``.  The hot paths have no torch fallback: tensors that are not on the GPU are refused."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch
from torch import Tensor, nn

from . import _lib

MAX_WIDTH = 128


def _padded(t: Tensor) -> Tensor:
    """``t [rows, E]`` as the kernels read it: fp32, last dimension contiguous, row stride a multiple of 4, base 16-byte aligned.
    Returned as it is when it already lies that way (every width that is a multiple of 4), else copied into padded rows."""
    if t.dtype != torch.float32 or t.dim() != 2:
        raise ValueError(f"expected a [rows, width] float32 tensor (got {tuple(t.shape)}, {t.dtype})")
    if not 1 <= t.shape[1] <= MAX_WIDTH:
        raise ValueError(f"widths 1..{MAX_WIDTH} only (got {t.shape[1]}); DESIGN.md 18")
    if (t.shape[1] == 1 or t.stride(1) == 1) and t.stride(0) % 4 == 0 and t.stride(0) >= t.shape[1] and t.data_ptr() % 16 == 0:
        return t
    buf = torch.zeros(t.shape[0], (t.shape[1] + 3) // 4 * 4, dtype=torch.float32, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def _ids(name: str, t: Tensor, dev=None) -> Tensor:
    if not torch.is_tensor(t) or t.dim() != 1 or t.dtype != torch.int64:
        raise ValueError(f"{name} must be a 1-d int64 tensor")
    if dev is not None and t.device != dev:
        raise ValueError(f"{name} lives on {t.device}, the embeddings on {dev}")
    return t.contiguous()


def _triples(s: Tensor, r: Tensor, o: Tensor, dev=None) -> Tuple[Tensor, Tensor, Tensor]:
    s, r, o = _ids("s", s, dev), _ids("r", r, dev), _ids("o", o, dev)
    if not (s.shape == r.shape == o.shape) or s.device != r.device or s.device != o.device:
        raise ValueError(f"s, r, o must have one length and one device (got {tuple(s.shape)}, {tuple(r.shape)}, {tuple(o.shape)})")
    return s, r, o


class _DistMultFunction(torch.autograd.Function):
    """rgcn_lp_score forward; rgcn_lp_index_build + rgcn_lp_backward backward.  The index is built in the backward, so at most once per
    forward / backward pair and only when a gradient is wanted, and only the halves the wanted gradients need."""

    @staticmethod
    def forward(ctx, z, rel, s, r, o, bad, builds):
        zp, rp = _padded(z.detach()), _padded(rel.detach())
        ctx.save_for_backward(zp, rp, s, r, o)
        ctx.bad, ctx.builds = bad, builds
        return _lib.lp_score(zp, rp, s, r, o, bad)

    @staticmethod
    def backward(ctx, g):
        zp, rp, s, r, o = ctx.saved_tensors
        need_z, need_rel = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dz = drel = None
        if need_z or need_rel:
            ix = _lib.lp_index_build(s, r, o, int(zp.shape[0]), int(rp.shape[0]), ctx.bad, nodes=need_z, relations=need_rel)
            ctx.builds["node"] += int(need_z)
            ctx.builds["relation"] += int(need_rel)
            dz, drel = _lib.lp_backward(zp, rp, s, r, o, g.contiguous(), ix, need_z, need_rel)
        return dz, drel, None, None, None, None, None


class DistMult(nn.Module):
    """``score(s, r, o) = sum_k z[s, k] rel[r, k] z[o, k]`` with one trainable row per relation.  ``rel`` is initialised with
    ``xavier_uniform_``, as PyG's example decoder is.  Ids out of range score 0, get no gradient and are reported by ``check()``."""

    def __init__(self, num_relations: int, dim: int):
        super().__init__()
        if isinstance(num_relations, bool) or not isinstance(num_relations, int) or not 1 <= num_relations <= 65536:
            raise ValueError(f"num_relations must be an int in 1..65536 (got {num_relations!r})")
        if isinstance(dim, bool) or not isinstance(dim, int) or not 1 <= dim <= MAX_WIDTH:
            raise ValueError(f"dim must be an int in 1..{MAX_WIDTH} (got {dim!r}); wider decoders are not built (DESIGN.md 18)")
        self.num_relations, self.dim = num_relations, dim
        self.rel = nn.Parameter(torch.empty(num_relations, dim))
        nn.init.xavier_uniform_(self.rel)
        self._bad: Optional[Tensor] = None
        self.index_builds = {"node": 0, "relation": 0}      # halves of the index built so far (tests, profiling)

    def _bad_word(self, dev) -> Tensor:
        if self._bad is None or self._bad.device != dev:
            self._bad = torch.zeros(1, dtype=torch.int32, device=dev)
        return self._bad

    def forward(self, z: Tensor, s: Tensor, r: Tensor, o: Tensor) -> Tensor:
        if not torch.is_tensor(z) or z.dim() != 2 or z.shape[1] != self.dim or z.dtype != torch.float32:
            raise ValueError(f"z must be float32 [N, {self.dim}] (got {tuple(z.shape) if torch.is_tensor(z) else type(z)})")
        if z.device != self.rel.device:
            raise ValueError(f"z lives on {z.device}, the decoder on {self.rel.device}")
        s, r, o = _triples(s, r, o, z.device)
        return _DistMultFunction.apply(z, self.rel, s, r, o, self._bad_word(z.device), self.index_builds)

    def check(self) -> None:
        """Raise if a call since the last ``check()`` met an id out of range.  Reads one word back: SYNCHRONISES."""
        if self._bad is None:
            return
        word = int(self._bad.item())
        if word:
            self._bad.zero_()
            what = [n for bit, n in ((_lib.LP_BAD_NODE, "a node id outside [0, N)"), (_lib.LP_BAD_REL, "a relation id outside [0, R)"))
                    if word & bit]
            raise ValueError("DistMult: " + " and ".join(what) + " (such triples scored 0 and got no gradient)")


def corrupt(s: Tensor, r: Tensor, o: Tensor, num_nodes: int, num_negatives: int, seed: int) -> Tuple[Tensor, Tensor, Tensor]:
    """``num_negatives`` negatives per triple: ``(s', r', o')``, each ``[T * num_negatives]``, position ``i * num_negatives + j``
    being triple i with its subject or its object replaced by a node drawn from the generator at ``(seed, i, j)``.  A pure function
    of its arguments.  Negatives are NOT filtered against true triples (nor do PyG's and DGL's examples)."""
    s, r, o = _triples(s, r, o)
    for name, v, lo in (("num_nodes", num_nodes, 1), ("num_negatives", num_negatives, 1), ("seed", seed, 0)):
        if isinstance(v, bool) or not isinstance(v, int) or v < lo:
            raise ValueError(f"{name} must be an int >= {lo} (got {v!r})")
    if num_nodes >= 2 ** 31 or seed >= 2 ** 63:
        raise ValueError("num_nodes < 2^31 and seed < 2^63")
    return _lib.lp_corrupt(s, r, o, num_nodes, num_negatives, seed)


def with_inverse_edges(edge_index: Tensor, edge_type: Tensor, num_relations: int) -> Tuple[Tensor, Tensor]:
    """The graph both frameworks feed the encoder: every edge (u, t, v) and its inverse (v, t + R, u), 2 R relations.  Plain
    torch, built once per graph."""
    if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_type.dim() != 1 or edge_type.shape[0] != edge_index.shape[1]:
        raise ValueError(f"edge_index [2, E] and edge_type [E] (got {tuple(edge_index.shape)}, {tuple(edge_type.shape)})")
    if isinstance(num_relations, bool) or not isinstance(num_relations, int) or num_relations < 1:
        raise ValueError(f"num_relations must be an int >= 1 (got {num_relations!r})")
    return torch.cat([edge_index, edge_index.flip(0)], dim=1), torch.cat([edge_type, edge_type + num_relations])


class FilterIndex:
    """The known triples of a dataset (train + valid + test), indexed once with torch ops (``sort`` / ``searchsorted``; built once
    per dataset, not a hot path): for a query (anchor, r) the entities that complete it to a known triple, on the object side
    (s, r, ?) and on the subject side (?, r, o).  ``lists`` cuts the CSR lists of a batch of queries, distinct ids per list, which
    ``ranks`` hands to the kernel."""

    def __init__(self, known_triples: Tensor, num_nodes: int, num_relations: int):
        if not torch.is_tensor(known_triples) or known_triples.dim() != 2 or known_triples.shape[1] != 3 or known_triples.dtype != torch.int64:
            raise ValueError("known_triples must be an int64 [M, 3] tensor of (s, r, o) rows")
        s, r, o = known_triples[:, 0], known_triples[:, 1], known_triples[:, 2]
        if known_triples.shape[0] and (int(torch.min(torch.minimum(s, o))) < 0 or int(torch.max(torch.maximum(s, o))) >= num_nodes
                                       or int(r.min()) < 0 or int(r.max()) >= num_relations):
            raise ValueError("known_triples holds an id out of range")
        self.num_nodes, self.num_relations = int(num_nodes), int(num_relations)
        self._sides = {"object": self._build(s * num_relations + r, o), "subject": self._build(o * num_relations + r, s)}

    @staticmethod
    def _build(key: Tensor, idx: Tensor):
        order = torch.argsort(idx, stable=True)
        order = order[torch.argsort(key[order], stable=True)]       # by (key, idx)
        key, idx = key[order], idx[order]
        if key.numel():
            keep = torch.ones_like(key, dtype=torch.bool)
            keep[1:] = (key[1:] != key[:-1]) | (idx[1:] != idx[:-1])
            key, idx = key[keep], idx[keep]
        ukey, counts = torch.unique_consecutive(key, return_counts=True)
        ptr = torch.zeros(ukey.numel() + 1, dtype=torch.int64, device=key.device)
        ptr[1:] = torch.cumsum(counts, 0)
        return ukey, ptr, idx.contiguous()

    def to(self, device) -> "FilterIndex":
        self._sides = {k: tuple(t.to(device) for t in v) for k, v in self._sides.items()}
        return self

    def lists(self, s: Tensor, r: Tensor, o: Tensor, side: str = "object") -> Tuple[Tensor, Tensor]:
        """``(filter_ptr [Q + 1], filter_idx)`` int64 for the queries (s, r, ?) (``side="object"``) or (?, r, o) (``"subject"``)"""
        if side not in self._sides:
            raise ValueError(f"side must be 'object' or 'subject' (got {side!r})")
        ukey, ptr, idx = self._sides[side]
        s, r, o = _triples(s, r, o, ukey.device)
        key = (s if side == "object" else o) * self.num_relations + r
        q = key.numel()
        out_ptr = torch.zeros(q + 1, dtype=torch.int64, device=key.device)
        if q == 0 or ukey.numel() == 0:
            return out_ptr, idx[:0]
        pos = torch.searchsorted(ukey, key).clamp_(max=ukey.numel() - 1)
        found = ukey[pos] == key
        length = torch.where(found, ptr[pos + 1] - ptr[pos], torch.zeros_like(pos))
        out_ptr[1:] = torch.cumsum(length, 0)
        total = int(out_ptr[-1])
        owner = torch.repeat_interleave(torch.arange(q, device=key.device), length, output_size=total)
        src = ptr[pos][owner] + (torch.arange(total, device=key.device) - out_ptr[:-1][owner])
        return out_ptr, idx[src].contiguous()


def ranks(z: Tensor, decoder: DistMult, s: Tensor, r: Tensor, o: Tensor, side: str = "object",
          filter: Optional[FilterIndex] = None) -> Tuple[Tensor, Tensor]:
    """``(greater, equal)`` int64 [Q]: for every test triple the candidates that score strictly above, and exactly like, its true
    object (``side="object"``: (s, r, ?)) or subject (``"subject"``: (?, r, o); DistMult is symmetric, the same kernel with the
    object as anchor), over all N entities but the true one and, with ``filter``, but every entity that completes the query to a
    known triple.  No [Q, N] scores exist anywhere.  A query with an id out of range gets (-1, -1)."""
    if side not in ("object", "subject"):
        raise ValueError(f"side must be 'object' or 'subject' (got {side!r})")
    if not isinstance(decoder, DistMult):
        raise ValueError("ranks scores with a DistMult decoder")
    if filter is not None and not isinstance(filter, FilterIndex):
        raise ValueError("filter must be a FilterIndex or None")
    if not torch.is_tensor(z) or z.dim() != 2 or z.shape[1] != decoder.dim:
        raise ValueError(f"z must be [N, {decoder.dim}]")
    s, r, o = _triples(s, r, o, z.device)
    fptr = fidx = None
    if filter is not None:
        if filter.num_nodes != z.shape[0] or filter.num_relations != decoder.num_relations:
            raise ValueError("the filter was built for another number of nodes or relations")
        fptr, fidx = filter.lists(s, r, o, side)
    anchor, target = (s, o) if side == "object" else (o, s)
    return _lib.lp_rank(_padded(z.detach()), _padded(decoder.rel.detach()), anchor, r, target, fptr, fidx)


def metrics(greater: Tensor, equal: Tensor, ks: Sequence[int] = (1, 3, 10), ties: str = "mean") -> Dict[str, float]:
    """MRR and Hits@k from rank counts.  ``ties="mean"``: rank = 1 + greater + equal / 2, the expected rank under a random order of
    the tied candidates; ``"optimistic"``: rank = 1 + greater."""
    if ties not in ("mean", "optimistic"):
        raise ValueError(f"ties must be 'mean' or 'optimistic' (got {ties!r})")
    if greater.shape != equal.shape or greater.dim() != 1:
        raise ValueError("greater and equal must be vectors of one length")
    if greater.numel() == 0:
        raise ValueError("no queries")
    if int(greater.min()) < 0 or int(equal.min()) < 0:
        raise ValueError("a query had an id out of range (negative count)")
    rank = 1.0 + greater.to(torch.float64) + (equal.to(torch.float64) / 2 if ties == "mean" else 0.0)
    out = {"mrr": float((1.0 / rank).mean())}
    for k in ks:
        out[f"hits@{int(k)}"] = float((rank <= k).to(torch.float64).mean())
    return out
