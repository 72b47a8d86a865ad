"""Link prediction on the R-GCN encoder: the ``DistMult`` decoder, ``corrupt`` negatives and filtered ``ranks`` on
the kernels of csrc/rgcn_linkpred.hip, with the plumbing both frameworks' examples have around them (PyG ``rgcn_link_pred.py``,
DGL ``link.py``): ``with_inverse_edges`` for the encoder's graph, ``FilterIndex`` for the known triples, ``metrics`` for MRR and
Hits@k.  The encoder is any model that returns ``z [N, dim]``, e.g. ``Emb_Layers(2 R, hidden, dim, N, emb)`` with
``activation=do_nothing``.  ``ComplEx`` and ``TransE`` are the asymmetric decoders, on the kernels of csrc/rgcn_kge.hip:
the same index, negatives, filter and metrics serve them.  ``topk`` answers a query with its ``k`` best entities on the kernels of csrc/rgcn_lp_topk.hip.  ``softmax_loss`` is the 1-N training loss over all entities, on the kernels of
csrc/rgcn_lp_softmax.hip and, for a wide ``DistMult``, of csrc/rgcn_lp_softmax_wide.hip.  The hot paths have no torch fallback: tensors that are not on the GPU are refused."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch
from torch import Tensor, nn

from . import _lib

MAX_WIDTH = 128
WIDE_MAX_WIDTH = _lib.XWIDE_MAX_WIDTH      # DistMult(..., wide=True): the rgcn_lpw_* kernels


def _padded(t: Tensor, max_width: int = MAX_WIDTH) -> Tensor:
    """``t [rows, E]`` as the kernels read it: fp32, last dimension contiguous, row stride a multiple of 4, base 16-byte aligned.
    Returned as it is when it already lies that way (every width that is a multiple of 4), else copied into padded rows."""
    if t.dtype != torch.float32 or t.dim() != 2:
        raise ValueError(f"expected a [rows, width] float32 tensor (got {tuple(t.shape)}, {t.dtype})")
    if not 1 <= t.shape[1] <= max_width:
        raise ValueError(f"widths 1..{max_width} only (got {t.shape[1]}); DESIGN.md 18, 21")
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
    forward / backward pair and only when a gradient is wanted, and only the halves the wanted gradients need.  ``family``: "lp", or
    "lpw" for a wide decoder's rows of more than 128 columns (the index is the same)."""

    @staticmethod
    def forward(ctx, z, rel, s, r, o, bad, builds, family):
        limit = WIDE_MAX_WIDTH if family == "lpw" else MAX_WIDTH
        zp, rp = _padded(z.detach(), limit), _padded(rel.detach(), limit)
        ctx.save_for_backward(zp, rp, s, r, o)
        ctx.bad, ctx.builds, ctx.family = bad, builds, family
        return _lib.lp_score(zp, rp, s, r, o, bad, family=family)

    @staticmethod
    def backward(ctx, g):
        zp, rp, s, r, o = ctx.saved_tensors
        need_z, need_rel = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dz = drel = None
        if need_z or need_rel:
            ix = _lib.lp_index_build(s, r, o, int(zp.shape[0]), int(rp.shape[0]), ctx.bad, nodes=need_z, relations=need_rel)
            ctx.builds["node"] += int(need_z)
            ctx.builds["relation"] += int(need_rel)
            dz, drel = _lib.lp_backward(zp, rp, s, r, o, g.contiguous(), ix, need_z, need_rel, family=ctx.family)
        return dz, drel, None, None, None, None, None, None


class DistMult(nn.Module):
    """``score(s, r, o) = sum_k z[s, k] rel[r, k] z[o, k]`` with one trainable row per relation.  ``rel`` is initialised with
    ``xavier_uniform_``, as PyG's example decoder is.  Ids out of range score 0, get no gradient and are reported by ``check()``.
    ``wide=True`` allows ``dim`` up to 512 (``None``: ``conv``'s import-time ``RGCN_WIDE`` default, as ``RGCNConv`` takes it): a
    ``dim`` above 128 runs on csrc/rgcn_linkpred_wide.hip, a wide decoder of at most 128 on the kernels of a narrow
    one, bit for bit."""

    def __init__(self, num_relations: int, dim: int, wide: Optional[bool] = None):
        super().__init__()
        if isinstance(num_relations, bool) or not isinstance(num_relations, int) or not 1 <= num_relations <= 65536:
            raise ValueError(f"num_relations must be an int in 1..65536 (got {num_relations!r})")
        if wide is None:
            from .conv import _WIDE_DEFAULT
            wide = _WIDE_DEFAULT
        if not isinstance(wide, bool):
            raise ValueError(f"wide must be a bool or None (got {wide!r})")
        limit = WIDE_MAX_WIDTH if wide else MAX_WIDTH
        if isinstance(dim, bool) or not isinstance(dim, int) or not 1 <= dim <= limit:
            raise ValueError(f"dim must be an int in 1..{limit} (got {dim!r}); wide=True allows 1..{WIDE_MAX_WIDTH} (DESIGN.md 21)")
        self.num_relations, self.dim, self.wide = num_relations, dim, wide
        self.family = "lpw" if dim > MAX_WIDTH else "lp"      # the kernels that serve this width
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
        return _DistMultFunction.apply(z, self.rel, s, r, o, self._bad_word(z.device), self.index_builds, self.family)

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


class _KgeFunction(torch.autograd.Function):
    """rgcn_kge_score forward; rgcn_lp_index_build + rgcn_kge_backward backward, as ``_DistMultFunction`` does it: the index is a
    function of the ids alone, so it is the same one, built in the backward and only the halves the wanted gradients need."""

    @staticmethod
    def forward(ctx, z, rel, s, r, o, bad, builds, code):
        zp, rp = _padded(z.detach()), _padded(rel.detach())
        ctx.save_for_backward(zp, rp, s, r, o)
        ctx.bad, ctx.builds, ctx.code = bad, builds, code
        return _lib.kge_score(code, zp, rp, s, r, o, bad)

    @staticmethod
    def backward(ctx, g):
        zp, rp, s, r, o = ctx.saved_tensors
        need_z, need_rel = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dz = drel = None
        if need_z or need_rel:
            ix = _lib.lp_index_build(s, r, o, int(zp.shape[0]), int(rp.shape[0]), ctx.bad, nodes=need_z, relations=need_rel)
            ctx.builds["node"] += int(need_z)
            ctx.builds["relation"] += int(need_rel)
            dz, drel = _lib.kge_backward(ctx.code, zp, rp, s, r, o, g.contiguous(), ix, need_z, need_rel)
        return dz, drel, None, None, None, None, None, None


class _KgeDecoder(nn.Module):
    """What ``ComplEx`` and ``TransE`` share: one trainable row per relation (``xavier_uniform_``), the ``bad`` word and
    ``check()``, ``index_builds``, and a forward on the kernels of csrc/rgcn_kge.hip.  ``dim`` is 1..128."""
    code: int

    def __init__(self, num_relations: int, dim: int):
        super().__init__()
        if isinstance(num_relations, bool) or not isinstance(num_relations, int) or not 1 <= num_relations <= 65536:
            raise ValueError(f"num_relations must be an int in 1..65536 (got {num_relations!r})")
        if isinstance(dim, bool) or not isinstance(dim, int) or not 1 <= dim <= MAX_WIDTH:
            raise ValueError(f"dim must be an int in 1..{MAX_WIDTH} (got {dim!r}); DESIGN.md 22")
        self.num_relations, self.dim = num_relations, dim
        self.rel = nn.Parameter(torch.empty(num_relations, dim))
        nn.init.xavier_uniform_(self.rel)
        self._bad: Optional[Tensor] = None
        self.index_builds = {"node": 0, "relation": 0}      # halves of the index built so far (tests, profiling)

    _bad_word = DistMult._bad_word

    def forward(self, z: Tensor, s: Tensor, r: Tensor, o: Tensor) -> Tensor:
        if not torch.is_tensor(z) or z.dim() != 2 or z.shape[1] != self.dim or z.dtype != torch.float32:
            raise ValueError(f"z must be float32 [N, {self.dim}] (got {tuple(z.shape) if torch.is_tensor(z) else type(z)})")
        if z.device != self.rel.device:
            raise ValueError(f"z lives on {z.device}, the decoder on {self.rel.device}")
        s, r, o = _triples(s, r, o, z.device)
        return _KgeFunction.apply(z, self.rel, s, r, o, self._bad_word(z.device), self.index_builds, self.code)

    def check(self) -> None:
        """Raise if a call since the last ``check()`` met an id out of range.  Reads one word back: SYNCHRONISES."""
        try:
            DistMult.check(self)
        except ValueError as err:
            raise ValueError(str(err).replace("DistMult", type(self).__name__)) from None


class ComplEx(_KgeDecoder):
    """``score(s, r, o) = Re sum_k s_k r_k conj(o_k)`` on ``dim / 2`` complex components: columns ``2k, 2k + 1`` of a row of ``z`` /
    ``rel`` are the real and imaginary part of component k, the layout ``torch.view_as_complex(z.view(N, dim // 2, 2))`` reads.
    Not symmetric in subject and object.  ``dim`` must be even."""
    code = _lib.KGE_COMPLEX

    def __init__(self, num_relations: int, dim: int):
        super().__init__(num_relations, dim)
        if dim % 2:
            raise ValueError(f"ComplEx needs an even dim: two columns per complex component (got {dim})")


class TransE(_KgeDecoder):
    """``score(s, r, o) = -sum_k |z[s, k] + rel[r, k] - z[o, k]|``: the L1 norm, PyG's default ``p_norm``.  The gradient uses
    ``sign(0) = 0``, torch's convention.  Scores are never positive: train it with ``loss="margin"``."""
    code = _lib.KGE_TRANSE_L1


class _SoftmaxLossFunction(torch.autograd.Function):
    """rgcn_lpsm_query + rgcn_lpsm_forward forward; rgcn_lpsm_backward, then rgcn_lp_index_build + rgcn_lpsm_query_backward
    backward.  The index is the decoders' own, built in the backward and only the halves the wanted gradients need."""

    @staticmethod
    def forward(ctx, z, rel, s, r, o, bad, builds, code, side, limit=MAX_WIDTH):
        zp, rp = _padded(z.detach(), limit), _padded(rel.detach(), limit)
        anchor, target = (s, o) if side == 0 else (o, s)
        qrows, qtarget = _lib.lpsm_query(code, side, zp, rp, anchor, r, target, bad)
        lse, _, loss = _lib.lpsm_forward(qrows, zp, qtarget)
        ctx.save_for_backward(zp, rp, s, r, o, qrows, qtarget, lse)
        ctx.bad, ctx.builds, ctx.code, ctx.side = bad, builds, code, side
        return loss

    @staticmethod
    def backward(ctx, g):
        zp, rp, s, r, o, qrows, qtarget, lse = ctx.saved_tensors
        need_z, need_rel = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dz = drel = None
        if need_z or need_rel:
            dq, dz = _lib.lpsm_backward(qrows, zp, qtarget, lse, g.contiguous(), need_z)
            ix = _lib.lp_index_build(s, r, o, int(zp.shape[0]), int(rp.shape[0]), ctx.bad, nodes=need_z, relations=need_rel)
            ctx.builds["node"] += int(need_z)
            ctx.builds["relation"] += int(need_rel)
            drel = _lib.lpsm_query_backward(ctx.code, ctx.side, zp, rp, s, r, o, dq, ix, dz, need_rel)
        return dz, drel, None, None, None, None, None, None, None, None


def softmax_loss(z: Tensor, decoder: nn.Module, s: Tensor, r: Tensor, o: Tensor, side: str = "object", wide: bool = False) -> Tensor:
    """The 1-N ("1vsAll") loss, float32 [Q]: ``loss_i = logsumexp_n <q_i, z_n> - <q_i, z_target_i>`` over ALL N entities, unfiltered
    and with the true one included; ``q_i`` is the decoder's query row of (s_i, r_i, ?) (``side="object"``, the target is o_i) or
    (?, r_i, o_i) (``"subject"``, the target is s_i), the row ``ranks`` scores with.  No [Q, N] logits exist, forward or backward
    (csrc/rgcn_lp_softmax.hip).  Differentiable in ``z`` and ``decoder.rel`` under any upstream [Q] gradient.
    ``DistMult`` of at most 128 columns and ``ComplEx``; ``TransE`` scores are no dot product with a query row.  ``wide=True`` also
    serves a ``DistMult(..., wide=True)`` of 129..512 columns, on csrc/rgcn_lp_softmax_wide.hip; every other decoder
    runs with the flag bit for bit as without it.  A triple with an id out of range gets loss 0 and no gradient and is reported by
    ``check()``."""
    if side not in ("object", "subject"):
        raise ValueError(f"side must be 'object' or 'subject' (got {side!r})")
    if not isinstance(wide, bool):
        raise ValueError(f"wide must be a bool (got {wide!r})")
    limit = MAX_WIDTH
    if isinstance(decoder, DistMult):
        if decoder.family != "lp":
            if not wide:
                raise ValueError(f"softmax_loss serves DistMult up to {MAX_WIDTH} columns (got {decoder.dim}) unless wide=True is passed "
                                 f"(up to {WIDE_MAX_WIDTH}); DESIGN.md 23, 24")
            limit = WIDE_MAX_WIDTH
        code = _lib.LPSM_DISTMULT
    elif isinstance(decoder, ComplEx):
        code = decoder.code
    else:
        raise ValueError("softmax_loss needs a DistMult or ComplEx decoder: the score must be a dot product with a query row")
    if not torch.is_tensor(z) or z.dim() != 2 or z.shape[1] != decoder.dim or z.dtype != torch.float32:
        raise ValueError(f"z must be float32 [N, {decoder.dim}] (got {tuple(z.shape) if torch.is_tensor(z) else type(z)})")
    if z.device != decoder.rel.device:
        raise ValueError(f"z lives on {z.device}, the decoder on {decoder.rel.device}")
    if z.device.type != "cuda":
        raise ValueError(f"softmax_loss runs on the GPU only: z lives on {z.device} and there is no torch fallback")
    s, r, o = _triples(s, r, o, z.device)
    return _SoftmaxLossFunction.apply(z, decoder.rel, s, r, o, decoder._bad_word(z.device), decoder.index_builds, code,
                                      0 if side == "object" else 1, limit)


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


def ranks(z: Tensor, decoder: nn.Module, s: Tensor, r: Tensor, o: Tensor, side: str = "object",
          filter: Optional[FilterIndex] = None) -> Tuple[Tensor, Tensor]:
    """``(greater, equal)`` int64 [Q]: for every test triple the candidates that score strictly above, and exactly like, its true
    object (``side="object"``: (s, r, ?)) or subject (``"subject"``: (?, r, o); DistMult is symmetric, the same kernel with the
    object as anchor), over all N entities but the true one and, with ``filter``, but every entity that completes the query to a
    known triple.  No [Q, N] scores exist anywhere.  A query with an id out of range gets (-1, -1).  ``ComplEx`` and ``TransE``
    decoders are ranked by rgcn_kge_rank, which is told the side."""
    if side not in ("object", "subject"):
        raise ValueError(f"side must be 'object' or 'subject' (got {side!r})")
    if not isinstance(decoder, (DistMult, _KgeDecoder)):
        raise ValueError("ranks scores with a DistMult, ComplEx or TransE decoder")
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
    if isinstance(decoder, _KgeDecoder):       # not symmetric: the kernel is told which end the anchor is
        return _lib.kge_rank(decoder.code, 0 if side == "object" else 1, _padded(z.detach()), _padded(decoder.rel.detach()), anchor, r,
                             target, fptr, fidx)
    limit = WIDE_MAX_WIDTH if decoder.family == "lpw" else MAX_WIDTH
    return _lib.lp_rank(_padded(z.detach(), limit), _padded(decoder.rel.detach(), limit), anchor, r, target, fptr, fidx,
                        family=decoder.family)


def topk(z: Tensor, decoder: nn.Module, anchor: Tensor, r: Tensor, k: int, side: str = "object",
         filter: Optional[FilterIndex] = None) -> Tuple[Tensor, Tensor]:
    """``(ids int64 [Q, k], scores float32 [Q, k])``: the ``k`` (1..64) best objects of (anchor, r, ?) (``side="object"``) or subjects
    of (?, r, anchor) (``"subject"``) among all N entities but, with ``filter``, those that complete the query to a known triple.  The
    scores are ``ranks``'s, bit for bit; the order is score descending, equal scores by ascending id; a NaN score is never selected.
    A query with fewer than ``k`` candidates ends in slots of id -1 and score -inf, a query with an id out of range is a whole row of
    them.  No [Q, N] scores exist anywhere; a query's row does not depend on the other queries of the call.  ``DistMult`` of at most
    128 columns and ``ComplEx`` (csrc/rgcn_lp_topk.hip)."""
    if side not in ("object", "subject"):
        raise ValueError(f"side must be 'object' or 'subject' (got {side!r})")
    if isinstance(decoder, TransE):
        raise ValueError("topk does not serve TransE: its candidates are swept on the vector ALU, not by the selection kernel (DESIGN.md 25)")
    if not isinstance(decoder, (DistMult, ComplEx)):
        raise ValueError("topk scores with a DistMult or ComplEx decoder")
    if isinstance(decoder, DistMult) and decoder.family != "lp":
        raise ValueError(f"topk serves DistMult rows of at most {MAX_WIDTH} columns (got {decoder.dim}; DESIGN.md 25)")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= 64:
        raise ValueError(f"k must be an int in 1..64 (got {k!r})")
    if filter is not None and not isinstance(filter, FilterIndex):
        raise ValueError("filter must be a FilterIndex or None")
    if not torch.is_tensor(z) or z.dim() != 2 or z.shape[1] != decoder.dim or z.dtype != torch.float32:
        raise ValueError(f"z must be float32 [N, {decoder.dim}]")
    anchor, r = _ids("anchor", anchor, z.device), _ids("r", r, z.device)
    if anchor.shape != r.shape:
        raise ValueError(f"anchor and r must have one length (got {tuple(anchor.shape)}, {tuple(r.shape)})")
    fptr = fidx = None
    if filter is not None:
        if filter.num_nodes != z.shape[0] or filter.num_relations != decoder.num_relations:
            raise ValueError("the filter was built for another number of nodes or relations")
        fptr, fidx = filter.lists(anchor, r, anchor, side)      # (lists keys on the anchor's end only)
    zp, rp = _padded(z.detach()), _padded(decoder.rel.detach())
    if isinstance(decoder, ComplEx):
        return _lib.kge_topk(decoder.code, 0 if side == "object" else 1, zp, rp, anchor, r, k, fptr, fidx)
    return _lib.lp_topk(zp, rp, anchor, r, k, fptr, fidx)


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
