"""``RGCNConv``: constructor-, attribute- and forward-compatible with PyG 2.3.1
``torch_geometric.nn.RGCNConv`` as the reference uses it (/root/reference/model/layers.py:15-16,
21-23, 33-46), with forward and backward running as the HIP kernels of
``csrc/rgcn_tile_fp32*.hip`` / ``rgcn_tile3p.hip`` / ``rgcn_ep.hip`` / ``rgcn_dw_*.hip`` through the C ABI of ``include/rgcn_mi355x.h``
(layers with a side above 128, opt-in ``wide=True``: ``csrc/rgcn_xwide.hip``).

Mutability contract (model/layers.py:33-46, model/modelTrainer.py:26-39): ``weight`` / ``root`` /
``bias`` are plain ``nn.Parameter`` attributes that callers REPLACE after construction and may
freeze; forward reads them at call time and backward skips the frozen ones.

There is no CPU path: CPU tensors (or a missing HIP library) raise.
"""
from __future__ import annotations

import math
import os
from collections import namedtuple
from typing import Optional, Tuple

import torch
from torch import Tensor, nn

from . import _lib
from .plan import GraphPlans, TilePlan, build_graph_plans, cached_graph_plans, choose_layout, padded_width


def _round4(n: int) -> int:
    return (n + 3) // 4 * 4


def _rows16(t: Tensor, width: int) -> Tensor:
    """float32, contiguous rows whose stride is a multiple of 4 elements, zero padded (C ABI rule)."""
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    if width % 4 != 0:
        return torch.nn.functional.pad(t, (0, _round4(width) - width))
    return t.contiguous()


# forward / dX on the bf16 x 3 kernel whose PRODUCER waves split the gathered rows (csrc/rgcn_tile3p.hip):
# fp32-equivalent arithmetic; layers padded to 64 x 64 on graphs dense enough for 128-slot chunks.  "1": on, anything else: off
_SPLIT_PRODUCERS_DEFAULT = os.environ.get("RGCN_SPLIT_PRODUCERS", "1")
_MERGE_RUNS_DEFAULT = os.environ.get("RGCN_MERGE_RUNS", "1") == "1"
_PATH_DEFAULT = os.environ.get("RGCN_PATH", "auto")       # auto | ring | ep
# layers with up to 512 features per side on the kernels of csrc/rgcn_xwide.hip: RGCNConv(..., wide=None) takes this default
_WIDE_DEFAULT = os.environ.get("RGCN_WIDE", "0") == "1"
NARROW_MAX_WIDTH = 128          # RGCN_MAX_WIDTH: the widest side the other kernels take
SPLIT_PRODUCERS_TILE = 224       # the largest tile whose fp32 accumulator fits beside the kernel's two 48 KiB ring slots
# exact-fp32 forward / dX of 64 x 64 layers on layout-3 plans (round 4): the largest tile it takes.  Measured at the headline
# config, forward / dX launch, A/B on one box (profiles/r04g_exact_merge_timing.txt): layout 0 at the cost model's 352: 10.42 /
# 10.33 ms; layout 3 at 352 (40 % of the chunks compacted, 5.8 % fewer head row tiles) 10.12 / 10.18; at 320: 10.21 / 10.19; at
# 288 (60 %, -10 %): 10.32 / 10.41 -- smaller tiles compact more chunks but pay more of them: the cap stays at 352
EXACT_MERGE_TILE = int(os.environ.get("RGCN_EXACT_MERGE_TILE", 352))
DW_TILES_MIN_EDGES = 4_000_000

_ACT_CODES = {None: _lib.ACT_NONE, "relu": _lib.ACT_RELU, "sigmoid": _lib.ACT_SIGMOID}
# graphs from this many nodes run the root / bias gradient kernel on a side stream beside the dX launch (below it the step is
# launch-bound and a second stream only adds event traffic)
_SIDE_STREAM_MIN_ROWS = int(os.environ.get("RGCN_SIDE_STREAM_MIN_ROWS", 262144))
_side_streams = {}


def _side_stream(device) -> "torch.cuda.Stream":
    key = torch.device(device).index
    st = _side_streams.get(key)
    if st is None:
        st = _side_streams[key] = torch.cuda.Stream(device=device)
    return st


def layout_for(in_channels: int, out_channels: int, n_nodes: int = 0, n_edges: int = 0,
               num_relations: int = 1) -> Tuple[int, int]:
    """(output nodes per tile, edge slots per chunk) for a layer (plan.choose_layout): bounded by the LDS budget of
    the wider side, tuned to the graph's density."""
    if not (1 <= in_channels <= 128 and 1 <= out_channels <= 128):
        raise ValueError(f"RGCNConv widths must be in 1..128, got {in_channels}->{out_channels}")
    return choose_layout(n_nodes, n_edges, num_relations, in_channels, out_channels)


def tile_for(in_channels: int, out_channels: int, n_nodes: int = 0, n_edges: int = 0, num_relations: int = 1) -> int:
    """Output nodes per tile of ``layout_for``."""
    return layout_for(in_channels, out_channels, n_nodes, n_edges, num_relations)[0]


class DistContext:
    """One process per GPU.  Output nodes are cut into ``pieces * world`` tile-aligned blocks, dealt piece-major: block
    (s, r) = rows [bounds[s * world + r], bounds[s * world + r + 1]) belongs to rank r.  A rank computes piece s straight into
    its block of the gathered buffer and the blocks of super-block s travel asynchronously while it computes piece s + 1
    (dist.py).  Two cuts:
      * uniform (``piece_rows`` rows per block, the last blocks padded past the graph's end): one in-place
        ``all_gather_into_tensor`` per piece -- the default wherever equal node blocks hold equal edge counts within 5 %;
      * balanced (``dist.balanced_bounds``: blocks of about equal EDGE count): unequal blocks, gathered by one
        broadcast per rank and piece (what an uneven all-gather is underneath).
    Two exchanges (round 4):
      * ``exchange = "full"`` (default): every rank ends up with every row of the gathered matrix -- the per-layer all-reduce
        of north_star with one contributor per row;
      * ``exchange = "needed"`` (opt-in, dist.attach(..., exchange="needed")): a rank receives only the rows its own plans
        gather (dist.NeededRows, derived from the edge list at plan time: the sources of the edges into its blocks for a
        forward output, the destinations of the edges out of them for a dX output) -- one ``all_to_all_single`` with split sizes
        per piece instead of the all-gather, packed rows scattered into place.  Owned rows and read rows are bit-identical to
        the full exchange; rows no plan of this rank reads are NOT written (they hold whatever the allocator returned), so
        the mode is for layers whose output feeds another partitioned layer over the same graph, not for a model's last layer.
    ``emulate``: no process group at all -- ONE process stands in for rank ``rank`` of a ``world``-rank job: it builds that
    rank's plans, launches that rank's kernels, packs / unpacks that rank's rows, and skips the collectives (bench.py
    --emulate-world: what a rank's share of a step costs, measured on one GPU).
    ``stats`` counts what the collectives moved (bench.py reports it per step)."""

    def __init__(self, group, rank: int, world: int, piece_rows: int, pieces: int, bounds=None, exchange: str = "full",
                 emulate: bool = False, split_hubs: bool = True, uniform: Optional[bool] = None):
        if exchange not in ("full", "needed"):
            raise ValueError("exchange must be 'full' or 'needed'")
        self.group, self.rank, self.world = group, rank, world
        self.pieces = pieces
        self.exchange, self.emulate = exchange, emulate
        # edge-parallel pieces: the heavy (node, relation) segments of the whole graph are summed by ALL ranks, an equal share of
        # their rows each, and one small all-reduce completes the sums (eplan.SharedHeavy) -- a hub no longer belongs to one rank
        self.split_hubs = split_hubs
        # uniform: the blocks of ONE piece are equal (one in-place all-gather per piece); ``bounds`` given with uniform = True:
        # pieces of different lengths (dist.piece_tiles: whole launch rounds), still equal blocks inside each
        self.uniform = (bounds is None) if uniform is None else bool(uniform)
        self.bounds_equal = bounds is None                 # every block of every piece has ``piece_rows`` rows
        self.piece_rows = piece_rows if bounds is None else None
        self.bounds = [i * piece_rows for i in range(pieces * world + 1)] if bounds is None else [int(b) for b in bounds]
        assert len(self.bounds) == pieces * world + 1
        if self.uniform:
            for s_ in range(pieces):
                sizes = {self.bounds[s_ * world + r + 1] - self.bounds[s_ * world + r] for r in range(world)}
                assert len(sizes) == 1, "uniform cut: the blocks of a piece are equal"
        self.stats = {"all_gather": 0, "all_gather_bytes": 0, "all_reduce": 0, "all_reduce_bytes": 0,
                      "wait_events": []}
        self.time_waits = False     # bench.py: HIP events around the waits on the collectives, piece by piece
        self.poison_unread = False  # tests: a row no exchange wrote is a NaN wherever it is read

    @property
    def total_rows(self) -> int:
        return self.bounds[-1]

    def block(self, s: int, r: Optional[int] = None) -> Tuple[int, int]:
        r = self.rank if r is None else r
        return self.bounds[s * self.world + r], self.bounds[s * self.world + r + 1]

    def node_range(self, s: int, n_nodes: int, r: Optional[int] = None) -> Tuple[int, int]:
        """owned node range of block (s, r), clipped to the graph; a block that lies wholly past the last node is
        the empty range at the tile-aligned end (n_nodes rounded up would not be a valid begin otherwise)"""
        b, e = self.block(s, r)
        if b >= n_nodes:
            return b, b
        return b, min(e, n_nodes)

    def src_rank(self, r: int) -> int:
        """global rank of group rank r (broadcast sources are global ranks)"""
        if self.group is None:
            return r
        return torch.distributed.get_global_rank(self.group, r)


def _gather_pieces(dctx: "DistContext", plans_list, launch, ld: int, n: int, device,
                   dtype: torch.dtype = torch.float32, needed=None, defer: bool = False):
    """Run ``launch(plan, out_rows)`` for every piece this rank owns and exchange the pieces, overlapping the collective of
    piece s (RCCL's own stream) with the kernels of piece s + 1 (current stream).
    Full exchange, uniform cut: an IN-PLACE all-gather (this rank's block is already where the collective would put it:
    sendbuf == recvbuf + rank * count, the aliasing NCCL / RCCL document for in-place all-gather).  Balanced cut: every rank
    broadcasts its block of the piece in place.  ``needed`` (dist.NeededRows of this direction, exchange = "needed"): the rows
    the peers read of this rank's block are packed (index_select, peer by peer), travel in one all_to_all_single with split
    sizes, and the rows this rank reads of the peers' blocks are scattered into place (index_copy_) one piece behind the
    launches.  Returns the gathered matrix, or with ``defer`` (the backward: the weight-gradient kernels need none of the
    gathered rows and run under the dX exchange) a pair (matrix, finish) -- ``finish()`` makes the current stream wait for what
    is still in flight."""
    full = torch.empty(max(dctx.total_rows, n), ld, dtype=dtype, device=device)
    if dctx.poison_unread:
        full.fill_(float("nan"))
    handles = []
    w = dctx.world
    esz = full.element_size()
    live = not dctx.emulate

    def unpack(s_idx, hs, recv):
        for h in hs:
            h.wait()
        if recv is not None and recv.shape[0] > 0:
            full.index_copy_(0, needed.recv_idx[s_idx], recv)

    for s_idx, plan in enumerate(plans_list):
        b, e = dctx.block(s_idx)
        mine = full[b:e]
        if plan.n_owned > 0:
            launch(plan, mine)
        if plan.n_owned < e - b:
            mine[plan.n_owned:].zero_()     # rows past the graph's end: defined bytes on the wire
        hs, recv = [], None
        if needed is not None:
            send = full.index_select(0, needed.send_idx[s_idx])
            recv = torch.empty(int(needed.recv_idx[s_idx].shape[0]), ld, dtype=dtype, device=device)
            if live:
                hs.append(torch.distributed.all_to_all_single(recv, send, needed.recv_splits[s_idx], needed.send_splits[s_idx],
                                                              group=dctx.group, async_op=True))
            dctx.stats["all_gather_bytes"] += recv.shape[0] * ld * esz
        elif dctx.uniform:
            sup = full[dctx.bounds[s_idx * w]:dctx.bounds[(s_idx + 1) * w]]
            if live:
                hs.append(torch.distributed.all_gather_into_tensor(sup, mine, group=dctx.group, async_op=True))
            dctx.stats["all_gather_bytes"] += (w - 1) * (e - b) * ld * esz      # bytes this rank RECEIVES
        else:
            for r in range(w):
                rb, re = dctx.block(s_idx, r)
                if re > rb:
                    if live:
                        hs.append(torch.distributed.broadcast(full[rb:re], src=dctx.src_rank(r), group=dctx.group, async_op=True))
                    if r != dctx.rank:
                        dctx.stats["all_gather_bytes"] += (re - rb) * ld * esz
        handles.append((s_idx, hs, recv))
        dctx.stats["all_gather"] += 1
        if needed is not None and len(handles) >= 2 and handles[-2] is not None:
            # the packed rows of the piece before: their collective had this piece's kernels to finish under
            unpack(*handles[-2])
            handles[-2] = None

    def finish():
        timed = dctx.time_waits and device.type == "cuda"
        evs = []
        for item in handles:          # piece by piece: which piece's exchange the launch stream had to wait for
            if timed:
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record()
            if item is not None:
                unpack(*item)
            if timed:
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record()
                evs.append((e0, e1))
        if timed:
            dctx.stats["wait_events"].append(evs)
        handles.clear()

    if defer:
        return full[:n], finish
    finish()
    return full[:n]


def _xwide_operand(wf: Tensor, cp: Optional[Tensor], rt: Optional[Tensor], num_rel: int, din: int, dout: int,
                   transpose: bool) -> Tensor:
    """The weight operand of rgcn_xwide_*: row-major [R' + 1, K, N], relation blocks then the root (zeros without one); blocks W_r
    (forward) or W_r^T (dX).  A basis or block-diagonal decomposition is composed into it by torch ops."""
    if cp is not None:
        w = (cp @ wf.view(wf.shape[0], -1)).view(num_rel, din, dout)
    elif wf.dim() == 4:
        eye = torch.eye(wf.shape[1], device=wf.device, dtype=wf.dtype)
        w = torch.einsum("rbio,bc->rbico", wf, eye).reshape(num_rel, din, dout)
    else:
        w = wf
    r = rt if rt is not None else torch.zeros(din, dout, dtype=torch.float32, device=wf.device)
    op = torch.cat([w, r.unsqueeze(0)], 0)
    return op.transpose(1, 2).contiguous() if transpose else op


def _xwide_decomposed_grads(dw: Tensor, wf: Tensor, cp: Optional[Tensor], need_weight: bool, need_comp: bool):
    """(d_weight, d_comp) of a decomposition from the dense d_W [R', in, out] scratch of rgcn_xwide_bwd_dw, by torch ops:
    basis d_bases = comp^T d_W, d_comp[r, b] = <d_W[r], bases[b]>; blocks: the diagonal blocks of d_W."""
    r = dw.shape[0]
    if cp is not None:
        flat = dw.view(r, -1)
        dv = (cp.t() @ flat).view_as(wf) if need_weight else None
        dc = flat @ wf.view(wf.shape[0], -1).t() if need_comp else None
        return dv, dc
    nb, bi, bo = wf.shape[1], wf.shape[2], wf.shape[3]
    return dw.view(r, nb, bi, nb, bo).diagonal(dim1=1, dim2=3).permute(0, 3, 1, 2).contiguous(), None


def _shared_heavy_sums(shared, x: Tensor, width: int, dctx: "DistContext") -> Optional[Tensor]:
    """H[segment] = sum of the weighted rows of every heavy (node, relation) segment of the WHOLE graph: this rank's share of the
    rows (rgcn_ep_segment_sum), then one all-reduce over the ranks (eplan.SharedHeavy)"""
    if shared is None:
        return None
    hmat = _lib.ep_aggregate_shared(shared, x, width)
    if not dctx.emulate:
        torch.distributed.all_reduce(hmat, group=dctx.group)
    dctx.stats["all_reduce"] += 1
    dctx.stats["all_reduce_bytes"] += hmat.numel() * 4
    dctx.stats["shared_heavy_rows"] = dctx.stats.get("shared_heavy_rows", 0) + (shared.row_hi - shared.row_lo)
    return hmat


def _operands(*params):
    """the layer's parameters as the kernels read them: detached, float32, contiguous (None stays None)"""
    return [None if p is None else p.detach().float().contiguous() for p in params]


def _padded_rows(n: int, width: int, device) -> Tensor:
    """an uninitialised float32 [n, width rounded up to 4] row buffer: what a kernel stores an output into (C ABI rule)"""
    return torch.empty(n, _round4(width), dtype=torch.float32, device=device)


def _trim(rows: Tensor, width: int) -> Tensor:
    """a padded row buffer without its padding columns"""
    return rows if rows.shape[1] == width else rows[:, :width]


def _keep_activated(ctx, act: int, grad_premasked: bool, out: Tensor) -> Optional[Tensor]:
    """Records on ``ctx`` whether the backward needs the activated output and returns what to save for it.  The activated output
    is only needed to differentiate the activation; a ReLU whose consumer folds the mask into its dX store (grad_premasked)
    needs nothing."""
    ctx.act, ctx.need_a = act, act == _lib.ACT_SIGMOID or (act == _lib.ACT_RELU and not grad_premasked)
    return out if ctx.need_a else None


def _grad_z(ctx, g: Tensor, dout: int, a_out: Optional[Tensor]) -> Tensor:
    """dL/dz = dL/da * act'(a) in padded rows, from the gradient ``g`` of the activated output (_keep_activated)"""
    gp = _rows16(g, dout)
    return _lib.act_backward(a_out, gp, ctx.act) if ctx.need_a else gp


def _own_param_grads(dw: Optional[Tensor], wf: Tensor, cp: Optional[Tensor], need_weight: bool, need_comp: bool, xwide: bool = False):
    """(d_weight, d_comp) of the layer's own parameters from the dense d_W [R, in, out] the weight-gradient kernels wrote: d_W
    itself for a dense layer, else the decomposition's gradients (rgcn_basis_backward / rgcn_block_backward; ``xwide``: torch ops)"""
    if dw is None or (cp is None and wf.dim() != 4):
        return dw, None
    return (_xwide_decomposed_grads if xwide else _lib.decomposed_weight_grads)(dw, wf, cp, need_weight, need_comp)


def _launch_fwd(pl, xp: Tensor, din: int, packed: Tensor, bs: Optional[Tensor], rows: Tensor, dout: int, act: int, flags: int,
                hmat: Optional[Tensor] = None) -> Optional[Tensor]:
    """forward of one plan into ``rows``: rgcn_fwd, or the edge-parallel path for an eplan.EdgePlan (returns its H)"""
    if not isinstance(pl, TilePlan):
        return _lib.ep_layer(pl, xp, din, packed, bs, rows, dout, act, None, flags, hmat=hmat)
    _lib.fwd(_lib.plan_struct(pl), xp, din, packed, bs, rows, dout, act, flags)


def _launch_dx(pl, gp: Tensor, dout: int, packed_t: Tensor, rows: Tensor, din: int, mask: Optional[Tensor], flags: int,
               hmat: Optional[Tensor] = None):
    """dX of one transposed plan into ``rows``: rgcn_bwd_dx, or the edge-parallel path for an eplan.EdgePlan"""
    if not isinstance(pl, TilePlan):
        return _lib.ep_layer(pl, gp, dout, packed_t, None, rows, din, _lib.ACT_NONE, mask, flags, hmat=hmat)
    _lib.bwd_dx(_lib.plan_struct(pl), gp, dout, packed_t, rows, din, mask, flags)


def _flat_grads(need_w: bool, need_root: bool, need_bias: bool, num_rel: int, din: int, dout: int, device):
    """ONE flat buffer for the three weight gradients (a single all-reduce in the distributed case): (new, views) -- ``new()``
    allocates one, ``views(flat)`` are its (d_weight, d_root, d_bias) parts, None for a gradient nobody needs"""
    o0 = num_rel * din * dout if need_w else 0
    o1 = o0 + (din * dout if need_root else 0)
    numel = o1 + (dout if need_bias else 0)

    def new(zeros: bool = False) -> Tensor:
        return (torch.zeros if zeros else torch.empty)(numel, dtype=torch.float32, device=device)

    def views(flat: Tensor):
        return (flat[:o0].view(num_rel, din, dout) if need_w else None,
                flat[o0:o1].view(din, dout) if need_root else None,
                flat[o1:].view(dout) if need_bias else None)

    return new, views


def _dw_tiles(dwp: TilePlan, walk: Tensor, xp: Tensor, din: int, gp: Tensor, dout: int, parts, flags: int) -> None:
    """d_weight by the tile-major kernel on ``dwp`` and d_root / d_bias by the plan-free streaming kernel, over the rows [b, e)
    ``dwp`` owns, into ``parts`` = (d_weight, d_root, d_bias) views of the flat buffer: a kernel whose views are None is skipped"""
    pw, pr, pb = parts
    b, e = dwp.node_begin, dwp.node_end
    if pw is not None:
        _lib.bwd_dw_tiles(_lib.plan_struct(dwp), walk, xp, din, gp[b:e], dout, pw, flags)
    if pr is not None or pb is not None:
        _lib.bwd_dw_root(xp[b:e], din, gp[b:e], dout, pr, pb)


def _dw_walk(pc: GraphPlans, xp: Tensor, din: int, gp: Tensor, dout: int, parts, flags: int, hmat: Optional[Tensor]) -> None:
    """one piece's weight gradients by the relation-major kernels on its forward plan's units (GraphPlans.fwd_walk), plus an
    edge-parallel forward's heavy segments: d_W_r += H_seg^T g[dst] over their pseudo rows (``hmat``: H of the forward)"""
    fp = pc.fwd_walk
    pw, pr, pb = parts
    gr = gp[fp.node_begin:fp.node_end]
    _lib.bwd_dw(_lib.plan_struct(fp), xp, din, gr, dout, pw, pr, pb, flags)
    epf = pc.ep_fwd
    if pw is not None and epf is not None and epf.heavy is not None:
        if hmat is None:
            hmat = _lib.ep_aggregate_heavy(epf, xp, din)
        pw2 = torch.empty_like(pw)
        _lib.bwd_dw(_lib.plan_struct(epf.heavy_tile_plan()), hmat, din, gr, dout, pw2, None, None, flags)
        pw.add_(pw2)


def _dw_on_tiles(pc: GraphPlans, tiles_ok: bool, need_w: bool, gp: Tensor) -> bool:
    """Which kernel takes the weight gradients of a piece (one GPU: the graph).  One with a tile-major d_weight plan takes that
    plan (layout-3 forward plans always: the relation-major kernels refuse them) unless the flags pin other kernels
    (``tiles_ok``: _RGCNLayerFn.backward); the tile-major kernel gathers x and g through buffer descriptors only."""
    return (tiles_ok and pc.dw is not None and (need_w or pc.fwd.layout == 3)
            and _lib.buffer_addressable(pc.fwd.n_owned, gp.shape[1]))


def _dw_one_gpu_root(plans: GraphPlans, parts, overlap: bool, xp: Tensor, din: int, gp: Tensor, dout: int, flags: int):
    """One GPU on the tile-major plan, the part enqueued BEFORE the dX launch: d_root / d_bias by the streaming kernel, on a side
    stream where ``overlap`` (a dX launch follows on a graph of at least _SIDE_STREAM_MIN_ROWS nodes).  Returns that stream, or
    None; _dw_one_gpu_tiles joins it."""
    _, pr, pb = parts
    side = None
    if overlap and (pr is not None or pb is not None):
        # d_root / d_bias on a SIDE stream, enqueued before the dX launch: the streaming kernel is HBM-bound with a tenth
        # of a launch's MFMAs, uses no LDS and few registers, so its workgroups share the CUs with the MFMA-bound dX
        # kernel instead of adding their ~1 ms behind it.  The join is a stream wait, never a host sync.
        side = _side_stream(gp.device)
        side.wait_stream(torch.cuda.current_stream(gp.device))      # gp (and xp) are produced on the current stream
    with torch.cuda.stream(side):
        _dw_tiles(plans.dw, plans.dw_walk, xp, din, gp, dout, (None, pr, pb), flags)
    return side


def _dw_one_gpu_tiles(plans: GraphPlans, parts, side, xp: Tensor, din: int, gp: Tensor, dout: int, flags: int) -> None:
    """One GPU on the tile-major plan, the part enqueued AFTER the dX launch: d_weight, then the join with ``side``"""
    _dw_tiles(plans.dw, plans.dw_walk, xp, din, gp, dout, (parts[0], None, None), flags)
    if side is not None:
        torch.cuda.current_stream(gp.device).wait_stream(side)


def _dw_rank_range(dw_rank, new, views, stats: dict, xp: Tensor, din: int, gp: Tensor, dout: int, flags: int) -> Optional[Tensor]:
    """Full exchange: x and g are replicated, so this rank's share of the weight gradients is ONE contiguous node range of its own
    (dist.dw_range) -- one tile-major launch + the streaming root part, whatever the pieces.  Returns the flat buffer (zeros for
    an empty range), or None where the kernel cannot address the range's rows of g: the pieces take the gradients then."""
    dwp, walk = dw_rank
    if dwp is None:
        return new(zeros=True)
    if not _lib.buffer_addressable(dwp.n_owned, gp.shape[1]):
        return None
    acc = new()
    _dw_tiles(dwp, walk, xp, din, gp, dout, views(acc), flags)
    stats["dw_tiles_rank"] = stats.get("dw_tiles_rank", 0) + 1
    return acc


def _dw_pieces(pieces, dctx: Optional[DistContext], new, views, on_tiles, hmat: Optional[Tensor], xp: Tensor, din: int, gp: Tensor,
               dout: int, flags: int) -> Tensor:
    """Piece by piece (one GPU off the tile-major plan: the graph is the one piece): each piece's gradients into a flat buffer
    of its own, by the tile-major kernel (a rank's pieces only) or the relation-major ones, and the buffers added up.  Zeros
    without a piece that owns a row."""
    acc = None
    for pc in pieces:
        if pc.fwd_walk.n_owned <= 0:
            continue
        part = new()
        if dctx is not None and on_tiles(pc):
            # a rank's piece on the tile-major kernel, as the single-GPU step (its root part: the piece's own rows)
            _dw_tiles(pc.dw, pc.dw_walk, xp, din, gp, dout, views(part), flags)
            dctx.stats["dw_tiles_pieces"] = dctx.stats.get("dw_tiles_pieces", 0) + 1
        else:
            _dw_walk(pc, xp, din, gp, dout, views(part), flags, hmat)
        acc = part if acc is None else acc.add_(part)
    return new(zeros=True) if acc is None else acc


class _RGCNLayerFn(torch.autograd.Function):
    """a = act(sum_r mean-aggregate_r(x) @ W_r + x @ root + bias)   (forward: rgcn_fwd with the activation fused
    into its store; backward: rgcn_bwd_dx on the transposed plan + the weight-gradient kernels)."""

    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, comp: Optional[Tensor], root: Optional[Tensor], bias: Optional[Tensor],
                plans: GraphPlans, dctx: Optional[DistContext], act: int, input_relu: bool, grad_premasked: bool,
                flags: int, num_rel: int, dout: int):
        # weight / comp: the layer's OWN parameters -- dense [R, in, out], bases [B, in, out] + comp [R, B], or blocks
        # [R, nb, in / nb, out / nb]: a decomposition is composed inside the weight packer and differentiated from the dense
        # d_W scratch of the weight-gradient kernels (rgcn_pack_weights_basis / _block, rgcn_basis_backward / rgcn_block_backward),
        # so autograd never holds an [R, in, out] tensor (PyG materialises it on every call)
        n, din = x.shape
        xp = _rows16(x, din)
        wf, cp, rt, bs = _operands(weight, comp, root, bias)
        packed = _lib.pack_weights_decomposed(wf, cp, rt, num_rel, din, dout, transpose=False)
        if dctx is None:
            out = _padded_rows(n, dout, x.device)
            ctx.ep_heavy = _launch_fwd(plans.fwd or plans.ep_fwd, xp, din, packed, bs, out, dout, act, flags)
        else:
            # every rank computes its own blocks straight into the gathered buffer; with destination-range
            # ownership the per-layer all-reduce of SURVEY.md 8e degenerates to an all-gather (each row has
            # exactly one non-zero contributor), issued piece by piece under the next piece's kernels
            # (a piece whose forward runs the edge-parallel path -- a hub's block -- carries an eplan.EdgePlan instead)
            # (hubs split across ranks, eplan.SharedHeavy: every rank sums its share of the heavy segments' rows, one all-reduce
            # of the [segments, in] sums, then the owners' pseudo rows go through the transform)
            hm_f = ctx.ep_heavy = _shared_heavy_sums(plans.shared_fwd, xp, din, dctx)
            out = _gather_pieces(dctx, [p.fwd or p.ep_fwd for p in plans.pieces],
                                 lambda pl, rows: _launch_fwd(pl, xp, din, packed, bs, rows, dout, act, flags, hm_f),
                                 _round4(dout), n, x.device, needed=plans.needed_fwd if dctx.exchange == "needed" else None)
        ctx.plans, ctx.dctx, ctx.dims = plans, dctx, (n, din, dout, num_rel)
        ctx.input_relu, ctx.flags = input_relu, flags
        ctx.save_for_backward(xp, wf, cp, rt, _keep_activated(ctx, act, grad_premasked, out))
        return _trim(out, dout)

    @staticmethod
    def backward(ctx, g: Tensor):
        xp, wf, cp, rt, a_out = ctx.saved_tensors
        plans, dctx, flags = ctx.plans, ctx.dctx, ctx.flags
        n, din, dout, num_rel = ctx.dims
        need_x, need_wparam, need_comp, need_root, need_bias = ctx.needs_input_grad[:5]      # (False for an input that is None)
        need_w = need_wparam or need_comp              # the dense d_W[R, in, out] (for a decomposition: scratch)
        need_any = need_w or need_root or need_bias
        dev = g.device
        gp = _grad_z(ctx, g, dout, a_out)
        new, views = _flat_grads(need_w, need_root, need_bias, num_rel, din, dout, dev)
        dw_ops = (xp, din, gp, dout, flags)            # what every weight-gradient launch takes
        # the flags leave the tile-major d_weight kernel open to this layer (_dw_on_tiles then asks piece by piece)
        tiles_ok = (not flags & (_lib.FLAG_DW_RING | _lib.FLAG_DW_DIRECT | _lib.FLAG_POINTER_GATHER)
                    and _lib.buffer_addressable(n, xp.shape[1]))
        one_gpu_tiles = dctx is None and need_any and _dw_on_tiles(plans, tiles_ok, need_w, gp)
        dx = acc = finish_dx = None
        # d_root / d_bias of one GPU on the tile-major plan: enqueued before the dX launch
        if one_gpu_tiles:
            acc = new()
            side = _dw_one_gpu_root(plans, views(acc), need_x and n >= _SIDE_STREAM_MIN_ROWS, *dw_ops)
        # dX
        if need_x:
            packed_t = _lib.pack_weights_decomposed(wf, cp, rt, num_rel, din, dout, transpose=True)
            mask = xp if ctx.input_relu else None            # x = relu(z_prev): store dL/dz_prev = dx * (x > 0)
            if dctx is None:
                dxp = _padded_rows(n, din, dev)
                _launch_dx(plans.bwd or plans.ep_bwd, gp, dout, packed_t, dxp, din, mask, flags)
            else:
                hm_b = _shared_heavy_sums(plans.shared_bwd, gp, dout, dctx)
                # the exchange of the dX pieces stays in flight under the weight-gradient kernels below (they read x and the
                # rank's own rows of g, none of the gathered rows); finish_dx() is the wait
                dxp, finish_dx = _gather_pieces(
                    dctx, [p.bwd or p.ep_bwd for p in plans.pieces],
                    lambda pl, rows: _launch_dx(pl, gp, dout, packed_t, rows, din,
                                                None if mask is None else mask[pl.node_begin:pl.node_end], flags, hm_b),
                    _round4(din), n, dev, needed=plans.needed_bwd if dctx.exchange == "needed" else None, defer=True)
            dx = _trim(dxp, din)
        # the weight gradients, and across ranks their all-reduce
        if one_gpu_tiles:
            _dw_one_gpu_tiles(plans, views(acc), side, *dw_ops)
        elif need_any:
            if dctx is not None and plans.dw_rank is not None and tiles_ok:
                acc = _dw_rank_range(plans.dw_rank, new, views, dctx.stats, *dw_ops)
            if acc is None:
                acc = _dw_pieces([plans] if dctx is None else plans.pieces, dctx, new, views,
                                 lambda pc: _dw_on_tiles(pc, tiles_ok, need_w, gp), ctx.ep_heavy, *dw_ops)
            if dctx is not None:
                if not dctx.emulate:
                    torch.distributed.all_reduce(acc, group=dctx.group)
                dctx.stats["all_reduce"] += 1
                dctx.stats["all_reduce_bytes"] += acc.numel() * 4
        dw, droot, dbias = (None, None, None) if acc is None else views(acc)
        if finish_dx is not None:
            finish_dx()
        dw, dcomp = _own_param_grads(dw, wf, cp, need_wparam, need_comp)      # a decomposition's own gradients from the dense d_W
        return dx, dw, dcomp, droot, dbias, None, None, None, None, None, None, None, None


class _MaxLayerFn(torch.autograd.Function):
    """a = act(sum_r max-aggregate_r(x) @ W_r + x @ root + bias) on an eplan.MaxPlan (one GPU): H (and the tie weights T when
    x needs a gradient) by rgcn_segment_max, then the edge-parallel transform and sums with the activation fused (_lib.ep_layer);
    backward: dX by _lib.max_layer_dx (the gradient of a max split evenly among the rows that attain it), d_W over the pseudo
    rows of H, d_root / d_bias by the streaming kernel (above 64 columns: rgcn_bwd_dw over the light units, the root rows)."""

    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, comp: Optional[Tensor], root: Optional[Tensor], bias: Optional[Tensor], mp,
                act: int, input_relu: bool, grad_premasked: bool, flags: int, num_rel: int, dout: int):
        n, din = x.shape
        xp = _rows16(x, din)
        wf, cp, rt, bs = _operands(weight, comp, root, bias)
        packed = _lib.pack_weights_decomposed(wf, cp, rt, num_rel, din, dout, transpose=False)
        hmat, tmat = _lib.max_aggregate(mp, xp, din, with_t=ctx.needs_input_grad[0])
        out = _padded_rows(n, dout, x.device)
        _lib.ep_layer(mp.ep, xp, din, packed, bs, out, dout, act, None, flags, hmat=hmat)
        ctx.mp, ctx.dims, ctx.input_relu, ctx.flags = mp, (n, din, dout, num_rel), input_relu, flags
        ctx.save_for_backward(xp, wf, cp, rt, hmat, tmat, _keep_activated(ctx, act, grad_premasked, out))
        return _trim(out, dout)

    @staticmethod
    def backward(ctx, g: Tensor):
        xp, wf, cp, rt, hmat, tmat, a_out = ctx.saved_tensors
        mp, flags = ctx.mp, ctx.flags
        n, din, dout, num_rel = ctx.dims
        need_x, need_wparam, need_comp, need_root, need_bias = ctx.needs_input_grad[:5]      # (False for an input that is None)
        gp = _grad_z(ctx, g, dout, a_out)
        f32 = dict(dtype=torch.float32, device=g.device)
        dx = dw = droot = dbias = None
        if need_x:
            packed_t = _lib.pack_weights_decomposed(wf, cp, rt, num_rel, din, dout, transpose=True)
            dxp = _padded_rows(n, din, g.device)
            _lib.max_layer_dx(mp, xp, hmat, tmat, gp, dout, packed_t, dxp, din, xp if ctx.input_relu else None, flags)
            dx = _trim(dxp, din)
        if need_wparam or need_comp:
            dw = torch.zeros(num_rel, din, dout, **f32) if mp.ep.heavy is None else torch.empty(num_rel, din, dout, **f32)
            if mp.ep.heavy is not None:
                _lib.bwd_dw(_lib.plan_struct(mp.ep.heavy_tile_plan()), hmat, din, gp, dout, dw, None, None, flags)
        if need_root or need_bias:
            droot = torch.empty(din, dout, **f32) if need_root else None
            dbias = torch.empty(dout, **f32) if need_bias else None
            if max(din, dout) <= 64:
                _lib.bwd_dw_root(xp, din, gp, dout, droot, dbias)
            else:        # (the light units hold the root rows alone: their relation-major walk is the root-only walk)
                _lib.bwd_dw(_lib.plan_struct(mp.ep.as_tile_plan()), xp, din, gp, dout, None, droot, dbias, flags)
        dw, dcomp = _own_param_grads(dw, wf, cp, need_wparam, need_comp)
        return dx, dw, dcomp, droot, dbias, None, None, None, None, None, None, None


class _XwideFn(torch.autograd.Function):
    """A layer with a side above 128 on csrc/rgcn_xwide.hip (one GPU, layout-0 plans): dX on the transposed plan, the weight
    gradients on the forward plan; a decomposition composed into / differentiated from a dense operand by torch ops."""

    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, comp: Optional[Tensor], root: Optional[Tensor], bias: Optional[Tensor],
                plans: GraphPlans, act: int, input_relu: bool, grad_premasked: bool, num_rel: int, dout: int):
        n, din = x.shape
        xp = _rows16(x, din)
        wf, cp, rt, bs = _operands(weight, comp, root, bias)
        out = _padded_rows(n, dout, x.device)
        op = _xwide_operand(wf, cp, rt, num_rel, din, dout, transpose=False)
        _lib.xwide_fwd(_lib.plan_struct(plans.fwd), xp, din, op, bs, out, dout, act)
        del op
        ctx.plans, ctx.dims, ctx.input_relu = plans, (n, din, dout, num_rel), input_relu
        ctx.save_for_backward(xp, wf, cp, rt, _keep_activated(ctx, act, grad_premasked, out))
        return _trim(out, dout)

    @staticmethod
    def backward(ctx, g: Tensor):
        xp, wf, cp, rt, a_out = ctx.saved_tensors
        n, din, dout, num_rel = ctx.dims
        need_x, need_wparam, need_comp, need_root, need_bias = ctx.needs_input_grad[:5]
        gp = _grad_z(ctx, g, dout, a_out)
        dx = dw = droot = dbias = None
        if need_x:
            opt = _xwide_operand(wf, cp, rt, num_rel, din, dout, transpose=True)
            dxp = _padded_rows(n, din, g.device)
            _lib.xwide_bwd_dx(_lib.plan_struct(ctx.plans.bwd), gp, dout, opt, dxp, din, xp if ctx.input_relu else None)
            del opt
            dx = _trim(dxp, din)
        if need_wparam or need_comp or need_root or need_bias:
            f32 = dict(dtype=torch.float32, device=g.device)
            dw = torch.empty(num_rel, din, dout, **f32) if need_wparam or need_comp else None
            droot = torch.empty(din, dout, **f32) if need_root else None
            dbias = torch.empty(dout, **f32) if need_bias else None
            _lib.xwide_bwd_dw(_lib.plan_struct(ctx.plans.fwd), xp, din, gp, dout, dw, droot, dbias)
        dw, dcomp = _own_param_grads(dw, wf, cp, need_wparam, need_comp, xwide=True)
        return dx, dw, dcomp, droot, dbias, None, None, None, None, None, None


class _FeaturelessFn(torch.autograd.Function):
    """Featureless layer (x = None or node indices): out = bias + sum over slots of w * W_rel[x_src] (root = rel R'), forward by
    rgcn_featureless_fwd on the forward plan, every parameter gradient by rgcn_featureless_bwd on the transposed plan.  There
    is no dX: x is an index."""

    @staticmethod
    def forward(ctx, weight: Tensor, comp: Optional[Tensor], root: Optional[Tensor], bias: Optional[Tensor], plans: GraphPlans,
                index, in_rows: int, dout: int):
        wf, cp, rt, bs = _operands(weight, comp, root, bias)
        out = _padded_rows(plans.fwd.n_nodes, dout, wf.device)
        _lib.featureless_fwd(_lib.plan_struct(plans.fwd), None if index is None else index[0], in_rows, wf, cp, rt, bs, out, dout)
        ctx.plans, ctx.index, ctx.in_rows, ctx.dout = plans, index, in_rows, dout
        ctx.save_for_backward(wf, cp)
        return _trim(out, dout)

    @staticmethod
    def backward(ctx, g: Tensor):
        wf, cp = ctx.saved_tensors
        need_w, need_comp, need_root, need_bias = ctx.needs_input_grad[:4]      # (False for an input that is None)
        dout, in_rows, dev = ctx.dout, ctx.in_rows, g.device
        dw = torch.empty_like(wf) if need_w else None
        dcomp = torch.empty_like(cp) if need_comp else None
        droot = torch.empty(in_rows, dout, dtype=torch.float32, device=dev) if need_root else None
        dbias = torch.empty(dout, dtype=torch.float32, device=dev) if need_bias else None
        if need_w or need_comp or need_root or need_bias:
            idx = ctx.index
            _lib.featureless_bwd(_lib.plan_struct(ctx.plans.bwd), None if idx is None else idx[0], None if idx is None else idx[1:3],
                                 in_rows, _rows16(g, dout), dout, wf, cp, dw, dcomp, droot, dbias)
        return dw, dcomp, droot, dbias, None, None, None, None


class _BipartiteFn(torch.autograd.Function):
    """out [N_dst, out] = sum_r aggregate_r(x_src) @ W_r + x_dst @ root + bias (PyG's ``x = (x_src, x_dst)``).  The relations run on
    the plans of a square graph of N = max(N_src, N_dst) nodes that own the rows [0, N_dst) forward and [0, N_src) transposed,
    with the root relation packed as zeros (its pseudo edges add exactly 0); the root term, d_x_dst and d_root -- a matrix of
    another width over rows that pair up one to one -- by csrc/rgcn_rows.hip.  ``plans`` is None without a destination row."""

    @staticmethod
    def forward(ctx, x_src: Tensor, x_dst: Tensor, weight: Tensor, comp: Optional[Tensor], root: Optional[Tensor],
                bias: Optional[Tensor], plans: Optional[GraphPlans], flags: int, num_rel: int, dout: int):
        (n_src, din), (n_dst, din_r) = x_src.shape, x_dst.shape
        n = max(n_src, n_dst)
        wf, cp, rt, bs = _operands(weight, comp, root, bias)
        ctx.plans, ctx.flags, ctx.dims = plans, flags, (n_src, n_dst, din, din_r, dout, num_rel)
        if plans is None:
            ctx.save_for_backward(wf, cp)
            return torch.empty(0, dout, dtype=torch.float32, device=x_src.device)
        if n_src == n:
            xp = _rows16(x_src, din)
        else:       # gathered operands have plan.n_nodes rows: the rows past N_src are the zeros no edge reads
            xp = torch.zeros(n, _round4(din), dtype=torch.float32, device=x_src.device)
            xp[:n_src, :din] = x_src.detach()
        xd = _rows16(x_dst, din_r)
        packed = _lib.pack_weights_decomposed(wf, cp, None, num_rel, din, dout, transpose=False)
        out = _padded_rows(n_dst, dout, x_src.device)
        ctx.ep_heavy = _launch_fwd(plans.fwd or plans.ep_fwd, xp, din, packed, bs, out, dout, _lib.ACT_NONE, flags)
        if rt is not None:
            _lib.rows_transform(xd, din_r, rt, dout, add=out, y=out)
        ctx.save_for_backward(xp, xd, wf, cp, rt)
        return _trim(out, dout)

    @staticmethod
    def backward(ctx, g: Tensor):
        n_src, n_dst, din, din_r, dout, num_rel = ctx.dims
        need_xs, need_xd, need_wparam, need_comp, need_root, need_bias = ctx.needs_input_grad[:6]   # (False for a None input)
        f32 = dict(dtype=torch.float32, device=g.device)
        if ctx.plans is None:       # no destination row: every gradient is a zero
            wf, cp = ctx.saved_tensors
            return (torch.zeros(n_src, din, **f32) if need_xs else None, torch.zeros(0, din_r, **f32) if need_xd else None,
                    torch.zeros_like(wf) if need_wparam else None, torch.zeros_like(cp) if need_comp else None,
                    torch.zeros(din_r, dout, **f32) if need_root else None, torch.zeros(dout, **f32) if need_bias else None,
                    None, None, None, None)
        xp, xd, wf, cp, rt = ctx.saved_tensors
        plans, flags = ctx.plans, ctx.flags
        n = max(n_src, n_dst)
        if n_dst == n:
            gp = _rows16(g, dout)
        else:       # the transposed plan gathers rows of g up to N: the upstream gradient straight into N rows, the tail zeroed
            gp = _padded_rows(n, dout, g.device)
            gp[n_dst:].zero_()
            if gp.shape[1] != dout:
                gp[:n_dst, dout:].zero_()
            gp[:n_dst, :dout] = g
        gd = gp[:n_dst]
        dxs = dxd = dw = droot = dbias = None
        if need_xs:
            packed_t = _lib.pack_weights_decomposed(wf, cp, None, num_rel, din, dout, transpose=True)
            bp = plans.bwd or plans.ep_bwd
            dxp = _padded_rows(bp.node_end - bp.node_begin, din, g.device)
            _launch_dx(bp, gp, dout, packed_t, dxp, din, None, flags)
            dxs = _trim(dxp, din)[:n_src]
        if need_xd and rt is not None:
            dxd = _trim(_lib.rows_transform(gd, dout, rt, din_r, transpose=True), din_r)
        need_w = need_wparam or need_comp
        if need_w or need_bias:
            new, views = _flat_grads(need_w, False, need_bias, num_rel, din, dout, g.device)
            acc = new()
            _dw_walk(plans, xp, din, gp, dout, views(acc), flags, ctx.ep_heavy)
            dw, _, dbias = views(acc)
        if need_root:
            droot = _lib.rows_dw(xd, din_r, gd, dout)
        dw, dcomp = _own_param_grads(dw, wf, cp, need_wparam, need_comp)
        return dxs, dxd, dw, dcomp, droot, dbias, None, None, None, None


class _BlockFn(torch.autograd.Function):
    """out [n_dst, out] = sum_r aggregate_r(x) @ W_r + x[:n_dst] @ root + bias on one sampling.BlockIndex (csrc/rgcn_minibatch.hip):
    the root is relation R of the index, so one transform + one sum per direction and one d_weight launch make the whole layer;
    the aggregated rows H of the forward are kept for d_weight.  No graph plan, no plan cache."""

    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, comp: Optional[Tensor], root: Optional[Tensor], bias: Optional[Tensor], index,
                num_rel: int, dout: int):
        n_src, din = x.shape
        wf, cp, rt, bs = _operands(weight, comp, root, bias)
        ctx.index, ctx.dims = index, (n_src, din, dout, num_rel)
        if index.n_dst == 0:
            ctx.save_for_backward(wf, cp, rt)
            return torch.empty(0, dout, dtype=torch.float32, device=x.device)
        xp = _rows16(x, din)
        packed = _lib.pack_weights_decomposed(wf, cp, rt, num_rel, din, dout, transpose=False)
        out, hmat = _lib.mb_fwd(index._ix, xp, din, packed, bs, dout)
        ctx.save_for_backward(wf, cp, rt, hmat)
        return _trim(out, dout)

    @staticmethod
    def backward(ctx, g: Tensor):
        n_src, din, dout, num_rel = ctx.dims
        need_x, need_wparam, need_comp, need_root, need_bias = ctx.needs_input_grad[:5]      # (False for an input that is None)
        f32 = dict(dtype=torch.float32, device=g.device)
        if ctx.index.n_dst == 0:       # no destination row: every gradient is a zero
            wf, cp, rt = ctx.saved_tensors
            return (torch.zeros(n_src, din, **f32) if need_x else None, torch.zeros_like(wf) if need_wparam else None,
                    torch.zeros_like(cp) if need_comp else None, torch.zeros(din, dout, **f32) if need_root else None,
                    torch.zeros(dout, **f32) if need_bias else None, None, None, None)
        wf, cp, rt, hmat = ctx.saved_tensors
        ix = ctx.index._ix
        gp = _rows16(g, dout)
        dx = dw = droot = dbias = None
        if need_x:
            packed_t = _lib.pack_weights_decomposed(wf, cp, rt, num_rel, din, dout, transpose=True)
            dx = _trim(_lib.mb_bwd_dx(ix, gp, dout, packed_t, din), din)
        need_w = need_wparam or need_comp
        if need_w or need_root:
            dw = torch.empty(num_rel, din, dout, **f32) if need_w else None
            droot = torch.empty(din, dout, **f32) if need_root else None
            _lib.mb_bwd_dw(ix, hmat, din, gp, dout, dw, droot)
        if need_bias:
            dbias = g.sum(0)
        dw, dcomp = _own_param_grads(dw, wf, cp, need_wparam, need_comp)
        return dx, dw, dcomp, droot, dbias, None, None, None


def target_block(edge_index: Tensor, edge_type: Tensor, rows: Tensor, num_nodes: int) -> Tuple[Tensor, Tensor]:
    """The edges of a graph of ``num_nodes`` nodes whose destination is one of ``rows`` (int64, unique, in [0, num_nodes)), with
    the destination relabelled to its position in ``rows``: ``conv((x, x[rows]), *target_block(edge_index, edge_type, rows, N))``
    equals ``conv(x, edge_index, edge_type)[rows]`` and walks only those edges.  ALL edges into a kept row are kept (duplicates
    too), so a mean's normaliser is the full graph's.  Pure torch on the device of the edges.  The returned tensors are new and
    the plan cache keys on their identity: build them ONCE per (graph, rows) and keep them, or every call builds plans."""
    if rows.dim() != 1 or rows.dtype != torch.int64:
        raise ValueError(f"rows must be a 1-d int64 tensor, got {tuple(rows.shape)} {rows.dtype}")
    dev = edge_index.device
    rows = rows.to(dev)
    k = int(rows.shape[0])
    if k and (int(rows.min()) < 0 or int(rows.max()) >= num_nodes):
        raise ValueError(f"rows must lie in [0, {num_nodes})")
    pos = torch.full((max(int(num_nodes), 1),), -1, dtype=torch.int64, device=dev)
    pos[rows] = torch.arange(k, dtype=torch.int64, device=dev)
    if k and not bool((pos[rows] == torch.arange(k, dtype=torch.int64, device=dev)).all()):
        raise ValueError("rows must be unique")
    dst = pos[edge_index[1].long()]
    keep = dst >= 0
    return torch.stack([edge_index[0].long()[keep], dst[keep]]).contiguous(), edge_type[keep].contiguous()


# inverted indices of integer x (featureless layers), keyed on the index tensor's identity like the plan cache: the node ids
# sorted by x value and where each value starts -- built (and range-checked, one host synchronisation) once per x
_INDEX_CACHE: dict = {}
_INDEX_CACHE_MAX = 16


def _node_index(x: Tensor, in_rows: int):
    key = (x.data_ptr(), x._version, tuple(x.shape), x.dtype, str(x.device), in_rows)
    hit = _INDEX_CACHE.pop(key, None)
    if hit is None:
        x64 = x.to(torch.int64).contiguous()
        if x64.numel() and bool(((x64 < 0) | (x64 >= in_rows)).any()):
            raise ValueError(f"featureless RGCNConv: node indices must lie in [0, {in_rows})")
        vals, perm = torch.sort(x64, stable=True)
        ptr = torch.searchsorted(vals, torch.arange(in_rows + 1, device=x.device, dtype=torch.int64)).to(torch.int32)
        hit = ((x64, ptr, perm.to(torch.int32)), x)     # (hold x: its storage must not be recycled while cached)
        while len(_INDEX_CACHE) >= _INDEX_CACHE_MAX:
            _INDEX_CACHE.pop(next(iter(_INDEX_CACHE)))
    _INDEX_CACHE[key] = hit
    return hit[0]


def _require_gpu(*tensors: Optional[Tensor]) -> None:
    """there is no CPU path: every tensor given (None: skipped) must live on the GPU"""
    if any(t is not None and t.device.type != "cuda" for t in tensors):
        raise RuntimeError("RGCNConv runs only on an MI355X (ROCm 'cuda' device); there is no CPU fallback")


def _fused(activation: Optional[str], grad_premasked: bool) -> Tuple[int, bool]:
    """(the rgcn_act code of the activation fused into the forward store, whether its backward is left to the consumers of the
    output: only a ReLU's mask can be folded into their dX stores)"""
    if activation not in _ACT_CODES:
        raise ValueError(f"fused activation must be one of {list(_ACT_CODES)}")
    return _ACT_CODES[activation], bool(grad_premasked and activation == "relu")


def rgcn_conv_function(x: Tensor, weight: Tensor, root: Optional[Tensor], bias: Optional[Tensor],
                       plans: GraphPlans, dctx: Optional[DistContext] = None, activation: Optional[str] = None,
                       input_relu: bool = False, grad_premasked: bool = False, flags: int = 0,
                       comp: Optional[Tensor] = None, num_relations: Optional[int] = None, out_channels: Optional[int] = None,
                       xwide: bool = False) -> Tensor:
    """weight: dense [R, in, out]; or, with ``comp [R, B]``, the bases [B, in, out]; or blocks [R, nb, in / nb, out / nb]
    (then ``out_channels`` = nb * weight.shape[3]).  ``xwide``: the kernels of csrc/rgcn_xwide.hip (1..512 per side; ``plans``
    at rgcn_xwide_geometry, layout 0, single GPU)."""
    _require_gpu(x)
    act, premasked = _fused(activation, grad_premasked)
    _lib.load()
    if comp is not None:
        num_rel, dout = int(comp.shape[0]), int(weight.shape[2])
    elif weight.dim() == 4:
        num_rel, dout = int(weight.shape[0]), int(weight.shape[1] * weight.shape[3])
    else:
        num_rel, dout = int(weight.shape[0]), int(weight.shape[2])
    if xwide:
        if dctx is not None:
            raise NotImplementedError("RGCNConv wider than 128 runs on one GPU: a dist context is not supported")
        return _XwideFn.apply(x, weight, comp, root, bias, plans, act, bool(input_relu), premasked, num_relations or num_rel,
                              out_channels or dout)
    return _RGCNLayerFn.apply(x, weight, comp, root, bias, plans, dctx, act, bool(input_relu), premasked, int(flags),
                              num_relations or num_rel, out_channels or dout)


def _paths(path):
    """``RGCNConv.path`` as the routing and the plan cache key it: "auto" or a (forward, dX) pair"""
    return path if path == "auto" else ((path, path) if isinstance(path, str) else tuple(path))


# what RGCNConv._route decides: tile, chunk, plan layout (0, or 3: plan.compact_runs), d_weight on its own tile-major plan,
# FLAG_SPLIT_PRODUCERS (the bf16 x 3 forms of 64 x 64 layers), paths ("auto" or a (forward, dX) pair of "ring" / "ep")
_Route = namedtuple("_Route", "tile chunk layout dw_tiles split_producers paths")


def glorot_(t: Tensor) -> Tensor:
    """PyG ``glorot``: U(+-sqrt(6 / (size(-2) + size(-1))))"""
    bound = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    with torch.no_grad():
        return t.uniform_(-bound, bound)


class RGCNConv(nn.Module):
    r"""Drop-in for ``torch_geometric.nn.RGCNConv`` (PyG 2.3.1):

    ``RGCNConv(in_channels, out_channels, num_relations, num_bases=None, num_blocks=None,
    aggr='mean', root_weight=True, is_sorted=False, bias=True)``;
    ``forward(x[N,in] f32, edge_index[2,E] int64, edge_type[E] int64) -> [N,out] f32``.

    Parameters (registered in PyG's order): ``weight`` ``[R,in,out]`` (``[B,in,out]`` with
    ``num_bases=B``; ``[R,nb,in/nb,out/nb]`` with ``num_blocks=nb``), ``comp`` ``[R,B]`` or ``None``,
    ``root`` ``[in,out]`` or ``None``, ``bias`` ``[out]`` or ``None``.

    ``featureless=True`` (opt-in): PyG's featureless mode, ``x`` is ``None`` (then N = ``in_channels``) or an int64 ``[N]``
    node-index tensor and every table ``W_r [in,out]`` is a per-node embedding (``in_channels`` = table rows, any positive
    int); kernels of ``csrc/rgcn_featureless.hip``.  Not with ``num_blocks`` nor a ``dist`` context.

    ``wide`` (opt-in; ``None``: ``RGCN_WIDE=1`` in the environment at import time switches it on): up to 512 features per side.
    A layer with both sides at most 128 runs exactly as without it; one with a side above 128 runs on the kernels of
    ``csrc/rgcn_xwide.hip`` (exact fp32) -- one GPU, no ``dist`` context, ``path`` not pinned to ``"ep"``.  Not with ``featureless``.

    ``aggr="max"``: PyG's max aggregation -- ``H_r[i]`` = the column-wise max of ``x[src]`` over the edges of relation r into i
    (no edge: 0), ``out[i] = sum_r H_r[i] W_r + x[i] root + bias``, in full, basis and block modes; the gradient of a max is split
    evenly among the edges that attain it (torch ``scatter_reduce(..., "amax", include_self=False)``, duplicate edges counted).
    It runs on its own kernels (``csrc/rgcn_segmax.hip`` with the edge-parallel transform and sums; plan: ``eplan.MaxPlan``) and
    has one path: ``path`` and ``RGCN_PATH`` are ignored.  One GPU only (no ``dist`` context; ``edge_index`` / ``edge_type`` on
    the device of ``x``), up to 128 features per side, not with ``featureless``.

    Bipartite layers (PyG's ``in_channels=(in_src, in_dst)`` / ``x = (x_src, x_dst)``): ``weight`` takes ``in_src`` rows, ``root`` is
    ``[in_dst, out]``; ``forward((x_src [N_src, in_src], x_dst [N_dst, in_dst]), edge_index, edge_type) -> [N_dst, out]`` with
    ``edge_index[0] < N_src``, ``edge_index[1] < N_dst``: ``out[i] = sum_r aggr_r(x_src) W_r + x_dst[i] root + bias``, mean or sum,
    full, basis or block weights, gradients to both members and every parameter.  A tuple is accepted on a layer built with an int
    too (both widths equal); ``in_channels`` stays the source width, ``in_channels_l`` / ``in_channels_r`` name both.  The relations
    run on the plans and kernels of a homogeneous layer over rectangular node ranges, the root term on ``csrc/rgcn_rows.hip``
    (DESIGN.md 12).  One GPU, up to 128 features per side, no fused activation; not with ``featureless`` nor ``aggr="max"``.
    ``target_block`` cuts the edges into a set of target rows for ``conv((x, x[rows]), *block)``.
    """

    def __init__(self, in_channels: int, out_channels: int, num_relations: int,
                 num_bases: Optional[int] = None, num_blocks: Optional[int] = None, aggr: str = "mean",
                 root_weight: bool = True, is_sorted: bool = False, bias: bool = True, featureless: bool = False,
                 wide: Optional[bool] = None, **kwargs):
        super().__init__()
        if num_bases is not None and num_blocks is not None:
            raise ValueError("Can not apply both basis-decomposition and block-diagonal-decomposition "
                             "at the same time.")
        self.featureless = bool(featureless)
        if self.featureless and wide:
            raise ValueError("featureless RGCNConv has no wide mode: its tables stay at 1..128 columns")
        # (a featureless layer under RGCN_WIDE=1 keeps its own limit)
        self.wide = (_WIDE_DEFAULT if wide is None else bool(wide)) and not self.featureless
        if self.featureless:
            if num_blocks is not None:
                raise ValueError("Block-diagonal decomposition not supported for non-continuous input features.")
            if isinstance(in_channels, (tuple, list)) or int(in_channels) != in_channels or in_channels < 1:
                raise ValueError(f"featureless RGCNConv: in_channels is the number of table rows, got {in_channels!r}")
            if not 1 <= out_channels <= 128:
                raise ValueError(f"RGCNConv out_channels must be in 1..128, got {out_channels}")
        in_channels_r = in_channels
        if isinstance(in_channels, (tuple, list)):
            # PyG's bipartite form: (source width, destination width); `weight` takes the first, `root` the second
            if len(in_channels) != 2:
                raise ValueError(f"in_channels must be an int or a (source, destination) pair, got {in_channels!r}")
            in_channels, in_channels_r = int(in_channels[0]), int(in_channels[1])
        if aggr not in ("mean", "sum", "add", "max"):
            raise ValueError(f"unsupported aggr {aggr!r} (mean / sum / max)")
        if in_channels_r != in_channels:
            if aggr == "max":
                raise NotImplementedError("bipartite RGCNConv aggregates by mean / sum only: aggr='max' is not built")
            if self.wide and max(in_channels, in_channels_r, out_channels) > NARROW_MAX_WIDTH:
                raise NotImplementedError(f"bipartite RGCNConv takes 1..{NARROW_MAX_WIDTH} features per side, got "
                                          f"({in_channels}, {in_channels_r})->{out_channels} (wide layers are homogeneous)")
            if not 1 <= in_channels_r <= NARROW_MAX_WIDTH:
                raise ValueError(f"RGCNConv widths must be in 1..{NARROW_MAX_WIDTH}, got ({in_channels}, {in_channels_r})->{out_channels}")
        if aggr == "max" and self.featureless:
            raise ValueError("featureless RGCNConv has no max aggregation: aggr='max' takes float features x")
        if aggr == "max" and self.wide and max(in_channels, out_channels) > NARROW_MAX_WIDTH:
            raise NotImplementedError(f"RGCNConv(aggr='max') takes 1..{NARROW_MAX_WIDTH} features per side, got "
                                      f"{in_channels}->{out_channels} (wide layers aggregate by mean / sum only)")
        self.in_channels = in_channels         # the SOURCE width (what the plans gather), an int as every use means
        self.in_channels_l = in_channels       # PyG's name for it
        self.in_channels_r = in_channels_r     # the destination width: rows of `root` (differs in a bipartite layer only)
        self.out_channels = out_channels
        self.num_relations = num_relations
        self.num_bases = num_bases
        self.num_blocks = num_blocks
        self.aggr = "sum" if aggr == "add" else aggr
        self.is_sorted = is_sorted  # only meaningful for PyG's pyg_lib path; plans are order-independent
        self.dist: Optional[DistContext] = None
        self._dist_plans = None
        self.kernel_flags = 0     # RGCN_FLAG_* passed to every launch of this layer (tests pin kernel paths with it)
        self.dw_tiles = True      # d_weight by the tile-major kernel where it applies (_route); False: relation-major kernels
        # forward / dX on the producer-split bf16 x 3 kernel where it applies (64 x 64, 128-slot chunks, single GPU): fp32-
        # equivalent arithmetic (24-bit operand significands, exact products, fp32 accumulation), 1 ms per step faster at
        # the headline config.  False (or RGCN_SPLIT_PRODUCERS=0): the exact-fp32 MFMA kernel everywhere
        self.split_producers = _SPLIT_PRODUCERS_DEFAULT == "1"
        # "auto": per direction, the tile kernels or the edge-parallel path (csrc/rgcn_ep.hip), whichever eplan.choose_path
        # expects to be faster on the graph (many relations / few tiles / hubs -> edge-parallel); "ring" / "ep" or a
        # (forward, dX) pair pins it.  RGCN_PATH in the environment at import time sets the default.
        self.path = _PATH_DEFAULT
        # forward / dX plans in layout 3 where the producer-split kernel runs them and the tile-major kernel takes d_weight: the rows
        # of a (destination, relation) run on ONE slot, summed by the producers before the cut -- aggregate, then transform, as the
        # reference does; 13 % fewer row tiles at the headline config (plan.compact_runs).  RGCN_MERGE_RUNS=0 / False: layout 0
        self.merge_runs = _MERGE_RUNS_DEFAULT
        if num_bases is not None:
            self.weight = nn.Parameter(torch.empty(num_bases, in_channels, out_channels))
            self.comp = nn.Parameter(torch.empty(num_relations, num_bases))
        elif num_blocks is not None:
            assert in_channels % num_blocks == 0 and out_channels % num_blocks == 0, \
                "in_channels and out_channels must be divisible by num_blocks"
            self.weight = nn.Parameter(torch.empty(num_relations, num_blocks, in_channels // num_blocks,
                                                   out_channels // num_blocks))
            self.register_parameter("comp", None)
        else:
            self.weight = nn.Parameter(torch.empty(num_relations, in_channels, out_channels))
            self.register_parameter("comp", None)
        if root_weight:
            self.root = nn.Parameter(torch.empty(in_channels_r, out_channels))
        else:
            self.register_parameter("root", None)
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        if self.wide:
            if not (1 <= in_channels <= _lib.XWIDE_MAX_WIDTH and 1 <= out_channels <= _lib.XWIDE_MAX_WIDTH):
                raise ValueError(f"wide RGCNConv widths must be in 1..{_lib.XWIDE_MAX_WIDTH}, got {in_channels}->{out_channels}")
        elif not self.featureless:
            tile_for(in_channels, out_channels)  # validates the widths early
        self.reset_parameters()

    def reset_parameters(self) -> None:
        glorot_(self.weight)
        if self.comp is not None:
            glorot_(self.comp)
        if self.root is not None:
            glorot_(self.root)
        if self.bias is not None:
            with torch.no_grad():
                self.bias.zero_()

    def effective_weight(self) -> Tensor:
        """Dense ``[R, in, out]`` relation weights by differentiable torch ops -- NOT on the forward path (the library composes
        a decomposition inside its weight packer: rgcn_pack_weights_basis / _block); kept as the reference the tests compare
        that packer with.  Basis: ``(comp @ weight.view(B,-1)).view(R,in,out)``; block-diagonal: blocks placed on the diagonal
        of a zero matrix."""
        if self.num_bases is not None:
            return (self.comp @ self.weight.view(self.num_bases, -1)).view(
                self.num_relations, self.in_channels, self.out_channels)
        if self.num_blocks is not None:
            nb = self.num_blocks
            bi, bo = self.in_channels // nb, self.out_channels // nb
            eye = torch.eye(nb, device=self.weight.device, dtype=self.weight.dtype)
            # [R, nb, bi, bo] -> [R, nb, bi, nb, bo] with zeros off the block diagonal
            w = torch.einsum("rbio,bc->rbico", self.weight, eye)
            return w.reshape(self.num_relations, self.in_channels, self.out_channels)
        return self.weight

    def _plans(self, x: Tensor, edge_index: Tensor, edge_type: Tensor, route: Optional["_Route"] = None):
        """the (cached) plans of this layer on the graph: GraphPlans, or with ``self.dist`` the rank's RankPlans"""
        n = x.shape[0]
        r = self._route(n, int(edge_type.shape[0]), x.is_cuda) if route is None else route
        widths = (self.in_channels, self.out_channels)
        if self.dist is None:
            return cached_graph_plans(edge_index, edge_type, n, self.num_relations, r.tile, self.aggr, chunk=r.chunk, split=r.layout,
                                      dw_tiles=r.dw_tiles, paths=r.paths, widths=widths)
        from .dist import cached_rank_plans
        return cached_rank_plans(edge_index, edge_type, n, self.num_relations, r.tile, self.aggr, self.dist, r.chunk, r.layout,
                                 r.dw_tiles, paths=r.paths, widths=widths)

    @property
    def _w64(self) -> bool:
        """both sides pad to 64 columns: the layers of the producer-split kernel, layout 3 and the tile-major d_weight kernel"""
        return padded_width(self.in_channels) == 64 and padded_width(self.out_channels) == 64

    def _use_split_producers(self, chunk: int) -> bool:
        """whether a plan of this layer with that chunk runs on the bf16 x 3 kernel (FLAG_SPLIT_PRODUCERS, _route)"""
        return self.split_producers and chunk in (112, 128) and self._w64

    @property
    def xwide(self) -> bool:
        """whether this layer runs on the kernels of csrc/rgcn_xwide.hip: ``wide`` and a side above 128"""
        return self.wide and max(self.in_channels, self.out_channels) > NARROW_MAX_WIDTH

    def _route(self, n_nodes: int, n_edges: int, on_gpu: bool, plain: bool = False) -> "_Route":
        """Every kernel choice of this layer on a graph of that size (``on_gpu``: its tensors are on the device).  The tile is
        ``layout_for``'s, capped at the producer-split kernel's tile where that kernel will run (dist.attach aligns the ranks' node
        ranges to it), or at the tile that leaves the exact-fp32 kernel room for shadow row tiles where it walks layout-3 plans.
        ``plain`` (bipartite layers): as with ``merge_runs`` and ``dw_tiles`` off -- layout 0, relation-major d_weight kernels."""
        if self.xwide:
            raise NotImplementedError("RGCNConv wider than 128 runs on one GPU only: no dist layout")
        if self.aggr == "max":
            raise NotImplementedError("RGCNConv(aggr='max') runs on one GPU only: a dist context is not supported")
        tile, chunk = layout_for(self.in_channels, self.out_channels, n_nodes, n_edges, self.num_relations)
        # the tile-major weight-gradient kernel: 64 x 64 layers with few relations on graphs large enough to fill it
        dw_rule = self.dw_tiles and not plain and self._w64 and self.num_relations <= 32 and n_edges >= DW_TILES_MIN_EDGES
        exact_merge = False
        if self._use_split_producers(128):
            # the bf16 x 3 kernel's own layout (128-slot chunks, tiles up to 224, its own cycles per chunk and row tile) against the
            # exact-fp32 kernel's, by modelled launch time -- round 4: on a 100k-node / 1M-edge graph the exact model's (400, 64)
            # kept the layer off the faster kernel: 0.416 ms per step replayed against 0.333 at (208, 128)
            args = (n_nodes, n_edges, self.num_relations, self.in_channels, self.out_channels)
            t3, c3, cost3 = choose_layout(*args, kernel="bf16x3", with_cost=True)
            if cost3 <= choose_layout(*args, with_cost=True)[2]:
                tile, chunk = t3, c3
            elif chunk == 128:      # (the exact-fp32 kernel with 128-slot chunks would be taken for the other one: keep it on 64)
                tile = min(tile, SPLIT_PRODUCERS_TILE)
        else:
            # the exact-fp32 kernel on layout-3 plans.  The cap asks the dW-tiles rule of the graph's size only, not whether the
            # tile-major kernel can address x and g (dw_tiles below): the tile sets the summation order of every output, layout()
            # and dist.attach ask without tensors, and past 2^24 rows / 4 GiB the capped tile stays on layout 0
            exact_merge = self.merge_runs and chunk == 128 and self._w64
            if exact_merge and dw_rule and self.kernel_flags == 0:
                tile = min(tile, EXACT_MERGE_TILE)
        split = self._use_split_producers(chunk)
        # (the tile-major kernel gathers through buffer descriptors only: above 2^24 rows / 4 GiB the relation-major kernels run)
        dw_tiles = (dw_rule and on_gpu and _lib.buffer_addressable(n_nodes, _round4(self.in_channels))
                    and _lib.buffer_addressable(n_nodes, _round4(self.out_channels)))
        # layout 3 only where nothing but rgcn_tile3p_kernel walks the forward / transposed plans: the split kernels unpinned
        # (no kernel flags), d_weight on its own tile-major plan, d_root / d_bias on the plan-free streaming kernel
        layout = 3 if self.merge_runs and dw_tiles and self.kernel_flags == 0 and (split or exact_merge) else 0
        return _Route(tile, chunk, layout, dw_tiles, split, _paths(self.path) if on_gpu else ("ring", "ring"))

    def layout(self, n_nodes: int, n_edges: int) -> Tuple[int, int]:
        """(tile, chunk) of this layer's plans on a graph of that size (``_route``; they do not depend on the device)"""
        if self.aggr == "max":
            raise NotImplementedError("RGCNConv(aggr='max') has no tile layout: it runs on its own edge-parallel plan (eplan.MaxPlan)")
        r = self._route(n_nodes, n_edges, False)
        return r.tile, r.chunk

    def forward(self, x: Tensor, edge_index: Tensor, edge_type: Optional[Tensor] = None, *,
                _activation: Optional[str] = None, _input_relu: bool = False,
                _grad_premasked: bool = False) -> Tensor:
        """PyG's ``forward(x, edge_index, edge_type)``; ``x`` a ``(x_src, x_dst)`` pair: the bipartite layer (class docstring).
        The keyword-only arguments are the private hook the model
        wrappers use to fuse the activations either side of the layer (layers._RGCNStack._tail):
        ``_activation`` ('relu' | 'sigmoid') is applied in the forward kernel's store; ``_input_relu`` says x is the
        ReLU output of the previous layer, so the dX kernel stores dL/dz_prev = dX * (x > 0); ``_grad_premasked`` says
        every consumer of THIS layer's ReLU output does that, so no ReLU backward runs here."""
        assert edge_type is not None, "edge_type is required (PyG RGCNConv asserts the same)"
        if isinstance(x, (tuple, list)):
            return self._forward_bipartite(x, edge_index, edge_type, _activation, _input_relu, _grad_premasked)
        if self.featureless:
            return self._forward_featureless(x, edge_index, edge_type)
        if self.in_channels_r != self.in_channels:
            raise ValueError(f"this RGCNConv was built with in_channels=({self.in_channels}, {self.in_channels_r}): "
                             f"x must be a (x_src, x_dst) pair")
        if x is None or not torch.is_floating_point(x):
            raise NotImplementedError("featureless (integer / None x) RGCNConv is never used by the reference "
                                      "(x is always float: model/layers.py:21,62,108) and is not built")
        if x.dim() != 2 or x.shape[1] != self.in_channels:
            raise ValueError(f"x must be [N, {self.in_channels}], got {tuple(x.shape)}")
        if self.aggr == "max":
            return self._forward_max(x, edge_index, edge_type, _activation, _input_relu, _grad_premasked)
        if self.xwide:
            return self._forward_xwide(x, edge_index, edge_type, _activation, _input_relu, _grad_premasked)
        route = self._route(x.shape[0], int(edge_type.shape[0]), x.is_cuda)
        plans = self._plans(x, edge_index, edge_type, route)
        # rgcn_fwd / rgcn_bwd_dx / rgcn_bwd_dw_tiles / rgcn_ep_transform: the bf16 x 3 (fp32-equivalent) forms of 64 x 64 layers
        # where they fit.  (The mode follows the route's chunk, not which path the other direction happened to take.)
        flags = self.kernel_flags | (_lib.FLAG_SPLIT_PRODUCERS if route.split_producers else 0)
        return rgcn_conv_function(x, self.weight, self.root, self.bias, plans, self.dist, _activation, _input_relu, _grad_premasked, flags,
                                  comp=self.comp, num_relations=self.num_relations, out_channels=self.out_channels)

    def _forward_xwide(self, x: Tensor, edge_index: Tensor, edge_type: Tensor, activation: Optional[str], input_relu: bool,
                       grad_premasked: bool) -> Tensor:
        if self.dist is not None:
            raise NotImplementedError("RGCNConv wider than 128 runs on one GPU: a dist context is not supported")
        paths = _paths(self.path)
        if paths != "auto" and "ep" in paths:
            raise ValueError("RGCNConv wider than 128 has no edge-parallel path: path must be 'auto' or 'ring'")
        _require_gpu(x)
        n = int(x.shape[0])
        tile, chunk = _lib.xwide_geometry(max(n, 1), self.in_channels, self.out_channels)
        plans = cached_graph_plans(edge_index, edge_type, n, self.num_relations, tile, self.aggr, chunk=chunk, extra_key=("xwide",))
        return rgcn_conv_function(x, self.weight, self.root, self.bias, plans, None, activation, input_relu, grad_premasked, 0,
                                  comp=self.comp, num_relations=self.num_relations, out_channels=self.out_channels, xwide=True)

    def _forward_max(self, x: Tensor, edge_index: Tensor, edge_type: Tensor, activation: Optional[str], input_relu: bool,
                     grad_premasked: bool) -> Tensor:
        if self.dist is not None:
            raise NotImplementedError("RGCNConv(aggr='max') runs on one GPU: a dist context is not supported")
        _require_gpu(x)
        if edge_index.device != x.device or edge_type.device != x.device:
            # (the plan is built where the edges live: a CPU plan's index arrays must never reach a kernel)
            raise RuntimeError(f"RGCNConv(aggr='max'): edge_index ({edge_index.device}) and edge_type ({edge_type.device}) must be on "
                               f"the device of x ({x.device})")
        act, premasked = _fused(activation, grad_premasked)
        _lib.load()
        from .eplan import build_max_plan
        n, r = int(x.shape[0]), self.num_relations
        mp = cached_graph_plans(edge_index, edge_type, n, r, 0, "max", paths=("ep", "ep"), extra_key=("max",),
                                builder=lambda paths: build_max_plan(edge_index, edge_type, n, r))
        # the bf16 x 3 (fp32-equivalent) transform of 64 x 64 layers, as on the edge-parallel path
        flags = self.kernel_flags | (_lib.FLAG_SPLIT_PRODUCERS if self.split_producers and self._w64 else 0)
        return _MaxLayerFn.apply(x, self.weight, self.comp, self.root, self.bias, mp, act, bool(input_relu), premasked, int(flags), r,
                                 self.out_channels)

    def _forward_bipartite(self, x, edge_index: Tensor, edge_type: Tensor, activation: Optional[str], input_relu: bool,
                           grad_premasked: bool) -> Tensor:
        """``x = (x_src [N_src, in_src], x_dst [N_dst, in_dst])``, ``edge_index[0] < N_src``, ``edge_index[1] < N_dst`` ->
        ``[N_dst, out]`` (_BipartiteFn).  Every refusal comes before a plan is built."""
        if self.featureless:
            raise NotImplementedError("featureless RGCNConv takes x = None or node indices: a (x_src, x_dst) pair is not built")
        if self.aggr == "max":
            raise NotImplementedError("bipartite RGCNConv aggregates by mean / sum only: aggr='max' is not built")
        if self.xwide:
            raise NotImplementedError(f"bipartite RGCNConv takes 1..{NARROW_MAX_WIDTH} features per side (wide layers are homogeneous)")
        if self.dist is not None:
            raise NotImplementedError("bipartite RGCNConv runs on one GPU: a dist context is not supported")
        if activation is not None or input_relu or grad_premasked:
            raise ValueError("bipartite RGCNConv fuses no activation: _activation / _input_relu / _grad_premasked must be unset")
        if len(x) != 2:
            raise ValueError(f"x must be a (x_src, x_dst) pair, got {len(x)} members")
        x_src, x_dst = x
        for t in (x_src, x_dst):
            if not isinstance(t, Tensor) or not torch.is_floating_point(t):
                raise NotImplementedError("bipartite RGCNConv takes float features on both sides (no None / integer member)")
        if x_src.dim() != 2 or x_src.shape[1] != self.in_channels:
            raise ValueError(f"x_src must be [N_src, {self.in_channels}], got {tuple(x_src.shape)}")
        if x_dst.dim() != 2 or x_dst.shape[1] != self.in_channels_r:
            raise ValueError(f"x_dst must be [N_dst, {self.in_channels_r}], got {tuple(x_dst.shape)}")
        if x_src.dtype != torch.float32 or x_dst.dtype != torch.float32:
            raise ValueError(f"x_src and x_dst must be float32, got {x_src.dtype} and {x_dst.dtype}")
        if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_type.dim() != 1 or edge_index.shape[1] != edge_type.shape[0]:
            raise ValueError(f"edge_index must be [2, E] and edge_type [E], got {tuple(edge_index.shape)} and {tuple(edge_type.shape)}")
        _require_gpu(x_src, x_dst)
        dev = x_src.device
        if x_dst.device != dev or edge_index.device != dev or edge_type.device != dev:
            # (the plan is built where the edges live: a CPU plan's index arrays must never reach a kernel)
            raise RuntimeError(f"bipartite RGCNConv: x_dst ({x_dst.device}), edge_index ({edge_index.device}) and edge_type "
                               f"({edge_type.device}) must be on the device of x_src ({dev})")
        _lib.load()
        n_src, n_dst, e, r = int(x_src.shape[0]), int(x_dst.shape[0]), int(edge_type.shape[0]), self.num_relations
        n = max(n_src, n_dst)
        if e and min(n_src, n_dst) == 0:
            raise ValueError(f"edge_index out of range: {e} edges between {n_src} source and {n_dst} destination nodes")
        plans, flags = None, self.kernel_flags
        if n_dst > 0:
            route = self._route(n, e, True, plain=True)
            plans = self._bipartite_plans(edge_index, edge_type, n_src, n_dst, route)
            flags |= _lib.FLAG_SPLIT_PRODUCERS if route.split_producers else 0
        return _BipartiteFn.apply(x_src, x_dst, self.weight, self.comp, self.root, self.bias, plans, int(flags), r, self.out_channels)

    def forward_block(self, x: Tensor, block, index=None) -> Tensor:
        """``conv((x, x[:block.n_dst]), block.edge_index, block.edge_type)`` for a ``sampling.Block`` whose destinations are its
        first ``n_dst`` source rows, on the kernels of ``csrc/rgcn_minibatch.hip``: ``x [n_src, in]`` float32 ->
        ``[n_dst, out]``, mean or sum, full, basis or block weights, gradients to ``x`` (source side plus, in its first ``n_dst``
        rows, the root term) and every parameter.  No graph plan is built and nothing is cached: ``index`` is the block's
        ``sampling.block_index(block, num_relations, aggr)``, built here when not given; no order is required of the edges.
        One GPU, 1..128 features per side, no fused activation.  Every refusal comes before anything is launched."""
        if self.featureless:
            raise NotImplementedError("featureless RGCNConv takes x = None or node indices: forward_block is not built for it")
        if self.aggr == "max":
            raise NotImplementedError("RGCNConv.forward_block aggregates by mean / sum only: aggr='max' is not built")
        if self.xwide:
            raise NotImplementedError(f"RGCNConv.forward_block takes 1..{NARROW_MAX_WIDTH} features per side: wide layers are not built")
        if self.dist is not None:
            raise NotImplementedError("RGCNConv.forward_block runs on one GPU: a dist context is not supported")
        if self.in_channels_r != self.in_channels:
            raise NotImplementedError(f"RGCNConv.forward_block reads the destinations' rows from x itself: a layer built with "
                                      f"in_channels=({self.in_channels}, {self.in_channels_r}) is not supported")
        if not isinstance(x, Tensor) or not torch.is_floating_point(x):
            raise NotImplementedError("RGCNConv.forward_block takes float features x (no None / integer / pair input)")
        if x.dtype != torch.float32:
            raise ValueError(f"x must be float32, got {x.dtype}")
        if x.dim() != 2 or x.shape[1] != self.in_channels:
            raise ValueError(f"x must be [n_src, {self.in_channels}], got {tuple(x.shape)}")
        n_src, n_dst = int(block.n_src), int(block.n_dst)
        if n_dst > n_src:
            raise ValueError(f"a block's destinations are its first source rows: n_dst ({n_dst}) exceeds n_src ({n_src})")
        if x.shape[0] != n_src:
            raise ValueError(f"x must hold the block's {n_src} source rows, got {x.shape[0]}")
        ei, et = block.edge_index, block.edge_type
        if ei.dim() != 2 or ei.shape[0] != 2 or et.dim() != 1 or ei.shape[1] != et.shape[0]:
            raise ValueError(f"edge_index must be [2, E] and edge_type [E], got {tuple(ei.shape)} and {tuple(et.shape)}")
        _require_gpu(x)
        if ei.device != x.device or et.device != x.device:
            raise RuntimeError(f"RGCNConv.forward_block: edge_index ({ei.device}) and edge_type ({et.device}) must be on the device "
                               f"of x ({x.device})")
        if index is None:
            from .sampling import block_index
            index = block_index(block, self.num_relations, self.aggr)
        elif (index.n_src, index.n_dst, index.num_edges, index.num_relations, index.aggr) != \
                (n_src, n_dst, int(et.shape[0]), self.num_relations, self.aggr) or index.device != x.device:
            raise ValueError("index does not belong to this block and layer (sizes, relations, aggregation or device differ)")
        _lib.load()
        return _BlockFn.apply(x, self.weight, self.comp, self.root, self.bias, index, self.num_relations, self.out_channels)

    def _bipartite_plans(self, edge_index: Tensor, edge_type: Tensor, n_src: int, n_dst: int,
                         route: Optional["_Route"] = None) -> GraphPlans:
        """the (cached) plans of a bipartite call with N_dst > 0: those of a homogeneous in_src -> out layer on N = max(N_src,
        N_dst) nodes that owns the rows [0, N_dst) forward and [0, N_src) transposed -- what a rank of a partitioned layer builds
        """
        e, r = int(edge_type.shape[0]), self.num_relations
        n = max(n_src, n_dst)
        route = self._route(n, e, True, plain=True) if route is None else route

        def build(paths):
            # the builder checks every id against N only: the side ranges here, one reduction, on a cache miss only
            if e:
                top = edge_index.amax(dim=1).tolist()
                if top[0] >= n_src or top[1] >= n_dst:
                    raise ValueError(f"edge_index out of range: sources must lie in [0, {n_src}), destinations in [0, {n_dst}) "
                                     f"(largest: {top[0]}, {top[1]})")
            return build_graph_plans(edge_index, edge_type, n, r, route.tile, self.aggr, fwd_range=(0, n_dst),
                                     bwd_range=(0, n_src or n), chunk=route.chunk, paths=paths)

        return cached_graph_plans(edge_index, edge_type, n, r, route.tile, self.aggr, builder=build,
                                  extra_key=("bipartite", n_src, n_dst), chunk=route.chunk, paths=route.paths,
                                  widths=(self.in_channels, self.out_channels))

    def _forward_featureless(self, x: Optional[Tensor], edge_index: Tensor, edge_type: Tensor) -> Tensor:
        if self.dist is not None:
            raise NotImplementedError("featureless RGCNConv runs on one GPU: a dist context is not supported")
        if x is not None:
            if torch.is_floating_point(x) or torch.is_complex(x) or x.dtype == torch.bool:
                raise ValueError("featureless RGCNConv takes x = None or an integer node-index tensor, not float features")
            if x.dim() != 1:
                raise ValueError(f"featureless RGCNConv: x must be a [N] node-index tensor, got {tuple(x.shape)}")
        _require_gpu(edge_index, x)
        _lib.load()
        n = self.in_channels if x is None else int(x.shape[0])
        index = None if x is None else _node_index(x, self.in_channels)
        nb = 0 if self.num_bases is None else int(self.num_bases)
        tile, chunk = _lib.featureless_geometry(max(n, 1), self.out_channels, nb)
        plans = cached_graph_plans(edge_index, edge_type, n, self.num_relations, tile, self.aggr, chunk=chunk,
                                   extra_key=("featureless",))
        return _FeaturelessFn.apply(self.weight, self.comp, self.root, self.bias, plans, index, self.in_channels,
                                    self.out_channels)

    def __repr__(self) -> str:
        return (f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, "
                f"num_relations={self.num_relations})")
