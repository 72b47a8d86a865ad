"""Graph plan: the HBM layout the HIP kernels walk.

Built once per (graph, tile size, direction, node range) from the COO tensors the
reference hands to the layer (``edge_index[2,E]`` int64, ``edge_type[E]`` int64, unsorted,
duplicates kept: /root/reference/graphs/graph.py:55-69) and cached, so the public
``forward(x, edge_index, edge_type)`` signature stays PyG's (SURVEY.md 8b "Ownership").
PyG recomputes masks and counts on every call; here they are computed once.

Layout (all int32 / float32, device resident):

* output nodes of the owned range ``[node_begin, node_end)`` are cut into TILES of ``tile``
  consecutive nodes; one workgroup owns a tile's accumulator in LDS;
* the edges scattering into a tile are grouped by relation; each (tile, relation) group is cut
  into CHUNKS of ``CHUNK`` = 64 edge slots (the last one padded), so a chunk is
  relation-homogeneous (one MFMA B operand) and exactly one LDS-DMA ring slot;
* the self-loop (PyG ``root``) is relation id ``num_relations`` with one pseudo edge per node;
* per slot: ``slot_src`` (row to gather; padding = ``n_nodes``, one past the last row, which a buffer-descriptor
  gather turns into zeros by its range check), ``slot_w`` (edge weight
  ``1 / max(1, c[dst, rel])`` for ``aggr='mean'``, 0 = padding), ``slot_dstl`` (row inside the tile,
  ``tile`` = padding; host-side only) and ``slot_row`` (the same as a row of the owned range, padding = one past the
  end: what the dW kernel gathers the upstream gradient by); inside a chunk the slots are
  sorted by ``slot_dstl``, which the forward kernel's run-sum relies on; ``slot_acc`` packs what that
  run-sum needs per slot (run-end position << 24 | accumulator row, see ``run_metadata``);
  duplicate (src, dst, relation) triples share ONE slot whose weight is the sum of theirs;
* per chunk: ``chunk_rel``, ``chunk_cnt`` (slots of the used 16-slot row tiles), ``chunk_tile``, ``chunk_flags``; ``tile_ptr`` gives the tile-major
  chunk ranges (forward / dX kernels) and ``rel_order`` the relation-major order (dW kernel).

The transposed plan (``direction='bwd'``) swaps the roles of source and destination and keeps
the forward weights, so dX is the same kernel run on it with W_r^T (SURVEY.md 7 "Backward dX
without atomics").  Everything here is torch tensor plumbing and runs on CPU or GPU alike.
"""
from __future__ import annotations

import functools
import os as _os

import numpy as np
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from .eplan import (HEAVY, PIECE, EdgePlan, SharedHeavy, _finish_levels, build_edge_plan, build_heavy_part, check_ep_ranges,
                    heavy_mask, resolve_paths, shared_heavy_part)

CHUNK = 64  # default edge slots per chunk == rows of one LDS ring slot (csrc/rgcn_common.h kChunk)
UNIT = 64   # rows the weight-gradient kernels walk at a time: a chunk is chunk // UNIT units
CHUNKS = (64, 128)   # chunk sizes (slot strides) the kernels are built for
CHUNK_112 = 112      # as the ``chunk`` argument of the builders: 128-slot chunks that hold at most SEVEN row tiles (112 rows) of rows
                     # -- what rgcn_tile3p_kernel's 42 KiB ring slots hold, leaving its accumulator room for tiles up to 272
                     # (TilePlan.chunk stays 128, TilePlan.chunk_rows says 112)


@dataclass
class TilePlan:
    n_nodes: int          # nodes of the whole graph (rows of the gathered matrix)
    node_begin: int       # first owned output node (multiple of tile)
    node_end: int         # one past the last owned output node
    num_relations: int    # R' (the root pseudo relation is id R')
    tile: int
    chunk: int            # edge slots per chunk (64 or 128)
    n_tiles: int
    n_chunks: int
    n_edges: int          # real edges placed (before merging duplicate triples; no root / padding)
    tile_ptr: Tensor      # int32 [n_tiles + 1]
    chunk_rel: Tensor     # int32 [n_chunks]
    chunk_cnt: Tensor     # int32 [n_chunks]
    chunk_tile: Tensor    # int32 [n_chunks]
    chunk_flags: Tensor   # int32 [n_chunks]  bit t: MFMA row tile t of the chunk holds a repeated destination
                          # (layout 5: bits 28-30 = which halves of a packed unit hold rows of chunk_tile + 1, see dw_pack)
    rel_order: Tensor     # int32 [n_units]  non-empty 64-row units (unit u = rows [64 u, 64 u + 64) of the slot
                          #   arrays, chunk u // (chunk // 64)), relation-major then tile: the dW kernels' walk
    slot_src: Tensor      # int32 [n_chunks * chunk]
    slot_w: Tensor        # float32 [n_chunks * chunk]
    slot_dstl: Optional[Tensor]   # int32 [n_chunks * chunk]  row inside the tile (padding: tile); host-side checks only:
                          #   None for plans built on the device
    slot_row: Tensor      # int32 [n_chunks * chunk]  row inside the owned range = tile index * tile + slot_dstl (padding: n_owned)
    slot_acc: Tensor      # int32 [n_chunks * chunk]  run-end position << 24 | accumulator row
    layout: int = 0       # 0: rows of a group dealt over all its row tiles; 1: team placement (team_placement);
    #                       3: layout 0 with the runs of equal (destination, relation) on one slot each (compact_runs)
    chunk_rows: int = 0   # rows a chunk may hold: 0 / chunk, or 112 (chunk = 128: seven row tiles of rows per chunk)
    slot_src2: Optional[Tensor] = None    # layout 5 (the tile-major weight-gradient plan): int32 [n_chunks * 8] second rows of the
                                          # slots 0..3 and 32..35 of every unit (padding: n_nodes), see dw_pairs
    _keep: tuple = field(default=(), repr=False)

    @property
    def device(self):
        return self.slot_src.device

    @property
    def n_owned(self) -> int:
        return self.node_end - self.node_begin

    @property
    def n_units(self) -> int:
        return int(self.rel_order.shape[0])

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (
            self.tile_ptr, self.chunk_rel, self.chunk_cnt, self.chunk_tile, self.chunk_flags, self.rel_order,
            self.slot_src, self.slot_w, self.slot_row, self.slot_acc))


def edge_weights(src: Tensor, dst: Tensor, rel: Tensor, num_relations: int, aggr: str = "mean") -> Tensor:
    """w_e = 1 / max(1, c[dst_e, rel_e]) (duplicates counted), float32, in input edge order; 1 for "sum" / "add" and for "max"
    (an edge's multiplicity: its weight in the tie count of a max, eplan.MaxPlan)."""
    if aggr in ("sum", "add", "max"):
        return torch.ones(dst.shape[0], dtype=torch.float32, device=dst.device)
    if aggr != "mean":
        raise ValueError(f"unsupported aggr {aggr!r}")
    key = dst.to(torch.int64) * num_relations + rel.to(torch.int64)
    skey, perm = torch.sort(key)
    _, inv, cnt = torch.unique_consecutive(skey, return_inverse=True, return_counts=True)
    w_sorted = 1.0 / cnt.to(torch.float32)[inv]
    w = torch.empty_like(w_sorted)
    w[perm] = w_sorted
    return w


def build_plan(gather: Tensor, scatter: Tensor, rel: Tensor, w: Tensor, n_nodes: int,
               num_relations: int, tile: int, node_begin: int = 0,
               node_end: Optional[int] = None, chunk: int = CHUNK, split: bool = False) -> TilePlan:
    """Lay out the edges scattering into ``[node_begin, node_end)``.

    gather / scatter: int64 [E] node ids (forward: src / dst; transposed: dst / src).
    chunk: edge slots per chunk (one of CHUNKS).
    split: the plan layout -- False / 0: layout 0; True / 1: the TEAM placement (128-slot chunks only), see ``team_placement``;
           3: layout 0 followed by ``compact_runs`` (128-slot chunks only).
    """
    cap = None            # row tiles a chunk may hold (None: chunk / 16)
    if chunk == CHUNK_112:
        if int(split) not in (0, 3):
            raise ValueError("112-row chunks: layouts 0 and 3 only")
        if int(split) == 3:
            return compact_runs(build_plan(gather, scatter, rel, w, n_nodes, num_relations, tile, node_begin, node_end, chunk, False))
        chunk, cap = 128, 7
    if chunk not in CHUNKS:
        raise ValueError(f"chunk must be one of {CHUNKS} (or {CHUNK_112})")
    if int(split) == 5:
        if chunk != 64:
            raise ValueError("layout 5 (pairs on one slot: the tile-major weight-gradient plan) needs 64-slot chunks")
        return dw_pack(dw_pairs(build_plan(gather, scatter, rel, w, n_nodes, num_relations, tile, node_begin, node_end, chunk, False)))
    if split and chunk != 128:
        raise ValueError("the team placement and the run compaction need 128-slot chunks")
    if int(split) == 3:
        return compact_runs(build_plan(gather, scatter, rel, w, n_nodes, num_relations, tile, node_begin, node_end, chunk, False))
    CHUNK = chunk  # noqa: N806  (shadows the module default inside this function)
    if node_end is None:
        node_end = n_nodes
    if node_end <= node_begin:
        return empty_plan(n_nodes, node_begin, num_relations, tile, chunk, gather.device, 1 if split else 0)
    if node_begin % tile != 0:
        raise ValueError("node_begin must be a multiple of the tile size")
    dev = gather.device
    n_own = node_end - node_begin
    r1 = num_relations + 1
    gather = gather.to(torch.int64)
    scatter = scatter.to(torch.int64)
    rel = rel.to(torch.int64)
    if rel.numel() and (int(rel.min()) < 0 or int(rel.max()) >= num_relations):
        raise ValueError("edge_type out of range [0, num_relations)")
    if gather.numel() and (int(gather.min()) < 0 or int(gather.max()) >= n_nodes
                           or int(scatter.min()) < 0 or int(scatter.max()) >= n_nodes):
        raise ValueError("edge_index out of range [0, num_nodes)")
    own = (scatter >= node_begin) & (scatter < node_end)
    if not bool(own.all()):
        gather, scatter, rel, w = gather[own], scatter[own], rel[own], w[own]
    n_edges = int(gather.shape[0])
    # root pseudo edges: node i gathers its own row with weight 1 under relation id R'
    nodes = torch.arange(node_begin, node_end, device=dev, dtype=torch.int64)
    g_all = torch.cat([gather, nodes])
    loc = torch.cat([scatter, nodes]) - node_begin
    r_all = torch.cat([rel, torch.full((n_own,), num_relations, device=dev, dtype=torch.int64)])
    w_all = torch.cat([w.to(torch.float32), torch.ones(n_own, device=dev, dtype=torch.float32)])
    tile_id = loc // tile
    dstl = loc - tile_id * tile
    key = (tile_id * r1 + r_all) * tile + dstl
    # Sort by (tile, relation, row in tile, gathered node) and MERGE duplicate (gather, scatter, relation)
    # triples into one slot whose weight is the sum of theirs (m / c for a triple repeated m times):
    # identical under the multiset semantics of the layer, but a repeated triple is gathered and
    # multiplied once, and -- decisive for the reference's summary graphs, where ~50k edges join 44
    # nodes -- thousands of bit-identical terms are no longer added one by one into an fp32
    # accumulator (that sum has a systematic rounding bias ~n*u; it cost 4e-4 on AIFB_sum_in).
    key2, perm = torch.sort(key * n_nodes + g_all)
    w_all = w_all[perm]
    key2, inv, mult = torch.unique_consecutive(key2, return_inverse=True, return_counts=True)
    if key2.shape[0] != w_all.shape[0]:
        w_all = torch.zeros(key2.shape[0], dtype=torch.float64, device=dev).index_add_(
            0, inv, w_all.to(torch.float64)).to(torch.float32)
    key = key2 // n_nodes
    g_all = key2 - key * n_nodes
    dstl = key % tile
    gk = key // tile
    gvals, gcnt = torch.unique_consecutive(gk, return_counts=True)
    per = cap if cap is not None else CHUNK // ROWS_PER_MFMA_TILE       # row tiles a chunk holds
    gch = ((gcnt + 15) // 16 + (per - 1)) // per if cap is not None else (gcnt + (CHUNK - 1)) // CHUNK
    chunk_base = torch.cumsum(gch, 0) - gch
    n_chunks = int(gch.sum())
    n_groups = gvals.shape[0]
    gstart = torch.cumsum(gcnt, 0) - gcnt
    grp_of_edge = torch.repeat_interleave(torch.arange(n_groups, device=dev), gcnt)
    rank = torch.arange(key.shape[0], device=dev) - gstart[grp_of_edge]
    # Row j of a group (sorted by destination) goes to MFMA row tile (j mod nt), position (j div nt), nt =
    # ceil(n / 16): every tile stays sorted by destination, the tiles of a group are equally full, and a run
    # of c equal destinations is spread over c different tiles (c <= nt), so most tiles hold pairwise distinct
    # destinations and the forward kernel can skip its run-sum product for them (chunk_flags).
    g16 = ROWS_PER_MFMA_TILE
    gnt = (gcnt + (g16 - 1)) // g16
    grp_of_chunk = torch.repeat_interleave(torch.arange(n_groups, device=dev), gch)
    idx_in_grp = torch.arange(n_chunks, device=dev) - chunk_base[grp_of_chunk]
    straddle = None
    if not split:
        nt_e = gnt[grp_of_edge]
        t_e = rank % nt_e                         # the group's row tile: chunk t // per of the group, its row tile t % per
        slot = (chunk_base[grp_of_edge] + t_e // per) * CHUNK + (t_e % per) * g16 + rank // nt_e
        # slots of the chunk's used row tiles (a multiple of 16; padding sits at the end of every tile)
        chunk_cnt = (torch.clamp(gnt[grp_of_chunk] - idx_in_grp * per, max=per) * g16).to(torch.int32)
    else:
        slot, chunk_cnt, straddle = team_placement(dstl, gcnt, grp_of_edge, rank, chunk_base, grp_of_chunk, idx_in_grp)
    n_slots = n_chunks * CHUNK
    slot_src = torch.full((n_slots,), n_nodes, dtype=torch.int32, device=dev)  # padding: one past the last row
    slot_w = torch.zeros(n_slots, dtype=torch.float32, device=dev)
    slot_dstl = torch.full((n_slots,), tile, dtype=torch.int32, device=dev)  # padding -> dummy accumulator row
    slot_src[slot] = g_all.to(torch.int32)
    slot_w[slot] = w_all
    slot_dstl[slot] = dstl.to(torch.int32)
    slot_acc, tile_dup = run_metadata(slot_dstl, tile)
    chunk_flags = (tile_dup.view(-1, CHUNK // g16).to(torch.int32)
                   * (2 ** torch.arange(CHUNK // g16, device=dev, dtype=torch.int32))).sum(1).to(torch.int32)
    if straddle is not None:
        chunk_flags = chunk_flags | (straddle.to(torch.int32) << 8)
    # the dW kernel gathers the upstream-gradient row of every slot: its index in the owned range
    tile_of_slot = torch.repeat_interleave((gvals[grp_of_chunk] // r1).to(torch.int32), CHUNK)
    slot_row = torch.where(slot_dstl < tile, tile_of_slot * tile + slot_dstl,
                           torch.full_like(slot_dstl, n_own))
    chunk_rel = (gvals[grp_of_chunk] % r1).to(torch.int32)
    chunk_tile = (gvals[grp_of_chunk] // r1).to(torch.int32)
    n_tiles = (n_own + tile - 1) // tile
    per_tile = torch.bincount(chunk_tile.to(torch.int64), minlength=n_tiles)
    tile_ptr = torch.zeros(n_tiles + 1, dtype=torch.int32, device=dev)
    tile_ptr[1:] = torch.cumsum(per_tile, 0).to(torch.int32)
    # the dW kernels walk 64-row units, relation-major: units of a chunk that hold no row tile are left out
    upc = CHUNK // UNIT
    order_key = chunk_rel.to(torch.int64) * max(n_tiles, 1) + chunk_tile.to(torch.int64)
    chunk_order = torch.sort(order_key, stable=True)[1]
    units = (chunk_order[:, None] * upc + torch.arange(upc, device=dev)[None, :]).reshape(-1)
    used = (chunk_cnt.to(torch.int64)[chunk_order][:, None] > UNIT * torch.arange(upc, device=dev)[None, :]).reshape(-1)
    # a dW launch hands every wave one CONTIGUOUS range of this (relation, tile) order: few relation changes = few accumulator
    # flushes.  (Interleaves that deal a relation's units over the concurrent waves, so that the caches might serve the gathered
    # upstream-gradient rows, were tried in round 2: no gain)
    rel_order = units[used].to(torch.int32)
    return TilePlan(n_nodes=n_nodes, node_begin=node_begin, node_end=node_end,
                    num_relations=num_relations, tile=tile, chunk=CHUNK, n_tiles=n_tiles, n_chunks=n_chunks,
                    n_edges=n_edges, tile_ptr=tile_ptr, chunk_rel=chunk_rel, chunk_cnt=chunk_cnt,
                    chunk_tile=chunk_tile, rel_order=rel_order, slot_src=slot_src, slot_w=slot_w,
                    slot_dstl=slot_dstl, slot_row=slot_row, slot_acc=slot_acc, chunk_flags=chunk_flags,
                    layout=1 if split else 0, chunk_rows=per * g16)


def compact_runs(plan: TilePlan) -> TilePlan:
    """Twin of ``compact_runs_kernel`` (csrc/rgcn_plan.hip): a layout-0 plan with 128-slot chunks -> layout 3.  The rows of a
    (destination, relation) run all go through the same W_r into the same output row, so the producers of ``rgcn_tile3p_kernel``
    may add them in fp32 before they cut them (aggregate, then transform -- the reference's own order) and the run takes ONE slot.
    Chunk-local, and only where it is simple: chunks that are a whole (tile, relation) group, runs of at most 3 rows, at most 32
    runs of 2+ rows and 16 of 3; any other chunk keeps its layout-0 slots.  New chunk: heads (first row of every run; runs of 3
    first, then of 2, then single rows, each class in destination order) on slots 0 .. H-1; the second row of head h on row tile
    7 - h // 16, place h % 16; the third on row tile 7 - ns1 (right below the tiles of second rows), place h.  ``chunk_cnt`` = 16 ceil(H / 16); ``chunk_flags`` bits 20-23 = the chunk's
    row tiles (every chunk, compacted or not), bits 16-17 = row tiles with second rows, bit 18 = a row tile with third rows, bit 19 = some run's rows differ in weight (the producers then
    scale a shadow row by its weight / its head's weight -- the float32 in the shadow's ``slot_acc`` -- before they add it).  Every
    slot keeps its own weight and its run's row (a walk over all slots with a weight still sums the layer: tests/plan_emulator.py).
    Plain loops over the chunks: small plans (tests) only."""
    if plan.chunk != 128 or plan.layout != 0:
        raise ValueError("compact_runs wants a layout-0 plan with 128-slot chunks")
    if plan.n_chunks == 0:
        plan.layout = 3
        return plan
    dev = plan.slot_src.device
    tile, n_nodes, n_own = plan.tile, plan.n_nodes, plan.n_owned
    src = plan.slot_src.cpu().numpy().copy()
    wbits = plan.slot_w.cpu().numpy().copy().view("uint32")
    row = plan.slot_row.cpu().numpy().copy()
    acc = plan.slot_acc.cpu().numpy().copy()
    cnt = plan.chunk_cnt.cpu().numpy().copy()
    flags = plan.chunk_flags.cpu().numpy().copy()
    crel = plan.chunk_rel.cpu().numpy()
    ctile = plan.chunk_tile.cpu().numpy()
    dstl = None if plan.slot_dstl is None else plan.slot_dstl.cpu().numpy().copy()
    pad_acc = (15 << 24) | tile

    def ratio(ws_bits, wh_bits):          # float32 bits of (shadow weight / head weight), IEEE division as on the device
        import numpy as np
        q = np.array([ws_bits], dtype=np.uint32).view(np.float32) / np.array([wh_bits], dtype=np.uint32).view(np.float32)
        return int(q.astype(np.float32).view(np.int32)[0])

    for c in range(plan.n_chunks):
        nt = int(cnt[c]) // 16
        flags[c] |= nt << 20           # every chunk: its row tiles beside its flags (one scalar word for the producers)
        if c > 0 and crel[c - 1] == crel[c] and ctile[c - 1] == ctile[c]:
            continue
        if c + 1 < plan.n_chunks and crel[c + 1] == crel[c] and ctile[c + 1] == ctile[c]:
            continue
        if nt == 0:
            continue
        base = c * 128
        tbase = int(ctile[c]) * tile
        rows = []
        for j in range(nt * 16):
            sl = base + (j % nt) * 16 + j // nt
            if int(src[sl]) == n_nodes:
                break
            rows.append((int(src[sl]), int(row[sl]) - tbase, int(wbits[sl])))
        runs, j, ok, uneq = [], 0, True, 0
        while j < len(rows):
            ln = 1
            while j + ln < len(rows) and rows[j + ln][1] == rows[j][1]:
                if rows[j + ln][2] != rows[j][2]:
                    uneq = 1
                ln += 1
            if ln > 3:
                ok = False
            runs.append((j, ln))
            j += ln
        if not ok:
            continue
        n1 = sum(1 for _, ln in runs if ln == 1)
        n2 = sum(1 for _, ln in runs if ln == 2)
        n3 = sum(1 for _, ln in runs if ln == 3)
        if n2 + n3 == 0 or n3 > 16 or n2 + n3 > 32:
            continue
        heads = n1 + n2 + n3
        nh, ns1, ns2 = (heads + 15) // 16, (n2 + n3 + 15) // 16, 1 if n3 else 0
        if nh >= nt or nh + ns1 + ns2 > 8:
            continue
        src[base:base + 128] = n_nodes
        wbits[base:base + 128] = 0
        row[base:base + 128] = n_own
        acc[base:base + 128] = pad_acc
        if dstl is not None:
            dstl[base:base + 128] = tile
        nxt = {3: 0, 2: n3, 1: n3 + n2}
        for j0, ln in runs:
            h = nxt[ln]
            nxt[ln] += 1
            s0, d0, w0 = rows[j0]
            src[base + h], wbits[base + h], row[base + h] = s0, w0, tbase + d0
            acc[base + h] = ((h & 15) << 24) | d0
            if dstl is not None:
                dstl[base + h] = d0
            if ln >= 2:
                s1 = base + (7 - h // 16) * 16 + (h & 15)
                src[s1], wbits[s1], row[s1] = rows[j0 + 1][0], rows[j0 + 1][2], tbase + d0
                acc[s1] = ratio(rows[j0 + 1][2], w0)
            if ln == 3:
                s2 = base + (7 - ns1) * 16 + h
                src[s2], wbits[s2], row[s2] = rows[j0 + 2][0], rows[j0 + 2][2], tbase + d0
                acc[s2] = ratio(rows[j0 + 2][2], w0)
        cnt[c] = nh * 16
        flags[c] = (ns1 << 16) | (ns2 << 18) | (uneq << 19) | (nh << 20)
    plan.slot_src = torch.from_numpy(src).to(dev)
    plan.slot_w = torch.from_numpy(wbits.view("float32")).to(dev)
    plan.slot_row = torch.from_numpy(row).to(dev)
    plan.slot_acc = torch.from_numpy(acc).to(dev)
    plan.chunk_cnt = torch.from_numpy(cnt).to(dev)
    plan.chunk_flags = torch.from_numpy(flags).to(dev)
    if dstl is not None:
        plan.slot_dstl = torch.from_numpy(dstl).to(dev)
    plan.layout = 3
    return plan


def dw_pairs(plan: TilePlan) -> TilePlan:
    """Twin of ``dw_pairs_kernel`` (csrc/rgcn_plan.hip): a layout-0 plan with 64-slot chunks -> layout 5, the plan the tile-major
    weight-gradient kernel walks.  d_W_r is a sum over slots of (w x[src])^T g[row]: two rows with ONE (row, weight) -- a pair --
    take ONE slot if x[src] + x[src2] is formed first.  Group-local: (tile, relation) groups of at most two chunks; runs of equal
    (row, weight) are cut into pairs; heads = pairs + single rows are dealt back densely, 64 per unit; the head of a pair needs one
    of the unit's pair places (slots 0..3, and 32..35 once the unit holds more than 32 heads); pairs beyond the group's places stay
    two single rows.  ``slot_src2[unit * 8 + k]``: the second row of pair place k.  Chunks the group no longer needs get
    ``chunk_cnt`` 0 and leave ``rel_order``.  Plain loops over the groups: small plans (tests) only."""
    if plan.chunk != 64 or plan.layout != 0:
        raise ValueError("dw_pairs wants a layout-0 plan with 64-slot chunks")
    dev = plan.slot_src.device
    n_nodes, n_own = plan.n_nodes, plan.n_owned
    src = plan.slot_src.cpu().numpy().copy()
    wbits = plan.slot_w.cpu().numpy().copy().view("uint32")
    row = plan.slot_row.cpu().numpy().copy()
    cnt = plan.chunk_cnt.cpu().numpy().copy()
    crel = plan.chunk_rel.cpu().numpy()
    ctile = plan.chunk_tile.cpu().numpy()
    nc = plan.n_chunks
    src2 = np.full(max(nc * 8, 1), n_nodes, dtype=np.int32)
    c = 0
    while c < nc:
        m = 1
        while c + m < nc and crel[c + m] == crel[c] and ctile[c + m] == ctile[c]:
            m += 1
        c0, c = c, c + m
        if m > 2:
            continue
        nt = sum(int(cnt[c0 + i]) // 16 for i in range(m))
        if nt == 0:
            continue
        base = c0 * 64
        rows = []
        for j in range(nt * 16):
            tt = j % nt
            sl = base + (tt // 4) * 64 + (tt % 4) * 16 + j // nt
            if int(src[sl]) == n_nodes:
                break
            rows.append((int(src[sl]), int(row[sl]), int(wbits[sl])))
        n = len(rows)
        runs, j = [], 0
        while j < n:
            ln = 1
            while j + ln < n and rows[j + ln][1:] == rows[j][1:]:
                ln += 1
            runs.append((j, ln))
            j += ln
        pairs = sum(ln // 2 for _, ln in runs)
        if pairs == 0:
            continue
        heads = n - pairs

        def unit_heads(u):
            return min(64, heads - 64 * u)

        def places(u):
            nu = unit_heads(u)
            return min(4, nu) + (min(4, nu - 32) if nu > 32 else 0)

        while pairs > sum(places(u) for u in range((heads + 63) // 64)):
            pairs -= 1
            heads += 1
        units = (heads + 63) // 64
        pairs_in, left = [0, 0], pairs
        for u in range(units):
            pairs_in[u] = min(left, places(u))
            left -= pairs_in[u]
        src[base:base + m * 64] = n_nodes
        wbits[base:base + m * 64] = 0
        row[base:base + m * 64] = n_own

        def is_pair_place(u, sl):
            if sl < 4:
                return sl < pairs_in[u]
            if 32 <= sl < 36:
                return sl - 28 < pairs_in[u]
            return False

        pair_left, next_pair, next_single, single_u = pairs, [0, 0], [0, 0], 0
        for j0, ln in runs:
            k = 0
            while k < ln:
                as_pair = k + 1 < ln and pair_left > 0
                if as_pair:
                    u = 0 if next_pair[0] < pairs_in[0] else 1
                    kk = next_pair[u]
                    next_pair[u] += 1
                    sl = kk if kk < 4 else 28 + kk
                    pair_left -= 1
                else:
                    u = single_u
                    while True:
                        while next_single[u] < unit_heads(u) and is_pair_place(u, next_single[u]):
                            next_single[u] += 1
                        if next_single[u] < unit_heads(u):
                            break
                        u += 1
                        single_u = u
                    sl = next_single[u]
                    next_single[u] += 1
                g = base + u * 64 + sl
                src[g], row[g], wbits[g] = rows[j0 + k]
                if as_pair:
                    src2[(c0 + u) * 8 + (sl if sl < 4 else sl - 28)] = rows[j0 + k + 1][0]
                    k += 2
                else:
                    k += 1
        for i in range(m):
            cnt[c0 + i] = (unit_heads(i) + 15) // 16 * 16 if i < units else 0
    plan.slot_src = torch.from_numpy(src).to(dev)
    plan.slot_w = torch.from_numpy(wbits.view("float32")).to(dev)
    plan.slot_row = torch.from_numpy(row).to(dev)
    plan.chunk_cnt = torch.from_numpy(cnt).to(dev)
    plan.slot_src2 = torch.from_numpy(src2).to(dev)
    if plan.slot_dstl is not None:
        plan.slot_dstl = None          # (host-side checks of the forward plans only)
    # the unit list: non-empty 64-slot units, relation-major then tile -- as build_plan emits it, over the new counts
    order_key = plan.chunk_rel.to(torch.int64) * max(plan.n_tiles, 1) + plan.chunk_tile.to(torch.int64)
    chunk_order = torch.sort(order_key, stable=True)[1]
    used = plan.chunk_cnt.to(torch.int64)[chunk_order] > 0
    plan.rel_order = chunk_order[used].to(torch.int32)
    plan.layout = 5
    return plan


DW_WALKERS = 64             # tile ranges of the tile-major weight-gradient kernel (rgcn_dw_tiles_geometry reports the same number)
DW_FLAG_H0_STRADDLES = 1 << 28      # chunk_flags of a packed unit: half 0 holds rows of chunk_tile AND of chunk_tile + 1
DW_FLAG_H1_STRADDLES = 1 << 29      # ... half 1 does
DW_FLAG_H1_NEXT = 1 << 30           # half 1 holds rows of chunk_tile + 1 only, half 0 rows of chunk_tile only


def dw_pack(plan: TilePlan, walkers: int = DW_WALKERS) -> TilePlan:
    """Twin of ``dw_pack_kernel`` (csrc/rgcn_plan.hip), the pass after ``dw_pairs``: the heads of a STREAM -- the units of one relation
    in the tiles of one walker range ``[p * n_tiles // walkers, (p + 1) * n_tiles // walkers)``, the stretch of ``rel_order`` one wave
    of the kernel walks -- are packed densely in tile order, 32 per half, 64 per unit, into the storage of the stream's first
    units.  A unit holds rows of at most two consecutive tiles, ``chunk_tile`` (its earliest row's) and the next; a head that would
    break that closes the unit with padding.  A half takes a consecutive stretch of the stream, its pair heads (at most four, on the
    half's first slots) first; a pair that meets four pairs in its half becomes two single rows.  ``chunk_flags`` of a packed unit =
    which of its halves straddle (DW_FLAG_*).  Units the stream no longer needs get ``chunk_cnt`` 0 and leave ``rel_order``.
    Streams of one tile (every plan of fewer tiles than walkers) or of one unit stay as ``dw_pairs`` left them.
    In place: output unit j is written when input unit i >= j has been read -- a pair only splits where a short half left room."""
    if plan.chunk != 64 or plan.layout != 5:
        raise ValueError("dw_pack wants a layout-5 plan")
    dev = plan.slot_src.device
    n_nodes, n_own, n_tiles = plan.n_nodes, plan.n_owned, plan.n_tiles
    src = plan.slot_src.cpu().numpy().copy()
    wbits = plan.slot_w.cpu().numpy().copy().view("uint32")
    row = plan.slot_row.cpu().numpy().copy()
    src2 = plan.slot_src2.cpu().numpy().copy()
    cnt = plan.chunk_cnt.cpu().numpy().copy()
    ctile = plan.chunk_tile.cpu().numpy().copy()
    flags = plan.chunk_flags.cpu().numpy().copy()
    crel = plan.chunk_rel.cpu().numpy()
    order = plan.rel_order.cpu().numpy().astype(np.int64)
    key = crel.astype(np.int64)[order] * max(n_tiles, 1) + ctile.astype(np.int64)[order]

    def pack_stream(units):
        # state of the output: unit j, half hh with its pairs / singles so far, the tiles its halves hold
        st = {"j": 0, "open": False, "ut": 0, "hh": 0, "n": [0, 0], "t1": [[False, False], [False, False]]}
        pairs, singles = [], []
        o_src, o_row, o_w, o_s2 = [None], [None], [None], [None]

        def open_unit(th):
            st.update(open=True, ut=th, hh=0, n=[0, 0], t1=[[False, False], [False, False]])
            o_src[0] = np.full(64, n_nodes, np.int32)
            o_row[0] = np.full(64, n_own, np.int32)
            o_w[0] = np.zeros(64, np.uint32)
            o_s2[0] = np.full(8, n_nodes, np.int32)

        def close_half():
            hh, b = st["hh"], 32 * st["hh"]
            for q, (s_, r_, w_, s2_) in enumerate(pairs):
                o_src[0][b + q], o_row[0][b + q], o_w[0][b + q], o_s2[0][4 * hh + q] = s_, r_, w_, s2_
            for q, (s_, r_, w_) in enumerate(singles):
                o_src[0][b + len(pairs) + q], o_row[0][b + len(pairs) + q], o_w[0][b + len(pairs) + q] = s_, r_, w_
            st["n"][hh] = len(pairs) + len(singles)
            pairs.clear()
            singles.clear()
            st["hh"] = hh + 1
            if hh == 1:
                close_unit()

        def close_unit():
            if pairs or singles:
                close_half()
                if not st["open"]:
                    return
            u = units[st["j"]]
            assert st["j"] <= st["i"], "dw_pack: output overtook input"
            n0, n1 = st["n"]
            src[64 * u:64 * u + 64], row[64 * u:64 * u + 64], wbits[64 * u:64 * u + 64] = o_src[0], o_row[0], o_w[0]
            src2[8 * u:8 * u + 8] = o_s2[0]
            cnt[u] = ((32 + n1 if n1 else n0) + 15) // 16 * 16
            ctile[u] = st["ut"]
            (a0, b0), (a1, b1) = st["t1"]
            flags[u] = ((DW_FLAG_H0_STRADDLES if a0 and b0 else 0) | (DW_FLAG_H1_STRADDLES if a1 and b1 else 0)
                        | (DW_FLAG_H1_NEXT if b1 and not a1 and not b0 else 0))
            st["j"] += 1
            st["open"] = False

        def put(s_, r_, w_, s2_, th):
            if st["open"] and th > st["ut"] + 1:
                close_unit()
            if not st["open"]:
                open_unit(th)
            if s2_ is not None and len(pairs) == 4:      # no pair place left in this half: two single rows
                put(s_, r_, w_, None, th)
                put(s2_, r_, w_, None, th)
                return
            st["t1"][st["hh"]][th - st["ut"]] = True
            if s2_ is not None:
                pairs.append((s_, r_, w_, s2_))
            else:
                singles.append((s_, r_, w_))
            if len(pairs) + len(singles) == 32:
                close_half()

        for i, u in enumerate(units):
            st["i"] = i
            i_src, i_row, i_w = src[64 * u:64 * u + 64].copy(), row[64 * u:64 * u + 64].copy(), wbits[64 * u:64 * u + 64].copy()
            i_s2, ti = src2[8 * u:8 * u + 8].copy(), int(ctile[u])
            for s in range(64):
                if i_src[s] == n_nodes:
                    continue
                k = s if s < 4 else (s - 28 if 32 <= s < 36 else -1)
                put(i_src[s], i_row[s], i_w[s], int(i_s2[k]) if k >= 0 and i_s2[k] != n_nodes else None, ti)
        st["i"] = len(units)
        if st["open"]:
            close_unit()
        for jj in range(st["j"], len(units)):
            u = units[jj]
            src[64 * u:64 * u + 64], row[64 * u:64 * u + 64], wbits[64 * u:64 * u + 64] = n_nodes, n_own, 0
            src2[8 * u:8 * u + 8] = n_nodes
            cnt[u], flags[u] = 0, 0

    for r in range(plan.num_relations):
        for p in range(walkers):
            t0, t1 = p * n_tiles // walkers, (p + 1) * n_tiles // walkers
            if t1 - t0 < 2:
                continue
            i0, i1 = np.searchsorted(key, [r * n_tiles + t0, r * n_tiles + t1])
            if i1 - i0 >= 2:
                pack_stream(order[i0:i1])
    plan.slot_src = torch.from_numpy(src).to(dev)
    plan.slot_w = torch.from_numpy(wbits.view("float32")).to(dev)
    plan.slot_row = torch.from_numpy(row).to(dev)
    plan.slot_src2 = torch.from_numpy(src2).to(dev)
    plan.chunk_cnt = torch.from_numpy(cnt).to(dev)
    plan.chunk_tile = torch.from_numpy(ctile).to(dev)
    plan.chunk_flags = torch.from_numpy(flags).to(dev)
    chunk_order = torch.sort(plan.chunk_rel.to(torch.int64), stable=True)[1]      # stable: a relation's units in tile order
    used = plan.chunk_cnt.to(torch.int64)[chunk_order] > 0
    plan.rel_order = chunk_order[used].to(torch.int32)
    return plan


def team_placement(dstl: Tensor, gcnt: Tensor, grp_of_edge: Tensor, rank: Tensor, chunk_base: Tensor,
                   grp_of_chunk: Tensor, idx_in_grp: Tensor):
    """Layout 1 (128-slot chunks): chunk c of a group takes the group's sorted rows [128 c, 128 c + 128) -- n_c of them, on
    nt = ceil(n_c / 16) row tiles.  The rows are cut at a RUN BOUNDARY s (the destination changes between rows s - 1 and s)
    into part A = rows [0, s) on the chunk's first nA = ceil(nt / 2) row tiles and part B = rows [s, n_c) on the other
    nB = nt - nA (row j of a part -> the part's tile j mod n_part, place j div n_part).  So the two parts of a chunk hold
    DISJOINT destination sets, and two teams of consumer waves of the forward / dX kernel (csrc/rgcn_tile3p.hip) accumulate
    them at the same time without ever touching the same accumulator row.  s lies in [max(1, n_c - 16 nB), min(n_c - 1,
    16 nA)] -- both parts fit their tiles and need all of them, so a chunk takes exactly the nt row tiles of layout 0 --
    and is the boundary closest to the middle of that window (the lower one on a tie); a chunk without one (a single
    destination's run covers the window) is cut at the middle and flagged (chunk_flags bit 8: the parts share a destination,
    one team takes the whole chunk).  nt = 1: everything in part A.
    Returns (slot of every row, chunk_cnt, straddle flag per chunk)."""
    C, g16 = 128, ROWS_PER_MFMA_TILE
    dev = dstl.device
    n_chunks = int(grp_of_chunk.shape[0])
    n_c = torch.clamp(gcnt[grp_of_chunk] - idx_in_grp * C, max=C)
    nt = (n_c + (g16 - 1)) // g16
    n_a = (nt + 1) // 2
    n_b = nt - n_a
    two = nt > 1
    lo_c = torch.clamp(n_c - g16 * n_b, min=1)
    hi_c = torch.minimum(n_c - 1, g16 * n_a)
    mid_c = (lo_c + hi_c + 1) // 2
    cidx = rank // C
    jc = rank - cidx * C
    chunk_of_row = chunk_base[grp_of_edge] + cidx
    prev_dstl = torch.cat([dstl[:1], dstl[:-1]])
    boundary = (jc >= 1) & (dstl != prev_dstl)             # jc >= 1: row jc - 1 belongs to the same chunk range
    cand = boundary & two[chunk_of_row] & (jc >= lo_c[chunk_of_row]) & (jc <= hi_c[chunk_of_row])
    dist = jc - mid_c[chunk_of_row]
    score = 2 * dist.abs() + (dist > 0).to(torch.int64)    # mid, mid - 1, mid + 1, mid - 2, ...
    big_score = 1 << 20
    best = torch.full((n_chunks,), big_score, dtype=torch.int64, device=dev)
    best = best.scatter_reduce(0, chunk_of_row[cand], score[cand], reduce="amin", include_self=True)
    has = best < big_score
    k = best // 2
    s_found = torch.where(best % 2 == 1, mid_c + k, mid_c - k)
    s_c = torch.where(two, torch.where(has, s_found, mid_c), n_c)
    straddle = two & ~has
    chunk_cnt = (nt * g16).to(torch.int32)
    s_r = s_c[chunk_of_row]
    na_r, nb_r = n_a[chunk_of_row], torch.clamp(n_b[chunk_of_row], min=1)
    j1 = torch.clamp(jc - s_r, min=0)
    in_chunk = torch.where(jc < s_r, (jc % na_r) * g16 + jc // na_r, (na_r + j1 % nb_r) * g16 + j1 // nb_r)
    return chunk_of_row * C + in_chunk, chunk_cnt, straddle


ROWS_PER_MFMA_TILE = 16
LDS_BYTES = 160 * 1024
ACC_PAD = 4    # floats of padding per accumulator row in the tile kernel's LDS tile (bank spread)


def padded_width(w: int) -> int:
    """the kernels pad feature widths to 16 / 32 / 64 / 128 (csrc/rgcn_common.h padded_width)"""
    return 16 if w <= 16 else 32 if w <= 32 else 64 if w <= 64 else 128


# measured ms per launch at the headline config over the model's cycle count, per kernel: what makes the two kernels' costs comparable
# (exact fp32: 10.15 ms where the model says 8.6; bf16 x 3: 8.4 ms where its model -- 1,800 cycles per chunk, 420 per row tile,
# DESIGN.md 8.0f -- says 9.2)
_KERNEL_MODEL = {"fp32": (800.0, 650.0, 1.18), "bf16x3": (1800.0, 420.0, 0.91)}
DW_PLAN_LAYOUT = 5      # pairs on one slot (round 4); layout 0 (one slot per row) stays reachable through _device_plan
P3_MAX_TILE = 224          # rgcn_tile3p_kernel: two 48 KiB ring slots (any 128-slot chunk) + the fp32 accumulator in 160 KiB
P3_MAX_TILE_112 = 272      # ... two 42 KiB slots (chunks of at most 112 rows: CHUNK_112)


def choose_layout(n_nodes: int, n_edges: int, num_relations: int, in_channels: int, out_channels: int, kernel: str = "fp32",
                  with_cost: bool = False):
    """cached front of ``_choose_layout`` (a layer asks on every forward call; the model is a few hundred erfc evaluations)"""
    return _choose_layout(int(n_nodes), int(n_edges), int(num_relations), int(in_channels), int(out_channels), kernel, bool(with_cost))


@functools.lru_cache(maxsize=256)
def _choose_layout(n_nodes: int, n_edges: int, num_relations: int, in_channels: int, out_channels: int, kernel: str = "fp32",
                   with_cost: bool = False):
    """(tile, chunk) for a layer: output nodes per tile and edge slots per chunk.  ``kernel="bf16x3"``: the layout for
    rgcn_tile3p_kernel (64 x 64 layers: 128-slot chunks, tiles up to 224, its own per-chunk / per-row-tile cycles);
    ``with_cost``: also the modelled time of one launch, comparable between the two kernels (conv.RGCNConv._route picks with it).

    Cost model of the forward / dX kernel, calibrated on the 10M-node / 100M-edge graph (a cycle-stamp build): a
    chunk costs ~800 cycles whatever it holds (barrier, metadata, pipeline fill and drain) and every 16-row MFMA tile
    ~650 (512 of them MFMA issue).  A (tile, relation) group of g = tile * E / (N R') edges (roughly normal, sd
    sqrt(g)) takes E[ceil(g / chunk)] chunks and ~g / 16 + 1/2 row tiles, so larger tiles and 128-slot chunks
    amortise the fixed part -- within the LDS: (tile + 1) * (pad(width) + 4) * 4 B of accumulator plus at least two
    ring slots of chunk * (pad(other width) + 2) * 4 B (three cost nothing extra; with two the producers run only one
    chunk ahead: +3 %).  128-slot chunks are built for widths <= 64.  The launch runs in rounds of 256 workgroups that
    walk up to 16 tiles each, so what is minimised is rounds x cycles per tile."""
    import math
    kp, np_ = padded_width(in_channels), padded_width(out_channels)
    density = n_edges / max(1.0, float(n_nodes) * max(1, num_relations))

    def lds(t, chunk, ring):
        fwd = (t + 1) * (np_ + ACC_PAD) * 4 + ring * chunk * (kp + 2) * 4
        bwd = (t + 1) * (kp + ACC_PAD) * 4 + ring * chunk * (np_ + 2) * 4
        return max(fwd, bwd)

    def expect_ceil(g, unit):
        if g <= 0:
            return 0.0
        sd = math.sqrt(g)
        return sum(0.5 * math.erfc((unit * k - g) / (sd * math.sqrt(2.0))) for k in range(0, int(g / unit) + 6))

    c_chunk, c_tile, scale = _KERNEL_MODEL[kernel]
    p3 = kernel == "bf16x3"

    def cost(t, chunk):
        g = density * t
        ring_penalty = 1.0 if (p3 or lds(t, chunk, 3) <= LDS_BYTES) else 1.03
        per_rel = expect_ceil(g, chunk) * c_chunk + (g / 16.0 + 0.5) * c_tile if g > 0 else 0.0
        root = math.ceil(t / chunk) * c_chunk + (t / 16.0) * c_tile
        return scale * ring_penalty * (max(1, num_relations) * per_rel + root) / t      # cycles per output node

    def launch_rounds(n_tiles):
        # tile times one launch takes: a workgroup (one per CU, 256 CUs) walks up to 16 tiles, start-up ~4 % of a tile;
        # the library picks the count the same way (csrc/rgcn_kernels_shared.h tiles_per_workgroup)
        return min(math.ceil(math.ceil(n_tiles / k) / 256) * (k + 0.04) for k in range(1, 17))

    if p3:      # 128-slot chunks up to tile 224, 112-row chunks (seven row tiles; the kernel's smaller ring slots) up to 272
        cands = ([(t, 128) for t in range(64, P3_MAX_TILE + 1, 16)] + [(t, CHUNK_112) for t in range(P3_MAX_TILE + 16, P3_MAX_TILE_112 + 1, 16)]
                 if max(kp, np_) == 64 and min(kp, np_) == 64 else [])
    else:
        cands = [(t, c) for c in CHUNKS for t in range(64, 513, 16)
                 if lds(t, c, 2) <= LDS_BYTES and (c == CHUNK or max(kp, np_) <= 64)]
    if not cands:
        return (64, CHUNK, float("inf")) if with_cost else (64, CHUNK)
    # time of a launch ~ rounds x (cycles per tile): on large graphs this is the cost per node, on small ones the round
    # count decides (100k nodes: 285 tiles of 352 are two rounds with the second one a ninth full)
    key = lambda tc: (round(launch_rounds(math.ceil(n_nodes / tc[0])) * cost(*tc) * tc[0] / 1e3, 1), -tc[0])
    best = min(cands, key=key)
    return (best[0], best[1], key(best)[0]) if with_cost else best


def run_metadata(slot_dstl: Tensor, tile: int):
    """Per slot, for the forward kernel's run-sum (csrc/rgcn_tile_fp32_kernel.h / rgcn_tile3p.hip: the Y-orientation run-sum product), precomputed here so
    the kernel spends no vector instructions on it: inside every 16-slot MFMA row tile, slots with equal
    destination are adjacent (tiles are sorted by destination) and form a RUN; the run's sum is written by
    its LAST slot only.  Returns (slot_acc, tile_dup).  slot_acc = (position 0..15 inside the row tile of the
    slot that ends this slot's run) << 24 | (accumulator row the slot writes).  The accumulator row is the
    slot's destination if it ends a run, else the dummy row ``tile`` (padding slots carry destination ``tile``
    already); it sits in the low 24 bits so that the kernel forms the LDS address with one 24-bit
    multiply-add, which ignores the top byte by itself.
    tile_dup[t]: row tile t contains a run longer than one slot (needs the run-sum product)."""
    g = ROWS_PER_MFMA_TILE
    d = slot_dstl.view(-1, g).to(torch.int64)
    nxt = torch.cat([d[:, 1:], torch.full_like(d[:, :1], -1)], dim=1)
    is_end = d != nxt                                    # last column always ends (next = -1)
    pos = torch.arange(g, device=d.device).expand_as(d)
    endpos = torch.where(is_end, pos, torch.full_like(pos, g))
    runend = torch.flip(torch.cummin(torch.flip(endpos, [1]), dim=1).values, [1])
    acc = torch.where(is_end, d, torch.full_like(d, tile))
    tile_dup = ((~is_end) & (d != tile)).any(dim=1)     # runs of padding slots do not count
    return ((runend << 24) | acc).to(torch.int32).reshape(-1), tile_dup


@dataclass
class GraphPlans:
    """Forward plan (edges grouped by destination) + transposed plan (grouped by source).  A direction that runs the
    edge-parallel path (eplan.choose_path) has an eplan.EdgePlan instead of a tile-major plan."""
    fwd: Optional[TilePlan]
    bwd: Optional[TilePlan]
    num_edges: int
    dw: Optional[TilePlan] = None        # forward-direction plan in the geometry of the tile-major dW kernel (dw_walk_table)
    dw_walk: Optional[Tensor] = None     # int32 [R'][walkers + 1]
    ep_fwd: Optional[object] = None      # eplan.EdgePlan: forward on rgcn_ep_*, weight gradients on its dense units
    ep_bwd: Optional[object] = None      # eplan.EdgePlan of the transposed graph: dX on rgcn_ep_*

    @property
    def fwd_walk(self) -> TilePlan:
        """the plan whose 64-slot units the relation-major weight-gradient kernels walk"""
        return self.fwd if self.fwd is not None else self.ep_fwd.as_tile_plan()

    def nbytes(self) -> int:
        return sum(q.nbytes() for q in (self.fwd, self.bwd, self.dw, self.ep_fwd, self.ep_bwd) if q is not None)


def build_graph_plans_torch(edge_index: Tensor, edge_type: Tensor, n_nodes: int, num_relations: int,
                            tile: int, aggr: str = "mean",
                            fwd_range: Optional[Tuple[int, int]] = None,
                            bwd_range: Optional[Tuple[int, int]] = None, chunk: int = CHUNK,
                            split: bool = False, paths: Tuple[str, str] = ("ring", "ring")) -> GraphPlans:
    """The plans as torch tensor ops (any device): the TEST ORACLE of the device-side builder and what the CPU-only
    tests walk with tests/plan_emulator.py.  paths: 'ring' (tile-major plan) or 'ep' (eplan.EdgePlan) per direction."""
    fb, fe = fwd_range if fwd_range is not None else (0, n_nodes)
    bb, be = bwd_range if bwd_range is not None else (0, n_nodes)
    check_ep_ranges(paths, [((fb, fe), (bb, be))])
    src, dst = edge_index[0], edge_index[1]
    w = edge_weights(src, dst, edge_type, num_relations, aggr)
    gp = GraphPlans(fwd=None, bwd=None, num_edges=int(edge_type.shape[0]))
    if paths[0] == "ep":
        gp.ep_fwd = build_edge_plan(src, dst, edge_type, w, n_nodes, num_relations, fb, fe, heavy=HEAVY)
    else:
        gp.fwd = build_plan(src, dst, edge_type, w, n_nodes, num_relations, tile, fb, fe, chunk, split)
    if paths[1] == "ep":
        gp.ep_bwd = build_edge_plan(dst, src, edge_type, w, n_nodes, num_relations, bb, be, heavy=HEAVY)
    else:
        gp.bwd = build_plan(dst, src, edge_type, w, n_nodes, num_relations, tile, bb, be, chunk, split)
    return gp


def empty_plan(n_nodes: int, node_begin: int, num_relations: int, tile: int, chunk: int, device, layout: int = 0) -> TilePlan:
    """the plan of an empty node range (dist.py: a block wholly past the last node, or squeezed out by a hub's block)"""
    z = lambda dt=torch.int32: torch.zeros(0, dtype=dt, device=device)
    rows = chunk
    chunk = 128 if chunk == CHUNK_112 else chunk
    return TilePlan(n_nodes=n_nodes, node_begin=node_begin, node_end=node_begin, num_relations=num_relations, tile=tile,
                    chunk_rows=rows, chunk=chunk, n_tiles=0, n_chunks=0, n_edges=0, tile_ptr=torch.zeros(1, dtype=torch.int32, device=device),
                    chunk_rel=z(), chunk_cnt=z(), chunk_tile=z(), chunk_flags=z(), rel_order=z(), slot_src=z(),
                    slot_w=z(torch.float32), slot_dstl=None, slot_row=z(), slot_acc=z(), layout=layout)


class PlanBuild:
    """The device build session of one graph: the C struct of its edge list (``_lib.graph_struct``), the tensors that struct points
    into, the edge weights (rgcn_edge_weights, one pass for both directions and every range) and the builder's workspace -- what
    every plan of the graph is laid out from (csrc/rgcn_plan.hip) and what lives exactly as long as the session does.
    ``max_owned``: the longest node range a plan will own; ``ws_tile``: the smallest tile of any plan (it sizes the group arrays)."""

    def __init__(self, edge_index: Tensor, edge_type: Tensor, n_nodes: int, num_relations: int, aggr: str, max_owned: int, ws_tile: int):
        self._graph(edge_index, edge_type, n_nodes, num_relations)
        self.ws = _lib.plan_workspace(self.num_edges, max_owned, num_relations, ws_tile, edge_type.device)
        try:
            self.w = _lib.edge_weights(self.graph, aggr, self.ws)
        except _lib.RgcnLibraryError as err:
            if "out of range" in str(err):
                raise ValueError("edge_index / edge_type out of range [0, num_nodes) / [0, num_relations)") from err
            raise

    def _graph(self, edge_index: Tensor, edge_type: Tensor, n_nodes: int, num_relations: int) -> None:
        self.edge_index, self.edge_type, self.n_nodes, self.num_relations = edge_index, edge_type, n_nodes, num_relations
        self.num_edges = int(edge_type.shape[0])
        self.graph, self._owned = _lib.graph_struct(edge_index, edge_type, n_nodes, num_relations)      # (_owned: what the struct points into)

    @classmethod
    def adopt(cls, graph, w: Tensor, ws: Tensor, n_nodes: int, num_relations: int, edge_index: Optional[Tensor] = None,
              edge_type: Optional[Tensor] = None) -> "PlanBuild":
        """a session over a struct, weights and workspace the caller made -- and keeps alive -- itself (eplan.build_edge_plan_device);
        without the COO tensors no heavy segment can be cut out"""
        pb = cls.__new__(cls)
        pb.edge_index, pb.edge_type, pb.n_nodes, pb.num_relations = edge_index, edge_type, n_nodes, num_relations
        pb.num_edges, pb.graph, pb._owned, pb.w, pb.ws = int(graph.num_edges), graph, (), w, ws
        return pb

    def without(self, edge_mask: Tensor) -> "PlanBuild":
        """the session of the same graph without the masked edges (the LIGHT graph once heavy segments are cut out): contiguous
        copies of its own, the kept edges' weights, the same workspace"""
        keep = ~edge_mask
        pb = PlanBuild.__new__(PlanBuild)
        pb._graph(self.edge_index[:, keep].contiguous(), self.edge_type[keep].contiguous(), self.n_nodes, self.num_relations)
        pb.w, pb.ws = self.w[keep].contiguous(), self.ws
        return pb

    def tile_plan(self, transposed: bool, tile: int, chunk: int, begin: int, end: int, layout: int = 0, aligned: bool = True) -> TilePlan:
        layout = int(layout)
        if end <= begin:           # nothing to lay out
            return empty_plan(self.n_nodes, begin, self.num_relations, tile, chunk, self.ws.device, layout)
        if aligned and begin % tile != 0:       # forward / dX plans of a rank: its tiles must be the single-rank tiles
            raise ValueError("node_begin must be a multiple of the tile size")
        ps, a, n_edges = _lib.plan_build(self.graph, self.w, transposed, begin, end, tile, chunk, self.ws, layout)
        if layout == 5:          # the pairs left fewer units than _begin sized rel_order for
            a["rel_order"] = a["rel_order"][:int(ps.n_units)]
        plan = TilePlan(n_nodes=self.n_nodes, node_begin=begin, node_end=end, num_relations=self.num_relations, tile=tile,
                        chunk=int(ps.chunk), n_tiles=int(ps.n_tiles), n_chunks=int(ps.n_chunks), n_edges=n_edges, slot_dstl=None,
                        layout=layout, chunk_rows=int(ps.chunk_rows), **a)
        plan._cstruct = ps
        return plan

    def dw_plan(self, begin: int, end: int):
        """(plan, walk table) of the tile-major weight-gradient kernel over the in-edges of [begin, end): its own layout of the
        same edges (layout 5: the two rows of a (destination, relation) pair on one slot -- dw_pairs / dw_pairs_kernel; the range
        need not be a multiple of THAT tile -- the sums of a partitioned d_weight differ in order from the single-rank ones
        anyway).  (None, None) for an empty range (its owner adds zeros); None past the relations the kernel holds."""
        t_dw, _, max_rel = _lib.dw_tiles_geometry()
        if self.num_relations > max_rel:
            return None
        if end <= begin:
            return None, None
        pl = self.tile_plan(False, t_dw, 64, begin, end, DW_PLAN_LAYOUT, aligned=False)
        return pl, _lib.dw_tiles_walk(_lib.plan_struct(pl), self.ws.device)

    def edge_plan(self, transposed: bool, begin: int, end: int, heavy: int, shared: Optional[SharedHeavy] = None, piece: int = PIECE) -> EdgePlan:
        """eplan.build_edge_plan by the library's own builder: rgcn_plan_build_begin / _finish with layout 2 lay the owned range out
        as one relation-major "tile", rgcn_eplan_segments sorts the slots by destination; only the sum levels of hubs (arithmetic
        on seg_ptr) and the split-off of the heavy segments stay here.  ``heavy`` > 0: this range's segments of at least that many
        rows become its HeavyPart and leave the units.  ``shared`` (hubs split across ranks): this is the ``without`` session of
        the whole graph's heavy segments, and the range gets the pseudo rows of its own."""
        n_own, light, hp = end - begin, self, None
        if shared is not None:
            hp = shared_heavy_part(shared, self.n_nodes, begin, end, self.num_relations)
        elif heavy > 0 and self.edge_index is not None and self.num_edges > 0:
            g_, s_ = (self.edge_index[1], self.edge_index[0]) if transposed else (self.edge_index[0], self.edge_index[1])
            own = (s_ >= begin) & (s_ < end)
            hm = heavy_mask(torch.where(own, s_, torch.full_like(s_, -1)), self.edge_type, self.n_nodes + 1, heavy)      # (-1: not owned, its own keys)
            hm = hm & own if hm is not None else None
            if hm is not None and bool(hm.any()):
                hp = build_heavy_part(g_[hm], s_[hm] - begin, self.edge_type[hm], self.w[hm], n_own, self.num_relations, piece)
                light = self.without(hm)
        ps, a, n_edges = _lib.plan_build(light.graph, light.w, transposed, begin, end, 16, UNIT, self.ws, 2)
        levels, n_all, max_rows = _finish_levels(a["slot_row"], hp, n_own, piece, True)
        ep = EdgePlan(n_nodes=self.n_nodes, node_begin=begin, node_end=end, num_relations=self.num_relations, n_units=int(ps.n_chunks),
                      n_rows=n_all - (hp.n_seg if hp is not None else 0), unit_rel=a["chunk_rel"], unit_cnt=a["chunk_cnt"],
                      slot_src=a["slot_src"], slot_w=a["slot_w"], slot_row=a["slot_row"], levels=levels, max_rows_per_dst=max_rows, heavy=hp)
        # the same arrays are the relation-major walk of the weight-gradient kernels: the struct the builder filled
        ep._tile_plan = TilePlan(n_nodes=self.n_nodes, node_begin=begin, node_end=end, num_relations=self.num_relations, tile=int(ps.tile),
                                 chunk=UNIT, n_tiles=int(ps.n_tiles), n_chunks=int(ps.n_chunks), n_edges=n_edges, slot_dstl=None, layout=2, **a)
        ep._tile_plan._cstruct = ps
        return ep


def range_plans(builds, fwd_range: Tuple[int, int], bwd_range: Tuple[int, int], tile: int, chunk: int, split, paths: Tuple[str, str],
                dw_tiles: bool = False, shared=(None, None)) -> GraphPlans:
    """The GraphPlans of one (forward range, dX range) pair.  ``builds``: the PlanBuild per direction -- one session twice, or
    (dist.py, hubs split across ranks) the ``without`` session of a direction whose heavy segments are ``shared[d]``."""
    if chunk not in CHUNKS and chunk != CHUNK_112:
        raise ValueError(f"chunk must be one of {CHUNKS} (or {CHUNK_112})")
    pb, (fb, fe), (bb, be) = builds[0], fwd_range, bwd_range
    if fe <= fb or be <= bb:       # an empty block of a rank (dist.py)
        return GraphPlans(fwd=empty_plan(pb.n_nodes, fb, pb.num_relations, tile, chunk, pb.ws.device, int(split)),
                          bwd=empty_plan(pb.n_nodes, bb, pb.num_relations, tile, chunk, pb.ws.device, int(split)), num_edges=0)
    gp = GraphPlans(fwd=None, bwd=None, num_edges=pb.num_edges)
    if paths[0] == "ep":       # edge-parallel direction: relation-major units + destination-major segments (eplan.py)
        gp.ep_fwd = builds[0].edge_plan(False, fb, fe, HEAVY, shared[0])
    else:
        gp.fwd = pb.tile_plan(False, tile, chunk, fb, fe, split)
    if paths[1] == "ep":
        gp.ep_bwd = builds[1].edge_plan(True, bb, be, HEAVY, shared[1])
    else:
        gp.bwd = builds[1].tile_plan(True, tile, chunk, bb, be, split)
    dw = pb.dw_plan(fb, fe) if dw_tiles and paths[0] != "ep" else None
    if dw is not None:
        gp.dw, gp.dw_walk = dw
    return gp


def build_graph_plans_device(edge_index: Tensor, edge_type: Tensor, n_nodes: int, num_relations: int, tile: int,
                             aggr: str = "mean", fwd_range: Optional[Tuple[int, int]] = None,
                             bwd_range: Optional[Tuple[int, int]] = None, chunk: int = CHUNK,
                             ranges=None, split: bool = False, dw_tiles: bool = False,
                             paths: Tuple[str, str] = ("ring", "ring")):
    """The plans built by the HIP library itself (csrc/rgcn_plan.hip through rgcn_edge_weights / rgcn_plan_build_*):
    what every GPU forward uses.  ``ranges``: a list of (forward range, dX range) pairs -> a list of GraphPlans laid out from one
    PlanBuild (one edge-weight pass, one workspace), each counting the edges of its own forward plan."""
    rs = ranges if ranges is not None else [(fwd_range or (0, n_nodes), bwd_range or (0, n_nodes))]
    check_ep_ranges(paths, rs)
    own_max = max([1] + [max(f[1] - f[0], b[1] - b[0]) for f, b in rs])
    ws_tile = min(tile, _lib.dw_tiles_geometry()[0]) if dw_tiles else tile
    pb = PlanBuild(edge_index, edge_type, n_nodes, num_relations, aggr, own_max, ws_tile)
    out = [range_plans((pb, pb), f, b, tile, chunk, split, paths, dw_tiles) for f, b in rs]
    if ranges is None:
        return out[0]
    for gp in out:
        if gp.fwd is not None:
            gp.num_edges = gp.fwd.n_edges
    return out


def dw_walk_table(plan: TilePlan, walkers: int) -> Tensor:
    """Torch form (test oracle) of rgcn_dw_tiles_walk -- walk_ptr of rgcn_bwd_dw_tiles: for relation r and walker p the first position in ``plan.rel_order`` (sorted by
    (relation, tile)) of a unit of relation r whose tile is >= p * n_tiles // walkers; column ``walkers`` = end of relation r."""
    dev = plan.rel_order.device
    units = plan.rel_order.long()
    upc = plan.chunk // UNIT
    key = plan.chunk_rel.long()[units // upc] * plan.n_tiles + plan.chunk_tile.long()[units // upc]
    r = torch.arange(plan.num_relations, device=dev)[:, None]
    t = (torch.arange(walkers + 1, device=dev) * plan.n_tiles // walkers)[None, :]
    return torch.searchsorted(key, (r * plan.n_tiles + t).reshape(-1)).view(plan.num_relations, walkers + 1).to(torch.int32).contiguous()


def build_graph_plans(edge_index: Tensor, edge_type: Tensor, n_nodes: int, num_relations: int,
                      tile: int, aggr: str = "mean",
                      fwd_range: Optional[Tuple[int, int]] = None,
                      bwd_range: Optional[Tuple[int, int]] = None, chunk: int = CHUNK,
                      split: bool = False, dw_tiles: bool = False, paths: Tuple[str, str] = ("ring", "ring")) -> GraphPlans:
    """Device tensors: the HIP plan builder behind the C ABI.  CPU tensors (tests without a GPU): the torch form."""
    if edge_type.device.type == "cuda":
        return build_graph_plans_device(edge_index, edge_type, n_nodes, num_relations, tile, aggr, fwd_range, bwd_range, chunk,
                                        split=split, dw_tiles=dw_tiles, paths=paths)
    return build_graph_plans_torch(edge_index, edge_type, n_nodes, num_relations, tile, aggr, fwd_range, bwd_range, chunk, split,
                                   paths=paths)


def balanced_ranges(counts_per_tile: Tensor, world: int, tile: int, n_nodes: int):
    """Cut the tile sequence into ``world`` contiguous node ranges of about equal edge count
    (SURVEY.md 8e "ranges balanced by edge count").  Boundaries are multiples of ``tile`` so a
    rank's tiles -- and therefore every accumulation order -- equal the single-rank ones."""
    n_tiles = counts_per_tile.shape[0]
    cum = torch.cumsum(counts_per_tile.to(torch.float64) + 1e-3, 0)  # +eps: spread empty tiles too
    total = float(cum[-1]) if n_tiles else 0.0
    bounds = [0]
    for p in range(1, world):
        t = int(torch.searchsorted(cum, torch.tensor(total * p / world, dtype=torch.float64,
                                                      device=cum.device)).item())
        t = min(max(t, bounds[-1]), n_tiles)
        bounds.append(t)
    bounds.append(n_tiles)
    return [(min(b * tile, n_nodes), min(e * tile, n_nodes)) for b, e in zip(bounds[:-1], bounds[1:])]


# ------------------------------------------------------------------------------------------
# plan cache, keyed on the identity of the tensors the caller passes every forward
# ------------------------------------------------------------------------------------------
_CACHE: Dict[tuple, tuple] = {}     # insertion-ordered: least recently used first
_CACHE_MAX = 16
_CACHE_MAX_BYTES = int(float(_os.environ.get("RGCN_PLAN_CACHE_GB", "48")) * (1 << 30))   # read once at import


def cached_graph_plans(edge_index: Tensor, edge_type: Tensor, n_nodes: int, num_relations: int,
                       tile: int, aggr: str, builder=None, extra_key=(), chunk: int = CHUNK, split: bool = False,
                       dw_tiles: bool = False, paths=("ring", "ring"), widths: Optional[Tuple[int, int]] = None) -> GraphPlans:
    """LRU over (edge tensors' identity, layout): at most ``_CACHE_MAX`` entries and ``RGCN_PLAN_CACHE_GB`` (48) GiB of
    plan arrays (4.3 GB per 100M edges), least recently used evicted first.  On a miss ``paths`` = "auto" is resolved
    (eplan.resolve_paths; the key keeps "auto") and ``builder(paths)``, where given, builds instead (dist.cached_rank_plans)."""
    key = (edge_index.data_ptr(), edge_type.data_ptr(), tuple(edge_index.shape), edge_index._version,
           edge_type._version, str(edge_index.device), n_nodes, num_relations, tile, chunk, aggr, int(split), bool(dw_tiles),
           paths if isinstance(paths, str) else tuple(paths), widths) + tuple(extra_key)
    hit = _CACHE.pop(key, None)
    if hit is not None:
        _CACHE[key] = hit           # most recently used last
        return hit[0]
    paths = resolve_paths(paths, edge_index, n_nodes, num_relations, widths, tile, chunk)
    if builder is None:
        plans = build_graph_plans(edge_index, edge_type, n_nodes, num_relations, tile, aggr, chunk=chunk, split=split,
                                  dw_tiles=dw_tiles, paths=paths)
    else:
        plans = builder(paths)
    nbytes = plans.nbytes()
    while _CACHE and (len(_CACHE) >= _CACHE_MAX or sum(v[3] for v in _CACHE.values()) + nbytes > _CACHE_MAX_BYTES):
        _CACHE.pop(next(iter(_CACHE)))
    # hold the key tensors so their storage (and data_ptr) cannot be recycled while cached
    _CACHE[key] = (plans, edge_index, edge_type, nbytes)
    return plans


def clear_plan_cache() -> None:
    _CACHE.clear()
