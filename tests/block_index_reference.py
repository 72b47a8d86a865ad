"""The index of one sampled block (csrc/rgcn_minibatch.hip) stated in CPU torch and Python integers, for
tests/test_block_index_reference.py (checks it against a brute-force layer) and tests/test_gpu_block_index.py (checks the device
arrays against it); ``walk``: the layer and its gradients computed by walking an index exactly as the kernels do, in the dtype of
its inputs; ``cases``: the small blocks both tests share; ``edge_cases``: the larger ones on the build's boundaries.  No tests here.

The root is relation R with one pseudo edge i -> i per destination, appended behind the block's edges.  All M = E_b + n_dst edges
are sorted stably by (relation, destination); a run of equal (relation, destination) is cut into rows of at most 256 consecutive
positions with scale 1 / run length (mean) or 1 (sum); rows lie relation-major in tiles of 16 slots that never straddle a relation
(the slots left over in a relation's last tile are empty: all zeros); ``dst_rows``: the slots grouped by destination, ascending
relation inside; ``src_row`` / ``src_scale``: slot and scale of every position grouped by source, ascending position inside."""
from typing import NamedTuple

import torch

ROW_EDGES = 256


class RefIndex(NamedTuple):
    tile_ptr: torch.Tensor     # int32 [R + 2]
    row_beg: torch.Tensor      # int32 [16 n_tiles]
    row_cnt: torch.Tensor
    row_dst: torch.Tensor
    row_scale: torch.Tensor    # float32
    edge_src: torch.Tensor     # int32 [M]
    dst_ptr: torch.Tensor      # int32 [n_dst + 1]
    dst_rows: torch.Tensor     # int32 [n_rows]
    src_ptr: torch.Tensor      # int32 [n_src + 1]
    src_row: torch.Tensor      # int32 [M]
    src_scale: torch.Tensor    # float32 [M]
    n_rows: int
    n_tiles: int
    n_src: int
    n_dst: int
    num_relations: int
    row_run: torch.Tensor      # int32 [16 n_tiles]: the length of the slot's run (reference only: the scale before rounding)
    mean: bool


ARRAYS = ("tile_ptr", "row_beg", "row_cnt", "row_dst", "row_scale", "edge_src", "dst_ptr", "dst_rows", "src_ptr", "src_row", "src_scale")


def build(edge_index, edge_type, n_src, n_dst, num_relations, aggr="mean") -> RefIndex:
    r1 = num_relations + 1
    loops = torch.arange(n_dst, dtype=torch.int64)
    src = torch.cat([edge_index[0].long().cpu(), loops]).tolist()
    dst = torch.cat([edge_index[1].long().cpu(), loops]).tolist()
    rel = torch.cat([edge_type.long().cpu(), torch.full((n_dst,), num_relations, dtype=torch.int64)]).tolist()
    m = len(src)
    order = sorted(range(m), key=lambda e: (rel[e], dst[e]))        # (sorted is stable)
    edge_src = [src[e] for e in order]
    # runs, then rows: (relation, destination, first position, positions, run length)
    rows, p = [], 0
    while p < m:
        q = p
        while q < m and (rel[order[q]], dst[order[q]]) == (rel[order[p]], dst[order[p]]):
            q += 1
        for b in range(p, q, ROW_EDGES):
            rows.append((rel[order[p]], dst[order[p]], b, min(ROW_EDGES, q - b), q - p))
        p = q
    per_rel = [0] * r1
    for row in rows:
        per_rel[row[0]] += 1
    tile_ptr = [0]
    for c in per_rel:
        tile_ptr.append(tile_ptr[-1] + (c + 15) // 16)
    n_tiles = tile_ptr[-1]
    n_slots = 16 * n_tiles
    row_beg, row_cnt, row_dst, row_run = [0] * n_slots, [0] * n_slots, [0] * n_slots, [0] * n_slots
    row_scale = torch.zeros(n_slots, dtype=torch.float32)
    one = torch.ones((), dtype=torch.float32)
    pos_slot, pos_scale = [0] * m, [None] * m
    seen, slots = [0] * r1, []
    for r, d, b, c, run in rows:
        slot = 16 * tile_ptr[r] + seen[r]
        seen[r] += 1
        slots.append(slot)
        scale = one / torch.tensor(float(run), dtype=torch.float32) if aggr == "mean" else one      # (fp32 division, as the device does)
        row_beg[slot], row_cnt[slot], row_dst[slot], row_scale[slot] = b, c, d, scale
        row_run[slot] = run
        for t in range(b, b + c):
            pos_slot[t], pos_scale[t] = slot, scale
    by_dst = sorted(range(len(rows)), key=lambda j: rows[j][1])
    dst_rows = [slots[j] for j in by_dst]
    dst_ptr = [0] * (n_dst + 1)
    for row in rows:
        dst_ptr[row[1] + 1] += 1
    for i in range(n_dst):
        dst_ptr[i + 1] += dst_ptr[i]
    by_src = sorted(range(m), key=lambda t: edge_src[t])
    src_ptr = [0] * (n_src + 1)
    for s in edge_src:
        src_ptr[s + 1] += 1
    for i in range(n_src):
        src_ptr[i + 1] += src_ptr[i]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    return RefIndex(i32(tile_ptr), i32(row_beg), i32(row_cnt), i32(row_dst), row_scale,
                    i32(edge_src), i32(dst_ptr), i32(dst_rows), i32(src_ptr), i32([pos_slot[t] for t in by_src]),
                    torch.stack([pos_scale[t] for t in by_src]) if m else torch.zeros(0, dtype=torch.float32),
                    len(rows), n_tiles, n_src, n_dst, num_relations, i32(row_run), aggr == "mean")


def walk(ix: RefIndex, x, weight, root, bias, g):
    """(out, {"x", "weight", "root", "bias"}) by walking ``ix`` through the steps of the kernels, in x's dtype: forward H = scaled
    row sums, Z = H W_rel, out = bias + destination sums; backward dH = g[row_dst] W_rel^T, dX = source sums of scale dH,
    dW = H^T g[row_dst].  ``weight`` dense [R, in, out]; ``root`` None: zeros.  (index_add_: the order inside a sum is torch's.)
    The scales are 1 / run length taken in x's dtype -- the float32 arrays of the index are that value rounded."""
    dt, r, (din, dout) = x.dtype, ix.num_relations, weight.shape[1:]
    w = torch.cat([weight.to(dt), (torch.zeros(din, dout, dtype=dt) if root is None else root.to(dt)).unsqueeze(0)], 0)
    n_slots, m = 16 * ix.n_tiles, int(ix.edge_src.shape[0])
    tiles = (ix.tile_ptr[1:] - ix.tile_ptr[:-1]).long()
    slot_rel = torch.repeat_interleave(torch.arange(r + 1), 16 * tiles)
    cnt = ix.row_cnt.long()
    slots = torch.arange(n_slots)
    # the positions of a row are row_beg .. row_beg + row_cnt - 1: rows in slot order are NOT in position order across relations
    pos_slot = torch.zeros(m, dtype=torch.int64)
    live = cnt > 0
    starts, lens = ix.row_beg.long()[live], cnt[live]
    pos = torch.repeat_interleave(starts - torch.cumsum(lens, 0) + lens, lens) + torch.arange(int(lens.sum()))
    pos_slot[pos] = torch.repeat_interleave(slots[live], lens)
    assert int(lens.sum()) == m and torch.equal(torch.sort(pos).values, torch.arange(m))      # every position in exactly one row
    scale = (1 / ix.row_run.to(dt).clamp(min=1)) * live.to(dt) if ix.mean else live.to(dt)
    assert torch.equal(scale.float(), ix.row_scale) and torch.equal(scale[ix.src_row.long()].float(), ix.src_scale)
    h = torch.zeros(n_slots, din, dtype=dt).index_add_(0, pos_slot, x[ix.edge_src.long()]) * scale[:, None]
    z = torch.bmm(h[:, None, :], w[slot_rel])[:, 0]
    dst_of = torch.repeat_interleave(torch.arange(ix.n_dst), (ix.dst_ptr[1:] - ix.dst_ptr[:-1]).long())
    out = torch.zeros(ix.n_dst, dout, dtype=dt).index_add_(0, dst_of, z[ix.dst_rows.long()])
    if bias is not None:
        out = out + bias.to(dt)
    gd = g.to(dt)[ix.row_dst.long()] * live.to(dt)[:, None] if n_slots else torch.zeros(0, dout, dtype=dt)
    dh = torch.bmm(gd[:, None, :], w[slot_rel].transpose(1, 2))[:, 0]
    src_of = torch.repeat_interleave(torch.arange(ix.n_src), (ix.src_ptr[1:] - ix.src_ptr[:-1]).long())
    dx = torch.zeros(ix.n_src, din, dtype=dt).index_add_(0, src_of, scale[ix.src_row.long()][:, None] * dh[ix.src_row.long()])
    # one product per relation over its slots (an index_add_ of 66,000 outer products, one after the other, is 3e-12 off at |d_root|
    # of 600 in float64: the blocked product is not)
    dw, tp = torch.zeros(r + 1, din, dout, dtype=dt), ix.tile_ptr.tolist()
    for rel in torch.nonzero(tiles)[:, 0].tolist():
        dw[rel] = h[16 * tp[rel]:16 * tp[rel + 1]].t() @ gd[16 * tp[rel]:16 * tp[rel + 1]]
    return out, {"x": dx, "weight": dw[:r], "root": dw[r], "bias": g.to(dt).sum(0)}


def _shuffled(src, dst, typ, seed):
    perm = torch.randperm(len(src), generator=torch.Generator().manual_seed(seed))
    t = lambda v: torch.tensor(v, dtype=torch.int64)[perm]
    return torch.stack([t(src), t(dst)]), t(typ)


def cases():
    """name -> (edge_index, edge_type, n_src, n_dst, num_relations): edges in no particular order"""
    out = {}
    g = torch.Generator().manual_seed(11)
    rnd = lambda hi, n: torch.randint(0, hi, (n,), generator=g).tolist()
    # runs of 600 (three rows), exactly 256 (one row) and 257 (two rows), duplicated triples, isolated destinations 9 .. 11
    src = rnd(40, 600) + rnd(40, 256) + rnd(40, 257) + [3, 3, 3, 5, 5] + rnd(40, 60)
    dst = [0] * 600 + [1] * 256 + [2] * 257 + [4, 4, 4, 6, 6] + [3 + d for d in rnd(6, 60)]
    typ = [0] * 600 + [0] * 256 + [1] * 257 + [2, 2, 2, 1, 1] + rnd(3, 60)
    out["runs"] = (*_shuffled(src, dst, typ, 1), 40, 12, 4)
    # relation 0: no row; 1: 16 rows (one full tile); 2: 17 rows (one row into a second tile); 3: none; isolated destinations 17 .. 19
    src = rnd(25, 16) + rnd(25, 17) + [7, 7]
    dst = list(range(16)) + list(range(17)) + [2, 2]
    typ = [1] * 16 + [2] * 17 + [2, 2]
    out["rel_rows"] = (*_shuffled(src, dst, typ, 2), 25, 20, 4)
    out["no_edges"] = (torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 9, 5, 3)
    out["no_dst"] = (torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 4, 0, 2)
    out["square"] = (*_shuffled(rnd(30, 200), rnd(30, 200), rnd(3, 200), 3), 30, 30, 3)
    out["one_row"] = (*_shuffled([0] * 5, [0] * 5, [0, 1, 1, 0, 0], 4), 1, 1, 2)
    # 300 relations, three of them in use
    out["many_rel"] = (*_shuffled(rnd(50, 90), rnd(20, 90), [0] * 30 + [7] * 30 + [299] * 30, 5), 50, 20, 300)
    return out


def _random_block(n_src, n_dst, r, e, seed, hub=600, dup=20, rels=None, every_relation=False):
    """``e`` edges in all: ``hub`` into destination 0 (relation ``rels[0]``), ``dup`` repeats of the first triples, the rest random
    over ``rels`` (default: all ``r``; ``every_relation``: the first ``r`` random edges take relations 0 .. r - 1).  The last
    source and the last destination are in use: their ids carry the top bit of the sort keys."""
    g = torch.Generator().manual_seed(seed)
    n = e - hub - dup
    assert n >= max(2, dup) and (not every_relation or n >= r)
    rels = torch.arange(r) if rels is None else torch.tensor(rels, dtype=torch.int64)
    rnd = lambda hi, k: torch.randint(0, hi, (k,), generator=g)
    src, dst, typ = rnd(n_src, n), rnd(n_dst, n), rels[rnd(len(rels), n)]
    if every_relation:
        typ[:r] = torch.arange(r)
    src[0], dst[1] = n_src - 1, n_dst - 1
    src = torch.cat([src, rnd(n_src, hub), src[:dup]])
    dst = torch.cat([dst, torch.zeros(hub, dtype=torch.int64), dst[:dup]])
    typ = torch.cat([typ, torch.full((hub,), int(rels[0])), typ[:dup]])
    perm = torch.randperm(e, generator=g)
    return torch.stack([src[perm], dst[perm]]), typ[perm], n_src, n_dst, r


def edge_cases():
    """name -> (edge_index, edge_type, n_src, n_dst, num_relations): the blocks that sit on the size, bit-width and pass-count
    boundaries of the device build (csrc/rgcn_minibatch.hip on csrc/rgcn_sort_scan.h).  Kept apart from ``cases``: up to 86,000
    edges.  A sort of b key bits takes ceil(b / 8) passes; bits_for(v) = bits that hold 0 .. v, at least 1."""
    out = {}
    # M = E_b + n_dst on both sides of one sort segment / one scan block (2,048) and of a four-segment sort workgroup (8,192):
    # n_dst = 300, so E_b = M - 300
    for m in (2047, 2048, 2049, 8191, 8192, 8193):
        out[f"m{m}"] = _random_block(400, 300, 3, m - 300, seed=m)
    # n_dst at and around a power of two: the keys' destination field is bits_for(n_dst - 1) = 1, 1, 8, 8, 9 bits wide, the dead
    # key n_dst of the destination sort needs bits_for(n_dst) = 1, 2, 8, 9, 9 (a second pass from n_dst = 256 on)
    for nd in (1, 2, 255, 256, 257):
        out[f"ndst{nd}"] = _random_block(nd + 40, nd, 3, 1500, seed=100 + nd)
    # R at and around a power of two, every relation in use: the root is relation R, bits_for(R) = 1, 2, 3, 8, 9, 9, 9, 10 bits
    # on top of bits_for(299) = 9: 10 .. 12 bits, two passes, up to R = 4; 17 .. 19 bits, three passes, from R = 255 on.  R + 1 =
    # 256, 257, 258, 512, 513 relations also put mb_rel_scan_kernel on both sides of one and of two trips of 256
    for r in (1, 2, 4, 255, 256, 257, 511, 512):
        out[f"rel{r}"] = _random_block(340, 300, r, 2500, seed=200 + r, every_relation=True)
    # the first sort in THREE passes with both fields on a power of two: bits_for(256) + bits_for(257 - 1) = 9 + 9 = 18 bits
    out["rel256_ndst257"] = _random_block(297, 257, 256, 2500, seed=300, every_relation=True)
    # the first sort in FOUR passes: bits_for(65,536) + bits_for(299) = 17 + 9 = 26 bits; 65,537 relations are 257 trips of
    # mb_rel_scan_kernel, rows in the first and in the last two
    out["rel65536"] = _random_block(340, 300, 65536, 2500, seed=301, rels=[0, 1, 65534, 65535])
    # the source sort: bits_for(n_src - 1) = 16 bits at 65,536 (two passes), 17 at 65,537 and 70,000 (three: the result lands in
    # the other buffer pair); n_src + 1 entries of src_ptr are scanned in 33 / 35 blocks where M = 5,300 takes three
    for ns in (65536, 65537, 70000):
        out[f"nsrc{ns}"] = _random_block(ns, 300, 3, 5000, seed=400 + ns % 1000)
    # the destination sort in three passes: bits_for(66,000) = 17 bits (and 2 + 17 = 19 bits, three passes, for the first sort)
    out["ndst66000"] = _random_block(66000, 66000, 3, 20000, seed=500)
    # runs of exactly 1, 512, 513 and 4,097 edges of relation 1 into destinations 0 .. 3: rows of (1), (256, 256), (256, 256, 1)
    # and 16 x 256 + 1 -- 23 rows, two tiles; relation 0 random into destinations 4 .. 9, relation 2 empty
    g = torch.Generator().manual_seed(600)
    rnd = lambda hi, n: torch.randint(0, hi, (n,), generator=g).tolist()
    lens = (1, 512, 513, 4097)
    src = rnd(60, sum(lens)) + rnd(60, 50)
    dst = [d for d, n in enumerate(lens) for _ in range(n)] + [4 + d for d in rnd(6, 50)]
    typ = [1] * sum(lens) + [0] * 50
    out["runs_1_512_513_4097"] = (*_shuffled(src, dst, typ, 6), 60, 10, 3)
    return out
