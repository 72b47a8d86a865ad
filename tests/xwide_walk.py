"""How the kernels of csrc/rgcn_xwide.hip walk a layout-0 plan, in plain Python over the plan's tensors: the host rules of the
source (d_W block shape, pieces, workspace; the forward / dX column blocks and K-slices) and, per plan, where every (piece,
relation) partial of d_W is stored and which row-tile counts the forward / dX kernel meets.  No GPU, no kernel arithmetic: the
tests use it to PROVE that a case runs the path it is named for (tests/test_xwide_walk.py on the torch builder's plans,
tests/test_gpu_xwide_edges.py on the device builder's).  The constants are held equal to the source by test_xwide_walk.py."""
from collections import Counter

KS = 32                 # kXwKS: gathered columns per K-slice
DW_B = 128              # kXwDwB
DW_WORKGROUPS = 512     # kXwDwWorkgroups
BIAS_ROWS = 256         # kXwBiasRows
BIAS_BLOCKS_MAX = 1024
PATHS = ("direct_first", "direct_middle", "direct_last", "slab0", "slab1")


def r4(w):
    return (w + 3) // 4 * 4


def align256(n):
    return (n + 255) & ~255


def xw_nb(n):
    return 64 if n <= 64 else 128


def dw_shape(din, dout):
    return 1 if din <= 64 < dout else (2 if dout <= 64 < din else 0)


def dw_block(din, dout):
    return {0: (DW_B, DW_B), 1: (64, 256), 2: (256, 64)}[dw_shape(din, dout)]


def dw_blocks(din, dout):
    bm, bn = dw_block(din, dout)
    return -(-din // bm) * -(-dout // bn)


def dw_pieces(n_units, din, dout):
    return max(1, min(n_units, DW_WORKGROUPS // dw_blocks(din, dout)))


def piece_start(p, n_units, pieces):
    return p * n_units // pieces


def bias_blocks(n_owned):
    return min(BIAS_BLOCKS_MAX, -(-n_owned // BIAS_ROWS))


def workspace_bytes(n_units, n_owned, din, dout):
    """rgcn_xwide_bwd_dw_workspace_bytes: the slabs [pieces][2][din][dout], then the d_bias block sums"""
    return align256(dw_pieces(n_units, din, dout) * 2 * din * dout * 4) + align256(bias_blocks(n_owned) * dout * 4)


def pieces_from_workspace(nbytes, n_owned, din, dout):
    """the number of pieces a queried workspace size was computed for (exact while a slab pair is at least 256 bytes)"""
    assert 8 * din * dout >= 256
    slab = nbytes - align256(bias_blocks(n_owned) * dout * 4)
    pieces = slab // (8 * din * dout)
    assert align256(pieces * 8 * din * dout) == slab, (nbytes, pieces)
    return pieces


def col_blocks(n):
    """forward / dX at output width n: (NB, column blocks, live waves of the last block)"""
    nb = xw_nb(n)
    ncb = -(-n // nb)
    n0 = (ncb - 1) * nb
    return nb, ncb, sum(n0 + w * (nb // 4) < n for w in range(4))


def k_slices(k):
    """(K-slices of the gathered width k, MFMA k-steps of the last slice)"""
    ns = -(-k // KS)
    return ns, min(KS, r4(k) - (ns - 1) * KS) >> 2


def _lists(plan):
    t = lambda a: [int(v) for v in a.cpu().tolist()]
    return t(plan.tile_ptr), t(plan.chunk_rel), t(plan.chunk_cnt), t(plan.rel_order)


def unit_rels(plan):
    """relation of every unit of rel_order (the d_W walk), and the slots the kernel multiplies in it"""
    _, chunk_rel, chunk_cnt, rel_order = _lists(plan)
    upc = plan.chunk // 64
    assert len(rel_order) == plan.n_units
    rels = [chunk_rel[u // upc] for u in rel_order]
    used = [min(64, chunk_cnt[u // upc] - 64 * (u % upc)) for u in rel_order]
    assert rels == sorted(rels) and all(0 < v <= 64 and v % 16 == 0 for v in used)
    return rels, used, [u % upc for u in rel_order]


def piece_paths(plan, din, dout):
    """Where xw_dw_kernel stores: ``stores`` {(piece, relation): path}, path one of PATHS -- the first and the last relation of a
    piece go to the piece's slab 0 / 1 when they continue from / into a neighbour (a relation that is both: slab 0), every other
    one straight to its output: ``direct_middle`` from the loop's relation change (followed by zero_acc), ``direct_first`` the
    same for the piece's first relation, ``direct_last`` from the final flush (a piece of one relation: direct_last).
    ``span`` {relation: (pieces it touches, slab slot xw_dw_reduce starts in or None when one piece stores it)}, ``units``
    {relation: units}, ``empty`` the relations 0..R' (R' = root) without units (xw_dw_reduce writes their zeros)."""
    rels, _, _ = unit_rels(plan)
    nu = len(rels)
    pieces = dw_pieces(nu, din, dout)
    stores, touched = {}, {}
    for p in range(pieces if nu else 0):
        u0, u1 = piece_start(p, nu, pieces), piece_start(p + 1, nu, pieces)
        if u0 >= u1:
            continue
        first, last = rels[u0], rels[u1 - 1]
        cont_in = u0 > 0 and rels[u0 - 1] == first
        cont_out = u1 < nu and rels[u1] == last
        runs = sorted(set(rels[u0:u1]))
        for i, r in enumerate(runs):
            if (r == first and cont_in) or (r == last and cont_out):
                path = "slab0" if r == first else "slab1"
            else:
                path = "direct_last" if i == len(runs) - 1 else ("direct_first" if i == 0 else "direct_middle")
            stores[(p, r)] = path
            touched.setdefault(r, []).append(p)
    span = {}
    for r, ps in touched.items():
        assert ps == list(range(ps[0], ps[-1] + 1))
        slot = None
        if len(ps) > 1:
            slot = int(stores[(ps[0], r)][-1])
            assert stores[(ps[0], r)].startswith("slab") and all(stores[(p, r)] == "slab0" for p in ps[1:])
            # xw_dw_reduce's own rule for the slot of the first piece
            assert slot == (0 if piece_start(ps[0], nu, pieces) == rels.index(r) else 1)
        else:
            assert stores[(ps[0], r)].startswith("direct")
        span[r] = (len(ps), slot)
    units = Counter(rels)
    empty = [r for r in range(plan.num_relations + 1) if r not in units]
    return dict(pieces=pieces, stores=stores, span=span, units=dict(units), empty=empty, paths=set(stores.values()))


def tile_walk(plan, k):
    """What xw_tile_kernel meets on this plan with a gathered width k: ``rt`` histogram of row tiles per chunk (chunk_cnt / 16,
    the MFMA walk's ``switch (nrt)``), ``slices`` / ``ksteps`` (K-slices, k-steps of the last), ``groups`` {(tile, relation):
    chunks}, ``last_rows`` owned rows of the last tile, ``tiles``."""
    tile_ptr, chunk_rel, chunk_cnt, _ = _lists(plan)
    assert all(c % 16 == 0 and 0 < c <= plan.chunk for c in chunk_cnt)
    groups = Counter()
    for t in range(len(tile_ptr) - 1):
        for c in range(tile_ptr[t], tile_ptr[t + 1]):
            groups[(t, chunk_rel[c])] += 1
    ns, ksteps = k_slices(k)
    return dict(rt=Counter(c // 16 for c in chunk_cnt), slices=ns, ksteps=ksteps, groups=dict(groups),
                last_rows=plan.n_owned - (len(tile_ptr) - 2) * plan.tile, tiles=len(tile_ptr) - 1)


def short_second_halves(plan):
    """units that are the second 64 slots of a 128-slot chunk and hold fewer than 64 used slots (xw_dw_kernel's ``used``)"""
    _, used, half = unit_rels(plan)
    return sum(h == 1 and v < 64 for v, h in zip(used, half))
