"""The link-prediction kernels (csrc/rgcn_linkpred.hip) where tests/test_gpu_linkpred.py stops: index sorts of two and
three radix passes and a node-pointer scan past 2,048^2 entries, relations with exactly a chunk's worth of triples and up to 65,536
relations, the exact backward workspace, strides and bases that are not the default, the rank kernel's remaining widths, grids of more
than 1,024 query blocks, filter entries and pointers out of range, non-finite scores, negatives past the grid cap, and the layouts
``linkpred._padded`` has to copy.  Same conventions as the first file, whose helpers are used: NaN in the inputs' pad columns,
sentinels and a guard row around every output, float results under ``oracle.tolerance.assert_close`` with the sums on absolute values
as ``cond``, everything integer EQUAL to tests/linkpred_reference.py."""
import numpy as np
import pytest
import torch

from oracle.tolerance import assert_close
from tests import linkpred_reference as R
from tests import test_gpu_linkpred as T

pytestmark = pytest.mark.gpu

SENT, DEV = T.SENT, T.DEV
NAN = float("nan")


def _lib():
    return T._lib()


def _np(t):
    return t.cpu().numpy().astype(np.int64)


def _second_call_has_the_same_bits(dz, drel, dev):
    zd, rd, sd, rdd, od, gd, ix = dev
    (_, dz2), (_, drel2) = T._output(*dz.shape), T._output(*drel.shape)
    assert T._backward_raw(zd, rd, sd, rdd, od, gd, ix, dz2, drel2) == 0
    assert torch.equal(dz, dz2) and torch.equal(drel, drel2)
    assert torch.equal(_lib().lp_score(zd, rd, sd, rdd, od), _lib().lp_score(zd, rd, sd, rdd, od))


# ---- 1. index build past one radix pass -----------------------------------------------------------------------------------
def _pooled(n_ids, n, pool, g):
    """n ids below n_ids: half of them from `pool` distinct ids spread over the whole range (0 and n_ids - 1 among them), so that a
    key repeats often enough for the sort's stability to show, half uniform; high and low digits both vary"""
    ids = torch.unique(torch.cat([torch.tensor([0, n_ids - 1]), torch.randint(0, n_ids, (pool,), generator=g)]))
    out = ids[torch.randint(0, len(ids), (n,), generator=g)]
    uniform = torch.rand(n, generator=g) < 0.5
    out[uniform] = torch.randint(0, n_ids, (int(uniform.sum()),), generator=g)
    return out


def _index_case(n_nodes, n_rel, seed, n=3000):
    """3,000 triples (6,000 node keys: three 2,048-key segments), about 1 % of them with an id out of range, of every kind"""
    g = torch.Generator().manual_seed(seed)
    s, o, r = _pooled(n_nodes, n, 150, g), _pooled(n_nodes, n, 150, g), _pooled(n_rel, n, 40, g)
    at = torch.randperm(n, generator=g)[:30].tolist()
    for j, t in enumerate(at[:29]):
        kind = j % 6
        if kind == 0:
            s[t] = n_nodes
        elif kind == 1:
            o[t] = 2 ** 40
        elif kind == 2:
            r[t] = n_rel
        elif kind == 3:
            s[t] = -1 - j
        elif kind == 4:
            r[t] = -1
        else:
            o[t] = n_nodes + 255
    s[at[29]], r[at[29]] = n_nodes, n_rel          # a bad node and a bad relation in one triple
    return s, r, o


def _check_index(ix, ref, n_nodes, n_rel, what):
    if ix.node_ptr is not None:
        ptr, slot = _np(ix.node_ptr), _np(ix.node_slot)
        assert np.array_equal(ptr, ref["node_ptr"]), f"{what}: node_ptr"
        assert np.array_equal(slot[:ptr[n_nodes]], ref["node_slot"]), f"{what}: node_slot is not in (node, slot) order"
        assert np.array_equal(np.sort(slot[ptr[n_nodes]:]), ref["bad_slots"]), f"{what}: the tail of node_slot"
    if ix.rel_ptr is not None:
        ptr, tri = _np(ix.rel_ptr), _np(ix.rel_triple)
        assert np.array_equal(ptr, ref["rel_ptr"]), f"{what}: rel_ptr"
        assert np.array_equal(tri[:ptr[n_rel]], ref["rel_triple"]), f"{what}: rel_triple is not in (relation, triple) order"
        assert np.array_equal(np.sort(tri[ptr[n_rel]:]), ref["bad_triples"]), f"{what}: the tail of rel_triple"


# bits_for(N): 8 bits (one pass) at 255, 9 at 256 -- the key N of a bad triple alone needs the ninth --, 16 at 65,535, 17 at 65,536
INDEX_SIZES = [(255, 255), (256, 256), (257, 257), (65535, 9), (65536, 65536)]


@pytest.mark.parametrize("n_nodes,n_rel", INDEX_SIZES)
def test_index_of_two_and_three_radix_passes(n_nodes, n_rel):
    lib = _lib()
    s, r, o = _index_case(n_nodes, n_rel, seed=n_nodes + n_rel)
    ref = R.triple_index(s, r, o, n_nodes, n_rel)
    assert ref["bad"] == R.BAD_NODE | R.BAD_REL and len(ref["bad_triples"]) == 30
    assert int(s.max()) >= 2 ** 40 or int(o.max()) >= 2 ** 40
    if n_nodes > 256:      # high and low digits both vary, and keys repeat
        ok = s[(s >= 0) & (s < n_nodes)]
        assert len(torch.unique(ok % 256)) > 200 and len(torch.unique(ok // 256)) > 1 and len(torch.unique(ok)) < len(ok) - 500
    sd, rd, od = T._ids(s), T._ids(r), T._ids(o)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    ix = lib.lp_index_build(sd, rd, od, n_nodes, n_rel, bad)
    _check_index(ix, ref, n_nodes, n_rel, f"N {n_nodes} R {n_rel}")
    assert int(bad.item()) == ref["bad"]
    for kw in ({"relations": False}, {"nodes": False}):
        bad.zero_()
        half = lib.lp_index_build(sd, rd, od, n_nodes, n_rel, bad, **kw)
        assert int(bad.item()) == ref["bad"], kw
        assert (half.rel_ptr is None) == ("relations" in kw) and (half.node_ptr is None) == ("nodes" in kw)
        for name in ("node_ptr", "node_slot", "rel_ptr", "rel_triple"):
            if getattr(half, name) is not None:
                assert torch.equal(getattr(half, name), getattr(ix, name)), (kw, name)


@pytest.mark.parametrize("n_nodes,n_rel", [(255, 255), (256, 256), (65536, 65536)])      # 1, 2 and 3 passes
def test_score_and_backward_on_an_index_of_each_pass_count(n_nodes, n_rel):
    s, r, o = _index_case(n_nodes, n_rel, seed=n_nodes + n_rel)
    g = torch.Generator().manual_seed(n_nodes)
    z, rel, gr = torch.randn(n_nodes, 20, generator=g), torch.randn(n_rel, 20, generator=g), torch.randn(len(s), generator=g)
    dz, drel, dev = T._check_case(z, rel, s, r, o, gr, what=f"index N {n_nodes} R {n_rel}")
    _second_call_has_the_same_bits(dz, drel, dev)


def test_node_pointer_scan_past_one_pass_of_its_top_kernel():
    """N + 1 = 4,194,310 counts: 2,049 sums of 2,048, so scan_top_kernel carries from its first 2,048 sums into the last one"""
    n_nodes, n_rel, n, top = 2048 * 2048 + 5, 3, 3000, 2048 * 2048
    g = torch.Generator().manual_seed(9)
    s, o = torch.randint(0, n_nodes, (n,), generator=g), torch.randint(0, n_nodes, (n,), generator=g)
    r = torch.randint(0, n_rel, (n,), generator=g)
    edge = torch.tensor([0, n_nodes - 1, top - 1, top, top + 1, top + 3, 2047, 2048, 2049, 2048 * 1024 - 1, 2048 * 1024, top - 2048,
                         top - 2047, top + 2])
    s[:len(edge)] = edge
    o[100:100 + len(edge)] = edge.flip(0)
    o[200:205] = top + 1                                      # a few slots on one node behind the carry
    s[300], o[301], r[302] = n_nodes, -1, n_rel
    perm = torch.randperm(n, generator=g)
    s, r, o = s[perm], r[perm], o[perm]
    sd, rd, od = T._ids(s), T._ids(r), T._ids(o)
    ix = _lib().lp_index_build(sd, rd, od, n_nodes, n_rel)
    torch.cuda.synchronize()
    ok = torch.as_tensor(R.valid_triples(s.numpy(), r.numpy(), o.numpy(), n_nodes, n_rel)[0])
    slot_node = torch.stack([s, o], 1).reshape(-1)
    slots = torch.nonzero(ok.repeat_interleave(2)).reshape(-1)
    order = torch.argsort(slot_node[slots], stable=True)
    want_ptr = torch.searchsorted(slot_node[slots][order], torch.arange(n_nodes + 1))
    got_ptr = ix.node_ptr.cpu().long()
    assert int(want_ptr[-1]) == 2 * (n - 3) and int(want_ptr[top]) < int(want_ptr[top + 1]) < int(want_ptr[-1])
    assert torch.equal(got_ptr, want_ptr)
    assert torch.equal(ix.node_slot.cpu().long()[:2 * (n - 3)], slots[order])
    _check_index(ix, R.triple_index(s, r, o, n_nodes, n_rel), n_nodes, n_rel, "N 2048^2 + 5")


# ---- 2. drel: chunk edges and many relations --------------------------------------------------------------------------------
CHUNK_COUNTS = (0, 1, 3, 255, 256, 257, 512, 513, 0, 70)


def _chunk_case(width, seed=4):
    g = torch.Generator().manual_seed(seed)
    n_nodes, n_rel, n = 40, len(CHUNK_COUNTS), sum(CHUNK_COUNTS)
    z, rel = torch.randn(n_nodes, width, generator=g), torch.randn(n_rel, width, generator=g)
    s, o = (torch.randint(0, n_nodes - 1, (n,), generator=g) for _ in range(2))       # node 39 in no triple
    r = torch.repeat_interleave(torch.arange(n_rel), torch.tensor(CHUNK_COUNTS))
    r = r[torch.randperm(n, generator=g)]
    assert tuple(torch.bincount(r, minlength=n_rel).tolist()) == CHUNK_COUNTS
    return z, rel, s, r, o, torch.randn(n, generator=g)


# lane groups per wave: 64 at width 4 (relations with 1 and 3 triples leave most of them idle), 21 at 12 (63 lanes), 5 at 44
# (55 lanes), 2 at 100 (50 lanes), 2 at 128
@pytest.mark.parametrize("width", [4, 12, 44, 100, 128])
def test_drel_with_relations_of_exactly_a_chunk(width):
    z, rel, s, r, o, g = _chunk_case(width)
    dz, drel, dev = T._check_case(z, rel, s, r, o, g, what=f"chunk edges width {width}")
    for row in (drel[0], drel[8], dz[39]):                    # no triple: +0 over the sentinels
        assert bool((row == 0).all()) and not bool(torch.signbit(row).any())
    _second_call_has_the_same_bits(dz, drel, dev)


@pytest.mark.parametrize("width", [4, 20])
@pytest.mark.parametrize("n_rel", [257, 1000, 65536])
def test_drel_with_many_relations(n_rel, width):
    """lp_chunk_ptr_kernel with 2, 4 and 256 relations per thread; most relations empty, three with more than one chunk"""
    g = torch.Generator().manual_seed(n_rel + width)
    n_nodes, n = 50, 4000
    z, rel = torch.randn(n_nodes, width, generator=g), torch.randn(n_rel, width, generator=g)
    s, o = (torch.randint(0, n_nodes, (n,), generator=g) for _ in range(2))
    some = torch.randperm(n_rel - 2, generator=g)[:21] + 1            # distinct, neither 0 nor R - 1
    r = some[1:][torch.randint(0, 20, (n,), generator=g)]
    r[:300], r[300:900], r[900:1600] = 0, n_rel - 1, some[0]
    r = r[torch.randperm(n, generator=g)]
    count = torch.bincount(r, minlength=n_rel)
    assert int(count[0]) == 300 and int(count[n_rel - 1]) == 600 and int((count > 256).sum()) == 3
    assert int((count == 0).sum()) == n_rel - 23
    dz, drel, dev = T._check_case(z, rel, s, r, o, torch.randn(n, generator=g), what=f"R {n_rel} width {width}")
    empty = drel[(count == 0).to(DEV)]
    assert bool((empty == 0).all()) and not bool(torch.signbit(empty).any())
    _second_call_has_the_same_bits(dz, drel, dev)


def test_backward_workspace_of_exactly_the_stated_bytes():
    """every relation non-empty and 257 triples each: 2 chunks per relation = T / 256 + R, the most the workspace is sized for"""
    lib = _lib()
    n_rel, width, guard = 5, 20, 4096
    n = 257 * n_rel
    g = torch.Generator().manual_seed(12)
    z, rel = torch.randn(30, width, generator=g), torch.randn(n_rel, width, generator=g)
    s, o = (torch.randint(0, 30, (n,), generator=g) for _ in range(2))
    r = torch.arange(n_rel).repeat_interleave(257)[torch.randperm(n, generator=g)]
    gr = torch.randn(n, generator=g)
    assert n % 256 != 0 and n // 256 + n_rel == 2 * n_rel
    zd, rd, sd, rdd, od, gd = T._input(z), T._input(rel), T._ids(s), T._ids(r), T._ids(o), gr.to(DEV)
    ix = lib.lp_index_build(sd, rdd, od, 30, n_rel)
    need = lib.load().rgcn_lp_backward_workspace_bytes(n, n_rel, width)
    assert need >= 4 * (n_rel + 1) + 2 * n_rel * 20 * 4
    buf = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    (zbuf, dz), (rbuf, drel) = T._output(30, width), T._output(n_rel, width)
    assert T._backward_raw(zd, rd, sd, rdd, od, gd, ix, dz, drel, workspace=buf[:need]) == 0
    assert bool((buf[need:] == 0xA5).all()), "the workspace was written behind its stated size"
    ref_dz, ref_drel = R.backward(z, rel, s, r, o, gr)
    c_dz, c_drel = R.backward_cond(z, rel, s, r, o, gr)
    assert_close(dz.cpu().numpy(), ref_dz, c_dz, "exact workspace dz")
    assert_close(drel.cpu().numpy(), ref_drel, c_drel, "exact workspace drel")
    T._check_output_pads(zbuf, 30, width, "dz")
    T._check_output_pads(rbuf, n_rel, width, "drel")
    # one byte fewer: refused before anything is launched
    buf.fill_(0xA5)
    (zbuf, dz), (rbuf, drel) = T._output(30, width), T._output(n_rel, width)
    assert T._backward_raw(zd, rd, sd, rdd, od, gd, ix, dz, drel, workspace=buf[:need - 1]) == -6
    assert bool((buf == 0xA5).all()) and bool((zbuf == SENT).all()) and bool((rbuf == SENT).all())


# ---- 3. strides and bases ---------------------------------------------------------------------------------------------------
def _inside(t, ld, fill):
    """(buffer, view): t [rows, width] as a 16-byte aligned view of row stride ld that starts at row 2, column 4 of a buffer of
    `fill`; t None: the view is left as it is filled"""
    rows, width = t if isinstance(t, tuple) else t.shape
    assert ld % 4 == 0 and ld >= 4 + width
    buf = torch.full((rows + 4, ld), fill, device=DEV)
    view = buf[2:2 + rows, 4:4 + width]
    if not isinstance(t, tuple):
        view.copy_(t.to(DEV))
    assert view.data_ptr() % 16 == 0 and view.data_ptr() != buf.data_ptr() and view.stride(0) == ld
    return buf, view


@pytest.mark.parametrize("width", [20, 3])
def test_four_distinct_strides_and_bases_inside_larger_buffers(width):
    lib = _lib()
    ldz, ldr, lddz, lddrel = 24, 32, 28, 40
    w4 = T._ld(width)
    z, rel, s, r, o, g = T._random_case(50, 5, width, 1000, seed=31 + width)
    s[7], r[9] = 50, -1
    sd, rdd, od, gd = T._ids(s), T._ids(r), T._ids(o), g.to(DEV)
    # the default layout
    zd, rd = T._input(z), T._input(rel)
    ix = lib.lp_index_build(sd, rdd, od, 50, 5)
    score = lib.lp_score(zd, rd, sd, rdd, od)
    (_, dz), (_, drel) = T._output(50, width), T._output(5, width)
    assert T._backward_raw(zd, rd, sd, rdd, od, gd, ix, dz, drel) == 0
    gq = torch.Generator().manual_seed(width)
    a, e, rq = torch.randint(0, 50, (70,), generator=gq), torch.randint(0, 50, (70,), generator=gq), torch.randint(0, 5, (70,), generator=gq)
    fptr, fidx = T._csr(T._lists(50, 70, e, gq))
    rank = lib.lp_rank(zd, rd, T._ids(a), T._ids(rq), T._ids(e), fptr, fidx)
    # the same data behind other strides and bases
    (zb, zv), (rb, rv) = _inside(z, ldz, NAN), _inside(rel, ldr, NAN)
    (dzb, dzv), (drb, drv) = _inside((50, width), lddz, SENT), _inside((5, width), lddrel, SENT)
    assert len({zv.stride(0), rv.stride(0), dzv.stride(0), drv.stride(0), w4}) == 5
    zb0, rb0 = zb.clone(), rb.clone()
    assert torch.equal(lib.lp_score(zv, rv, sd, rdd, od), score)
    assert T._backward_raw(zv, rv, sd, rdd, od, gd, ix, dzv, drv) == 0
    assert torch.equal(dzv, dz) and torch.equal(drv, drel)
    got = lib.lp_rank(zv, rv, T._ids(a), T._ids(rq), T._ids(e), fptr, fidx)
    assert torch.equal(got[0], rank[0]) and torch.equal(got[1], rank[1])
    # nothing outside the views but the +0 pads of the last 16-byte piece
    for buf, ref, rows, what in ((dzb, dz, 50, "dz"), (drb, drel, 5, "drel")):
        want = torch.full_like(buf, SENT)
        want[2:2 + rows, 4:4 + w4] = 0
        want[2:2 + rows, 4:4 + width] = ref
        assert torch.equal(buf, want), f"{what}: written outside its view"
        assert not bool(torch.signbit(buf[2:2 + rows, 4 + width:4 + w4]).any())
    assert torch.equal(zb.view(torch.int32), zb0.view(torch.int32)) and torch.equal(rb.view(torch.int32), rb0.view(torch.int32))
    # against float64 too: the default call is not its own reference
    ref_dz, ref_drel = R.backward(z, rel, s, r, o, g)
    c_dz, c_drel = R.backward_cond(z, rel, s, r, o, g)
    assert_close(dzv.cpu().numpy(), ref_dz, c_dz, f"strided dz width {width}")
    assert_close(drv.cpu().numpy(), ref_drel, c_drel, f"strided drel width {width}")


# ---- 4. ranks -----------------------------------------------------------------------------------------------------------------
def _rank_raw(z, rel, a, r, e, fptr, fidx, flen):
    """rgcn_lp_rank at the C ABI, with filter_ptr / filter_len as they are (the binding refuses nothing of them either, but passes
    the length of filter_idx)"""
    c = _lib().load()
    nq = len(a)
    greater, equal = (torch.full((nq + 1,), -7, dtype=torch.int64, device=DEV) for _ in range(2))
    ws = torch.empty(c.rgcn_lp_rank_workspace_bytes(nq, z.shape[0], z.shape[1]), dtype=torch.uint8, device=DEV)
    st = c.rgcn_lp_rank(z.data_ptr(), z.stride(0), rel.data_ptr(), rel.stride(0), z.shape[1], z.shape[0], rel.shape[0], a.data_ptr(),
                        r.data_ptr(), e.data_ptr(), nq, fptr.data_ptr(), fidx.data_ptr(), flen, greater.data_ptr(), equal.data_ptr(),
                        ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0 and int(greater[nq]) == -7 and int(equal[nq]) == -7
    return _np(greater[:nq]), _np(equal[:nq])


def _rank_equals(z, rel, a, r, e, lists, what):
    fptr, fidx = T._csr(lists) if lists is not None else (None, None)
    got_g, got_e = _lib().lp_rank(T._input(z), T._input(rel), T._ids(a), T._ids(r), T._ids(e), fptr, fidx)
    with np.errstate(invalid="ignore"):
        sc, _ = R.rank_scores(z, rel, a, r)
    ref_g, ref_e = R.rank_counts(sc, np.asarray(e), lists)
    assert np.array_equal(_np(got_g), ref_g), (what, np.flatnonzero(_np(got_g) != ref_g)[:10])
    assert np.array_equal(_np(got_e), ref_e), (what, np.flatnonzero(_np(got_e) != ref_e)[:10])
    return sc, ref_g, ref_e


# padded widths 16 (1, 3), 32 (17), 48 (36), 80 (68), 112 (100), 128 (127): a masked last piece in every KT
@pytest.mark.parametrize("width", [1, 3, 17, 36, 68, 100, 127])
@pytest.mark.parametrize("filtered", [False, True])
def test_rank_counts_at_the_remaining_widths(width, filtered):
    for n_nodes in (33, 130):
        z, rel, a, r, e, g = T._exact_case(n_nodes, 70, width, seed=width + n_nodes)
        lists = T._lists(n_nodes, 70, e, g) if filtered else None
        sc, ref_g, ref_e = _rank_equals(z, rel, a, r, e, lists, f"width {width} N {n_nodes}")
        assert np.abs(sc).max() < 2 ** 24
        assert ref_g.sum() > 0 and ref_e.sum() > 0


def _short_lists(n_nodes, n_q, target, seed):
    """per query, in turn: no list, only the target, three distinct ids"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, n_nodes, n_q)
    target = np.asarray(target)
    return [[] if i % 3 == 0 else [int(target[i])] if i % 3 == 1 else [int(b), int((b + 7) % n_nodes), int((b + 19) % n_nodes)]
            for i, b in enumerate(base)]


# 1,025 query blocks: one entity slice, whose eight waves deal the block's 64 filter lists; 313 blocks: three slices of 300 entities
@pytest.mark.parametrize("n_q,n_nodes,width", [(65600, 40, 4), (20000, 300, 20)])
def test_rank_with_many_query_blocks(n_q, n_nodes, width):
    z, rel, a, r, e, g = T._exact_case(n_nodes, n_q, width, seed=n_q)
    lists = _short_lists(n_nodes, n_q, e, seed=n_q)
    sc, ref_g, ref_e = _rank_equals(z, rel, a, r, e, lists, f"Q {n_q}")
    assert np.abs(sc).max() < 2 ** 24 and ref_g[-64:].sum() > 0 and ref_e[-64:].sum() > 0
    _rank_equals(z, rel, a, r, e, None, f"Q {n_q} raw")


def _filter_edge_case():
    n_nodes, n_q = 50, 20
    z, rel, a, r, e, g = T._exact_case(n_nodes, n_q, 20, seed=77)
    lists = []
    for i in range(n_q):
        ids = torch.randperm(n_nodes, generator=g)[:6].tolist()
        if i % 4 == 0:
            ids = [-1, ids[0], n_nodes, ids[1], 2 ** 40, int(e[i]), ids[2], -2 ** 40, n_nodes + 15]
        elif i % 4 == 1:
            ids = [n_nodes, -1, 2 ** 40, 2 ** 31, -50]                 # nothing in range
        elif i % 4 == 2:
            ids = ids + [int(e[i]), 2 ** 62] + list(range(n_nodes, n_nodes + 20))      # more than one tile of sixteen entries
        lists.append(ids)
    return z, rel, a, r, e, lists


def test_rank_filter_entries_out_of_range_count_nothing():
    z, rel, a, r, e, lists = _filter_edge_case()
    _, ref_g, ref_e = _rank_equals(z, rel, a, r, e, lists, "filter entries out of range")
    # the same counts as with those entries taken out
    clean = [[v for v in ids if 0 <= v < 50] for ids in lists]
    g2, e2 = R.rank_counts(R.rank_scores(z, rel, a, r)[0], e.numpy(), clean)
    assert np.array_equal(ref_g, g2) and np.array_equal(ref_e, e2)
    raw_g, raw_e = R.rank_counts(R.rank_scores(z, rel, a, r)[0], e.numpy())
    assert (raw_g[1::4] == ref_g[1::4]).all() and (raw_e[1::4] == ref_e[1::4]).all() and (raw_g != ref_g).any()


def test_rank_filter_ptr_is_clamped_to_the_filter():
    z, rel, a, r, e, g = T._exact_case(50, 20, 20, seed=78)
    lists = [torch.randperm(50, generator=g)[:5].tolist() for _ in range(20)]
    ptr = np.zeros(21, dtype=np.int64)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    idx = np.array([v for x in lists for v in x], dtype=np.int64)
    sc, _ = R.rank_scores(z, rel, a, r)
    zd, rd, ad, rdd, ed = T._input(z), T._input(rel), T._ids(a), T._ids(r), T._ids(e)

    def clamped(ptr, flen):
        p = np.clip(ptr, 0, flen)
        return [idx[p[i]:p[i + 1]].tolist() for i in range(20)]

    whole = R.rank_counts(sc, e.numpy(), lists)
    for what, p, flen in (("ptr[0] < 0", np.concatenate([[-3], ptr[1:]]), len(idx)),
                          ("ptr[0] far below 0", np.concatenate([[-2 ** 40], ptr[1:]]), len(idx)),
                          ("ptr[Q] > filter_len", ptr, len(idx) - 7),          # cuts list 18 short, leaves list 19 empty
                          ("both", np.concatenate([[-1], ptr[1:]]), len(idx) - 2)):
        ref_g, ref_e = R.rank_counts(sc, e.numpy(), clamped(p, flen))
        got_g, got_e = _rank_raw(zd, rd, ad, rdd, ed, T._ids(p), T._ids(idx), flen)
        assert np.array_equal(got_g, ref_g) and np.array_equal(got_e, ref_e), what
        if flen == len(idx):
            assert np.array_equal(ref_g, whole[0]) and np.array_equal(ref_e, whole[1])
    assert clamped(ptr, len(idx) - 7)[19] == [] and len(clamped(ptr, len(idx) - 7)[18]) == 3
    # no entries, a filter_ptr of zeros: the raw ranks
    zeros = torch.zeros(21, dtype=torch.int64, device=DEV)
    got = _lib().lp_rank(zd, rd, ad, rdd, ed, zeros, torch.zeros(0, dtype=torch.int64, device=DEV))
    raw = R.rank_counts(sc, e.numpy())
    assert np.array_equal(_np(got[0]), raw[0]) and np.array_equal(_np(got[1]), raw[1])
    got_g, got_e = _rank_raw(zd, rd, ad, rdd, ed, zeros, T._ids(idx), 0)
    assert np.array_equal(got_g, raw[0]) and np.array_equal(got_e, raw[1])


def _non_finite_case():
    """integer-valued z with one +inf and one NaN; queries whose target is the NaN row (0), the +inf row (1), whose anchor holds the
    +inf (2) and with an id out of range (3, 4, 5)"""
    n_nodes, width, inf_row, nan_row = 40, 8, 5, 7
    z, rel, a, r, e, g = T._exact_case(n_nodes, 24, width, seed=21)
    rel[:, 2] = torch.tensor([1., -1., 1.])
    z[:, 2] = torch.tensor([1., -2., 0., 2.]).repeat(10)        # rows 2, 6, 10, ..: a zero where the +inf sits
    z[inf_row, 2] = float("inf")
    z[nan_row, 1] = NAN
    a = (a // 4) * 4 + torch.tensor([0, 1, 3]).repeat(8)          # anchors with a non-zero column 2 ..
    a[a == nan_row] = 1
    a[a == inf_row] = 9
    e[0], e[1], a[2] = nan_row, inf_row, inf_row                   # .. but for query 2, whose anchor holds the +inf
    r[2], e[2] = 0, 3
    a[3], r[4], e[5] = n_nodes, 3, -1                              # ids out of range beside them
    ok = np.ones(24, dtype=bool)
    ok[3:6] = False
    with np.errstate(invalid="ignore"):
        sc, _ = R.rank_scores(z, rel, a.clamp(0, n_nodes - 1), r.clamp(0, 2))
    assert np.isnan(sc[ok]).any() and np.isposinf(sc[ok]).any() and np.isneginf(sc[ok]).any()
    assert np.isnan(sc[0, nan_row]) and np.isinf(sc[1, inf_row]) and np.isnan(sc[2, 2]) and np.isinf(sc[2, 0])
    return z, rel, a, r, e, g, ok, sc


def test_rank_non_finite_scores():
    """+inf, -inf and NaN scores: sums and comparisons on them do not depend on the order of the sum, so the counts are numpy's"""
    z, rel, a, r, e, g, ok, sc = _non_finite_case()
    n_nodes = z.shape[0]
    ref_g, ref_e = R.rank_counts(sc, e.clamp(0, n_nodes - 1).numpy())
    assert ref_g[0] == 0 and ref_e[0] == 0                         # a NaN target: nothing is greater, nothing equal
    ref_g[~ok], ref_e[~ok] = -1, -1
    lists = T._lists(n_nodes, 24, e.clamp(0, n_nodes - 1), g)
    fil_g, fil_e = R.rank_counts(sc, e.clamp(0, n_nodes - 1).numpy(), lists)
    fil_g[~ok], fil_e[~ok] = -1, -1
    zd, rd = T._input(z), T._input(rel)
    got = _lib().lp_rank(zd, rd, T._ids(a), T._ids(r), T._ids(e))
    assert np.array_equal(_np(got[0]), ref_g), (_np(got[0]), ref_g)
    assert np.array_equal(_np(got[1]), ref_e), (_np(got[1]), ref_e)
    got = _lib().lp_rank(zd, rd, T._ids(a), T._ids(r), T._ids(e), *T._csr(lists))
    assert np.array_equal(_np(got[0]), fil_g), (_np(got[0]), fil_g)
    assert np.array_equal(_np(got[1]), fil_e), (_np(got[1]), fil_e)


def _random_rank_case(width, seed, n_nodes=300, n_q=128, n_copies=40):
    """standard normal; the last 40 rows are bit copies of other rows, the first 20 of them of targets; filter lists that hold some
    of the copies"""
    g = torch.Generator().manual_seed(seed)
    first = n_nodes - n_copies
    z, rel = torch.randn(n_nodes, width, generator=g), torch.randn(4, width, generator=g)
    a, e = torch.randint(0, first, (n_q,), generator=g), torch.randint(0, first, (n_q,), generator=g)
    r = torch.randint(0, 4, (n_q,), generator=g)
    z[first:] = z[torch.cat([e[:20], torch.randint(0, first, (n_copies - 20,), generator=g)])]
    lists = []
    for i in range(n_q):
        ids = torch.randperm(n_nodes, generator=g)[:int(torch.randint(0, 30, (1,), generator=g))].tolist()
        if i % 3 == 0 and i < 20:
            ids = sorted(set(ids) | {first + i})            # the copy of this query's target is filtered
        lists.append(ids)
    return z, rel, a, r, e, lists


def _pick_random_rank_case(width):
    """tests/test_gpu_linkpred.py's condition on the inputs: the first seed below 20 whose float64 bands, with the bit copies of
    the target taken out of the candidates, are open for at most 2 % of the queries"""
    for seed in range(20):
        z, rel, a, r, e, lists = case = _random_rank_case(width, seed)
        out = [sorted(set(lists[i]) | set(T._copies(z, e, i))) for i in range(len(e))]
        lo, hi = R.rank_band(z.numpy(), rel.numpy(), a.numpy(), r.numpy(), e.numpy(), out)
        open_ = int((lo != hi).sum())
        if open_ <= 0.02 * len(lo):
            return case, lo, hi, open_, seed
    raise AssertionError("no seed gives at most 2 % open bands")


@pytest.mark.parametrize("width", [17, 100, 127])
def test_rank_random_inputs_copies_and_bands_at_the_remaining_widths(width):
    (z, rel, a, r, e, lists), lo, hi, open_, seed = _pick_random_rank_case(width)
    n_q = len(e)
    assert open_ <= 0.02 * n_q
    copies = [T._copies(z, e, i) for i in range(n_q)]
    want_equal = np.array([len([v for v in copies[i] if v != int(e[i]) and v not in set(lists[i])]) for i in range(n_q)])
    assert want_equal[:20].sum() >= 10 and want_equal[:20].sum() < sum(len(c) - 1 for c in copies[:20])
    got_g, got_e = (_np(t) for t in _lib().lp_rank(T._input(z), T._input(rel), T._ids(a), T._ids(r), T._ids(e), *T._csr(lists)))
    print(f"rank random width {width}: seed {seed}, open bands {open_}/{n_q}, equal counted {got_e.sum()} (expected "
          f"{want_equal.sum()}), greater outside its band in {int(((got_g < lo) | (got_g > hi)).sum())} queries")
    assert np.array_equal(got_e, want_equal)
    assert ((got_g >= lo) & (got_g <= hi)).all()
    raw_g, raw_e = (_np(t) for t in _lib().lp_rank(T._input(z), T._input(rel), T._ids(a), T._ids(r), T._ids(e)))
    lo_r, hi_r = R.rank_band(z.numpy(), rel.numpy(), a.numpy(), r.numpy(), e.numpy(), copies)
    assert ((raw_g >= lo_r) & (raw_g <= hi_r)).all() and (raw_g >= got_g).all() and (raw_e >= got_e).all()
    assert np.array_equal(raw_e, [len(c) - 1 for c in copies])


# ---- 5. negatives -----------------------------------------------------------------------------------------------------------
def test_corrupt_past_the_grid_cap():
    """2^24 + 8 outputs on a grid capped at 65,536 x 256 = 2^24 threads: the last eight are a second turn of the grid-stride loop"""
    from scaling_rgcn_training_amd.linkpred import corrupt
    n, k, n_nodes, seed, cap = 2097153, 8, 1000003, 20240607, 65536 * 256
    total = n * k
    assert total == cap + 8
    g = torch.Generator().manual_seed(1)
    s, o = (torch.randint(0, n_nodes, (n,), generator=g) for _ in range(2))
    r = torch.randint(0, 11, (n,), generator=g)
    sd, rd, od = T._ids(s), T._ids(r), T._ids(o)
    so, ro, oo = corrupt(sd, rd, od, n_nodes, k, seed)
    assert so.shape == ro.shape == oo.shape == (total,)
    pos = np.unique(np.concatenate([np.arange(64), np.arange(total - 64, total), np.arange(cap - 64, cap), np.arange(cap, cap + 8),
                                    np.random.default_rng(5).integers(0, total, 2000)]))
    assert len(pos) >= 2000
    pd = T._ids(pos)
    for got, ref in zip((so, ro, oo), R.corrupt_at(s.numpy(), r.numpy(), o.numpy(), n_nodes, k, seed, pos)):
        assert np.array_equal(got[pd].cpu().numpy(), ref)
    # the whole tensors
    s_rep, o_rep = sd.repeat_interleave(k), od.repeat_interleave(k)
    assert torch.equal(ro, rd.repeat_interleave(k))
    ds, do = so != s_rep, oo != o_rep
    assert not bool((ds & do).any())                              # one end is the source triple's
    for t in (so, oo):
        assert int(t.min()) >= 0 and int(t.max()) < n_nodes
    rate_s, rate_o = float(ds.double().mean()), float(do.double().mean())
    print(f"corrupt past the grid cap: subject replaced at rate {rate_s:.6f}, object at {rate_o:.6f}")
    assert abs(rate_s - 0.5) < 0.001 and abs(rate_o - 0.5) < 0.001


@pytest.mark.parametrize("n,k,seed", [(7, 1000, 99), (300, 3, 2 ** 63 - 1), (300, 3, 0)])
def test_corrupt_many_negatives_and_the_ends_of_the_seed_range(n, k, seed):
    from scaling_rgcn_training_amd.linkpred import corrupt
    g = torch.Generator().manual_seed(k)
    s, o = (torch.randint(0, 1000, (n,), generator=g) for _ in range(2))
    r = torch.randint(0, 9, (n,), generator=g)
    got = corrupt(T._ids(s), T._ids(r), T._ids(o), 1000, k, seed)
    for a, b in zip(got, R.corrupt(s.numpy(), r.numpy(), o.numpy(), 1000, k, seed)):
        assert np.array_equal(a.cpu().numpy(), b)


# ---- 6. the Python layer ----------------------------------------------------------------------------------------------------
def _layouts(z):
    """[(name, leaf, view, region, copied)]: z [N, E] on the device as a leaf and the view of it that is handed to the decoder -- as
    it is; with a base 4 bytes off a 16-byte boundary; with a row stride that is no multiple of 4; with a column stride that is
    not 1 (at width 1 also one that the kernels read where it lies: rows 16 bytes apart).  ``region`` cuts the viewed part out of
    a tensor shaped like the leaf; ``copied``: must ``_padded`` copy it?"""
    n, w = z.shape
    zd = z.to(DEV)

    def leaf_of(shape, put):
        leaf = torch.full(shape, NAN, device=DEV)
        put(leaf).copy_(zd)
        return leaf.requires_grad_(True)

    cuts = [("contiguous", (n, w), lambda t: t, w % 4 != 0),
            ("base off by 4 bytes", (n, w + 4), lambda t: t[:, 1:1 + w], True),
            ("row stride w + 1", (n, w + 1), lambda t: t[:, :w], True),
            ("transposed", (w, n), lambda t: t.t(), True)]
    if w == 1:
        cuts.append(("column stride 4 n", (1, 4 * n), lambda t: t[:, ::4].t(), False))
    out = [(name, leaf_of(shape, cut), cut, copied) for name, shape, cut, copied in cuts]
    out = [(name, leaf, cut(leaf), cut, copied) for name, leaf, cut, copied in out]
    views = {name: view for name, _, view, _, _ in out}
    assert views["base off by 4 bytes"].data_ptr() % 16 == 4 and views["row stride w + 1"].stride(0) % 4 != 0
    assert views["transposed"].stride() == (1, n) and (w != 1 or views["column stride 4 n"].stride() == (4, 4 * n))
    return out


@pytest.mark.parametrize("width", [20, 1])
def test_distmult_on_layouts_that_have_to_be_copied(width):
    from scaling_rgcn_training_amd.linkpred import DistMult, _padded, ranks
    z, rel, s, r, o, g = T._random_case(50, 5, width, 300, seed=40 + width)
    sd, rd, od, gd = T._ids(s), T._ids(r), T._ids(o), g.to(DEV)
    dec = DistMult(5, width).to(DEV)
    with torch.no_grad():
        dec.rel.copy_(rel)
    results = {}
    for name, leaf, view, region, copied in _layouts(z):
        assert view.shape == z.shape and (_padded(view.detach()).data_ptr() != view.data_ptr()) == copied, name
        dec.rel.grad = None
        out = dec(view, sd, rd, od)
        out.backward(gd)
        assert leaf.grad.shape == leaf.shape and dec.rel.grad.shape == rel.shape
        outside = torch.ones_like(leaf, dtype=torch.bool)
        region(outside).fill_(False)
        assert not bool(leaf.grad[outside].any()), f"{name}: a gradient outside the view"
        counts = ranks(view.detach(), dec, sd[:70], rd[:70], od[:70])
        results[name] = (out.detach().clone(), region(leaf.grad).clone(), dec.rel.grad.clone(), counts)
    dec.check()
    ref = results["contiguous"]
    for name, got in results.items():
        assert torch.equal(got[0], ref[0]), f"{name}: scores"
        assert torch.equal(got[1], ref[1]), f"{name}: z.grad"
        assert torch.equal(got[2], ref[2]), f"{name}: rel.grad"
        assert torch.equal(got[3][0], ref[3][0]) and torch.equal(got[3][1], ref[3][1]), f"{name}: rank counts"
    sc, cond, _ = R.score(z, rel, s, r, o)
    assert_close(ref[0].cpu().numpy(), sc, cond, f"DistMult forward width {width}")
    ref_dz, ref_drel = R.backward(z, rel, s, r, o, g)
    c_dz, c_drel = R.backward_cond(z, rel, s, r, o, g)
    assert_close(ref[1].cpu().numpy(), ref_dz, c_dz, f"DistMult dz width {width}")
    assert_close(ref[2].cpu().numpy(), ref_drel, c_drel, f"DistMult drel width {width}")
    # the counts on random inputs: inside the float64 band, and the same for every layout (above)
    lo, hi = R.rank_band(z.numpy(), rel.numpy(), s[:70].numpy(), r[:70].numpy(), o[:70].numpy())
    assert ((_np(ref[3][0]) >= lo) & (_np(ref[3][0]) <= hi)).all()
