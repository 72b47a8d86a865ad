"""Link prediction on rows of up to 512 columns (csrc/rgcn_linkpred_wide.hip) where tests/test_gpu_linkpred_wide.py
stops: rgcn_lpw_* at the C ABI below 129 columns (the module routes those widths to the narrow kernels, the header does not), the
ranking pass's own copy of the filter-list, target and count code on entries and pointers out of range and on non-finite scores, its
three workgroup shapes at the remaining widths, relations of exactly a chunk and of kChunkWaves +- 1 triples at the widths' ends,
``lpw_chunk_ptr_kernel`` with up to 65,536 relations, the exact backward workspace, four distinct strides and bases, and the layouts
``linkpred._padded`` has to copy.  Conventions and helpers are those of tests/test_gpu_linkpred.py, tests/test_gpu_linkpred_wide.py
and tests/test_gpu_linkpred_edges.py."""
import numpy as np
import pytest
import torch

from oracle.tolerance import assert_close
from tests import linkpred_reference as R
from tests import test_gpu_linkpred as T
from tests import test_gpu_linkpred_edges as E
from tests import test_gpu_linkpred_wide as W

pytestmark = pytest.mark.gpu

SENT, DEV, NAN, INF = T.SENT, T.DEV, float("nan"), float("inf")
SHAPES = (0, 32, 64)         # wg_queries: the library's choice, 32 and 64 query rows per workgroup
_np = E._np


def _lib():
    return T._lib()


def _backward(z, rel, s, r, o, g, ix, dz, drel, workspace=None):
    """rgcn_lpw_backward into the caller's views, with the caller's workspace"""
    c = _lib().load()
    if workspace is None:
        workspace = torch.empty(max(c.rgcn_lpw_backward_workspace_bytes(len(s), rel.shape[0], rel.shape[1]), 1), dtype=torch.uint8, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    st = c.rgcn_lpw_backward(z.data_ptr(), z.stride(0), rel.data_ptr(), rel.stride(0), rel.shape[1], z.shape[0], rel.shape[0],
                             s.data_ptr(), r.data_ptr(), o.data_ptr(), len(s), g.data_ptr(), p(ix.node_ptr), p(ix.node_slot),
                             p(ix.rel_ptr), p(ix.rel_triple), p(dz), 0 if dz is None else dz.stride(0), p(drel),
                             0 if drel is None else drel.stride(0), workspace.data_ptr(), workspace.numel(),
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


def _plus_zero(rows):
    return bool((rows == 0).all()) and not bool(torch.signbit(rows).any())


def _rank_raw(z, rel, a, r, e, fptr, fidx, flen, wg_queries=0):
    """rgcn_lpw_rank at the C ABI, with filter_ptr / filter_len as they are (the binding passes the length of filter_idx)"""
    c = _lib().load()
    nq = len(a)
    greater, equal = (torch.full((nq + 1,), -7, dtype=torch.int64, device=DEV) for _ in range(2))
    ws = torch.empty(c.rgcn_lpw_rank_workspace_bytes(nq, z.shape[0], z.shape[1]), dtype=torch.uint8, device=DEV)
    st = c.rgcn_lpw_rank(z.data_ptr(), z.stride(0), rel.data_ptr(), rel.stride(0), z.shape[1], z.shape[0], rel.shape[0], a.data_ptr(),
                         r.data_ptr(), e.data_ptr(), nq, fptr.data_ptr(), fidx.data_ptr(), flen, greater.data_ptr(), equal.data_ptr(),
                         wg_queries, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0 and int(greater[nq]) == -7 and int(equal[nq]) == -7
    return _np(greater[:nq]), _np(equal[:nq])


# ---- 1. ranks at the C ABI: widths below 129 and between the first tests', every workgroup shape ----------------------------------
def _exact_case(n_nodes, n_q, width, seed):
    """entries in [-3, 3], relations in [-1, 1]: every score is an exact integer in fp32 (at most 511 * 9)"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randint(-3, 4, (n_nodes, width), generator=g).float()
    rel = torch.randint(-1, 2, (3, width), generator=g).float()
    a, e = (torch.randint(0, n_nodes, (n_q,), generator=g) for _ in range(2))
    return z, rel, a, torch.randint(0, 3, (n_q,), generator=g), e, g


def _reference_counts(z, rel, a, r, e, lists):
    sc, _ = R.rank_scores(z, rel, a, r)
    assert np.abs(sc).max() < 2 ** 24 and (sc == np.round(sc)).all()
    return R.rank_counts(sc, np.asarray(e), lists)


def _rank_equals(z, rel, a, r, e, lists, what):
    """the three workgroup shapes give the reference's counts (so the same counts)"""
    fptr, fidx = T._csr(lists) if lists is not None else (None, None)
    ref_g, ref_e = _reference_counts(z, rel, a, r, e, lists)
    for wg in SHAPES:
        got_g, got_e = _lib().lpw_rank(T._input(z), T._input(rel), T._ids(a), T._ids(r), T._ids(e), fptr, fidx, wg_queries=wg)
        assert np.array_equal(_np(got_g), ref_g), (what, wg, np.flatnonzero(_np(got_g) != ref_g)[:10])
        assert np.array_equal(_np(got_e), ref_e), (what, wg, np.flatnonzero(_np(got_e) != ref_e)[:10])
    return ref_g, ref_e


# k16 = 1 with one column, 2 (a ragged step in a ragged slab), 8 (exactly a slab), 24 (exactly three), 25 (a fourth slab of one ragged
# step), 32 (the last piece of the last slab holds three columns)
@pytest.mark.parametrize("width", [1, 20, 128, 384, 388, 511])
@pytest.mark.parametrize("filtered", [False, True])
def test_rank_counts_at_the_remaining_widths(width, filtered):
    for n_nodes in (33, 130):
        z, rel, a, r, e, g = _exact_case(n_nodes, 70, width, seed=width + n_nodes)
        lists = T._lists(n_nodes, 70, e, g) if filtered else None
        ref_g, ref_e = _rank_equals(z, rel, a, r, e, lists, f"width {width} N {n_nodes}")
        assert ref_g.sum() > 0 and ref_e.sum() > 0


# ---- 2. filter entries and pointers out of range, width 260 ----------------------------------------------------------------------
def test_rank_filter_entries_out_of_range_count_nothing():
    """lists with entries < 0, >= N and equal to the target, with nothing in range, and of 78 entries (five tiles of sixteen)"""
    n_nodes, n_q = 50, 20
    z, rel, a, r, e, g = _exact_case(n_nodes, n_q, 260, seed=77)
    lists = []
    for i in range(n_q):
        ids = torch.randperm(n_nodes, generator=g)[:45].tolist()
        if i % 4 == 0:
            ids = [-1, ids[0], n_nodes, ids[1], 2 ** 40, int(e[i]), ids[2], -2 ** 40, n_nodes + 15]
        elif i % 4 == 1:
            ids = [n_nodes, -1, 2 ** 40, 2 ** 31, -50]                 # nothing in range
        elif i % 4 == 2:
            ids = list(range(n_nodes, n_nodes + 20)) + ids[:40] + [int(e[i]), 2 ** 62] + list(range(-10, 0)) + ids[40:] + [int(e[i])]
            assert len(ids) == 78 and any(0 <= v < n_nodes for v in ids[64:])
        else:
            ids = ids[:6]
        lists.append(ids)
    ref_g, ref_e = _rank_equals(z, rel, a, r, e, lists, "filter entries out of range")
    clean = [sorted({v for v in ids if 0 <= v < n_nodes}) for ids in lists]
    g2, e2 = _reference_counts(z, rel, a, r, e, clean)
    assert np.array_equal(ref_g, g2) and np.array_equal(ref_e, e2)
    raw_g, raw_e = _reference_counts(z, rel, a, r, e, None)
    assert (raw_g[1::4] == ref_g[1::4]).all() and (raw_e[1::4] == ref_e[1::4]).all() and (raw_g != ref_g).any()


def test_rank_filter_ptr_is_clamped_to_the_filter():
    z, rel, a, r, e, g = _exact_case(50, 20, 260, seed=78)
    lists = [torch.randperm(50, generator=g)[:5].tolist() for _ in range(20)]
    ptr = np.zeros(21, dtype=np.int64)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    idx = np.array([v for x in lists for v in x], dtype=np.int64)
    zd, rd, ad, rdd, ed = T._input(z), T._input(rel), T._ids(a), T._ids(r), T._ids(e)

    def clamped(ptr, flen):
        p = np.clip(ptr, 0, flen)
        return [idx[p[i]:p[i + 1]].tolist() for i in range(20)]

    whole = _reference_counts(z, rel, a, r, e, lists)
    for what, p, flen in (("ptr[0] < 0", np.concatenate([[-3], ptr[1:]]), len(idx)),
                          ("ptr[0] far below 0", np.concatenate([[-2 ** 40], ptr[1:]]), len(idx)),
                          ("ptr[Q] > filter_len", ptr, len(idx) - 7),          # cuts list 18 short, leaves list 19 empty
                          ("both", np.concatenate([[-1], ptr[1:]]), len(idx) - 2)):
        ref_g, ref_e = _reference_counts(z, rel, a, r, e, clamped(p, flen))
        for wg in SHAPES:
            got_g, got_e = _rank_raw(zd, rd, ad, rdd, ed, T._ids(p), T._ids(idx), flen, wg)
            assert np.array_equal(got_g, ref_g) and np.array_equal(got_e, ref_e), (what, wg)
        if flen == len(idx):
            assert np.array_equal(ref_g, whole[0]) and np.array_equal(ref_e, whole[1])
    assert clamped(ptr, len(idx) - 7)[19] == [] and len(clamped(ptr, len(idx) - 7)[18]) == 3
    # no entries, a filter_ptr of zeros: the raw ranks
    raw = _reference_counts(z, rel, a, r, e, None)
    assert (raw[0] != whole[0]).any()
    got_g, got_e = _rank_raw(zd, rd, ad, rdd, ed, torch.zeros(21, dtype=torch.int64, device=DEV), T._ids(idx), 0)
    assert np.array_equal(got_g, raw[0]) and np.array_equal(got_e, raw[1])


# ---- 3. non-finite scores ----------------------------------------------------------------------------------------------------------
def test_rank_non_finite_scores():
    """width 260: integer-valued z with one +inf (row 5, column 130: the second slab) and one NaN (row 7, column 257: the last, ragged
    step of the third); queries whose target is the NaN row (0), the +inf row (1), whose anchor holds the +inf (2) and with an id out
    of range (3, 4, 5).  A score's class -- finite, an infinity, NaN -- follows from its terms z[a, k] rel[r, k] z[e, k] whatever
    the order of the sum (NaN if a term is NaN or terms of both infinities meet, else the infinity that occurs), which is asserted on
    the reference; so the counts are numpy's."""
    n_nodes, width, inf_row, nan_row = 40, 260, 5, 7
    z, rel, a, r, e, g = _exact_case(n_nodes, 24, width, seed=21)
    rel[:, 130] = torch.tensor([1., -1., 1.])
    z[:, 130] = torch.tensor([1., -2., 0., 2.]).repeat(10)        # rows 2, 6, 10, ..: a zero where the +inf sits
    z[inf_row, 130], z[nan_row, 257] = INF, NAN
    a[(a == nan_row) | (a == inf_row)] = 9
    e[0], e[1], a[2], r[2], e[2] = nan_row, inf_row, inf_row, 0, 3
    a[3], r[4], e[5] = n_nodes, 3, -1
    ok = np.ones(24, dtype=bool)
    ok[3:6] = False
    ac, rc, ec = a.clamp(0, n_nodes - 1), r.clamp(0, 2), e.clamp(0, n_nodes - 1)
    with np.errstate(invalid="ignore"):
        sc, _ = R.rank_scores(z, rel, ac, rc)
        terms = (z.double().numpy()[ac.numpy()] * rel.double().numpy()[rc.numpy()])[:, None, :] * z.double().numpy()[None]
    nan = np.isnan(terms).any(-1) | (np.isposinf(terms).any(-1) & np.isneginf(terms).any(-1))
    assert np.array_equal(np.isnan(sc), nan) and np.array_equal(np.isposinf(sc), ~nan & np.isposinf(terms).any(-1))
    assert np.array_equal(np.isneginf(sc), ~nan & np.isneginf(terms).any(-1))
    assert np.isnan(sc[ok]).any() and np.isposinf(sc[ok]).any() and np.isneginf(sc[ok]).any()
    assert np.isnan(sc[0, nan_row]) and np.isinf(sc[1, inf_row]) and np.isnan(sc[2, 2]) and np.isinf(sc[2, 0])
    ref_g, ref_e = R.rank_counts(sc, ec.numpy())
    assert ref_g[0] == 0 and ref_e[0] == 0                         # a NaN target: nothing is greater, nothing equal
    lists = T._lists(n_nodes, 24, ec, g)
    fil_g, fil_e = R.rank_counts(sc, ec.numpy(), lists)
    for counts in (ref_g, ref_e, fil_g, fil_e):
        counts[~ok] = -1
    zd, rd = T._input(z), T._input(rel)
    for wg in SHAPES:
        got = _lib().lpw_rank(zd, rd, T._ids(a), T._ids(r), T._ids(e), wg_queries=wg)
        assert np.array_equal(_np(got[0]), ref_g), (wg, _np(got[0]), ref_g)
        assert np.array_equal(_np(got[1]), ref_e), (wg, _np(got[1]), ref_e)
        got = _lib().lpw_rank(zd, rd, T._ids(a), T._ids(r), T._ids(e), *T._csr(lists), wg_queries=wg)
        assert np.array_equal(_np(got[0]), fil_g), (wg, _np(got[0]), fil_g)
        assert np.array_equal(_np(got[1]), fil_e), (wg, _np(got[1]), fil_e)


# ---- 4. random inputs at width 388 ---------------------------------------------------------------------------------------------------
# tests/test_gpu_linkpred_edges._pick_random_rank_case(388), on the CPU: seed 0, 0 of 128 bands open
def test_rank_random_inputs_copies_and_bands_at_width_388():
    (z, rel, a, r, e, lists), lo, hi, open_, seed = E._pick_random_rank_case(388)
    n_q = len(e)
    assert open_ <= 0.02 * n_q
    copies = [T._copies(z, e, i) for i in range(n_q)]
    want_equal = np.array([len([v for v in copies[i] if v != int(e[i]) and v not in set(lists[i])]) for i in range(n_q)])
    assert want_equal[:20].sum() >= 10 and want_equal[:20].sum() < sum(len(c) - 1 for c in copies[:20])
    lo_r, hi_r = R.rank_band(z.numpy(), rel.numpy(), a.numpy(), r.numpy(), e.numpy(), copies)
    args = (T._input(z), T._input(rel), T._ids(a), T._ids(r), T._ids(e))
    for wg in SHAPES:
        got_g, got_e = (_np(t) for t in _lib().lpw_rank(*args, *T._csr(lists), wg_queries=wg))
        print(f"rank random width 388 wg {wg}: seed {seed}, open bands {open_}/{n_q}, equal counted {got_e.sum()} (expected "
              f"{want_equal.sum()}), greater outside its band in {int(((got_g < lo) | (got_g > hi)).sum())} queries")
        assert np.array_equal(got_e, want_equal)
        assert ((got_g >= lo) & (got_g <= hi)).all()
        raw_g, raw_e = (_np(t) for t in _lib().lpw_rank(*args, wg_queries=wg))
        assert ((raw_g >= lo_r) & (raw_g <= hi_r)).all() and (raw_g >= got_g).all() and (raw_e >= got_e).all()
        assert np.array_equal(raw_e, [len(c) - 1 for c in copies])


# ---- 5. score and backward: chunk edges, many relations, widths below 129 --------------------------------------------------------------
WAVES = W.WAVES
CHUNK_COUNTS = (0, 1, 255, 256, 257, 513, WAVES - 1, WAVES, WAVES + 1, 0)


# the first wide width (a second piece for lane 0 only), exactly two slabs, every lane two pieces
@pytest.mark.parametrize("width", [129, 256, 512])
def test_score_and_backward_with_relations_of_exactly_a_chunk(width):
    """40 nodes: node 0 in two triples of three, node 39 in none; relations of exactly CHUNK_COUNTS triples"""
    gen = torch.Generator().manual_seed(4)
    n_nodes, n_rel, n = 40, len(CHUNK_COUNTS), sum(CHUNK_COUNTS)
    z, rel = torch.randn(n_nodes, width, generator=gen), torch.randn(n_rel, width, generator=gen)
    s, o = (torch.randint(1, n_nodes - 1, (n,), generator=gen) for _ in range(2))
    s[::3], o[1::3] = 0, 0
    r = torch.repeat_interleave(torch.arange(n_rel), torch.tensor(CHUNK_COUNTS))[torch.randperm(n, generator=gen)]
    assert tuple(torch.bincount(r, minlength=n_rel).tolist()) == CHUNK_COUNTS
    assert int(((s == 0) | (o == 0)).sum()) > n // 2 and not bool(((s == 39) | (o == 39)).any())
    (dz, drel), _ = W._check_case(z, rel, s, r, o, torch.randn(n, generator=gen), f"chunk edges width {width}")
    for row in (drel[0], drel[9], dz[39]):                    # no triple: +0 over the sentinels
        assert _plus_zero(row)
    assert bool((drel[1] != 0).any()) and bool((dz[0] != 0).any())


@pytest.mark.parametrize("n_rel", [257, 1000, 65536])
def test_drel_with_many_relations(n_rel):
    """lpw_chunk_ptr_kernel with 2, 4 and 256 relations per thread; most relations empty, three with more than one chunk"""
    g = torch.Generator().manual_seed(n_rel)
    n_nodes, n, width = 50, 4000, 132
    z, rel = torch.randn(n_nodes, width, generator=g), torch.randn(n_rel, width, generator=g)
    s, o = (torch.randint(0, n_nodes, (n,), generator=g) for _ in range(2))
    some = torch.randperm(n_rel - 2, generator=g)[:21] + 1            # distinct, neither 0 nor R - 1
    r = some[1:][torch.randint(0, 20, (n,), generator=g)]
    r[:300], r[300:900], r[900:1600] = 0, n_rel - 1, some[0]
    r = r[torch.randperm(n, generator=g)]
    count = torch.bincount(r, minlength=n_rel)
    assert int(count[0]) == 300 and int(count[n_rel - 1]) == 600 and int((count > 256).sum()) == 3
    assert int((count == 0).sum()) == n_rel - 23
    (dz, drel), _ = W._check_case(z, rel, s, r, o, torch.randn(n, generator=g), f"R {n_rel}")
    assert _plus_zero(drel[(count == 0).to(DEV)])


# the module never sends these widths to rgcn_lpw_*; include/rgcn_mi355x.h admits them
@pytest.mark.parametrize("width", [1, 20, 128])
def test_score_and_backward_below_129_columns(width):
    for n_triples in (1, 65, 1000):
        z, rel, s, r, o, g = T._random_case(50, 5, width, n_triples, seed=width * 7 + n_triples)
        W._check_case(z, rel, s, r, o, g, f"width {width} T {n_triples}")


def test_backward_workspace_of_exactly_the_stated_bytes():
    """every relation non-empty and 257 triples each: 2 chunks per relation = T / 256 + R, the most the workspace is sized for"""
    lib = _lib()
    n_rel, width, guard = 5, 260, 4096
    n = 257 * n_rel
    g = torch.Generator().manual_seed(12)
    z, rel = torch.randn(30, width, generator=g), torch.randn(n_rel, width, generator=g)
    s, o = (torch.randint(0, 30, (n,), generator=g) for _ in range(2))
    r = torch.arange(n_rel).repeat_interleave(257)[torch.randperm(n, generator=g)]
    gr = torch.randn(n, generator=g)
    assert n % 256 != 0 and n // 256 + n_rel == 2 * n_rel
    zd, rd, sd, rdd, od, gd = T._input(z), T._input(rel), T._ids(s), T._ids(r), T._ids(o), gr.to(DEV)
    ix = lib.lp_index_build(sd, rdd, od, 30, n_rel)
    need = lib.load().rgcn_lpw_backward_workspace_bytes(n, n_rel, width)
    assert need >= 4 * (n_rel + 1) + 2 * n_rel * width * 4
    buf = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    (zbuf, dz), (rbuf, drel) = T._output(30, width), T._output(n_rel, width)
    assert _backward(zd, rd, sd, rdd, od, gd, ix, dz, drel, workspace=buf[:need]) == 0
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
    assert _backward(zd, rd, sd, rdd, od, gd, ix, dz, drel, workspace=buf[:need - 1]) == -6
    assert bool((buf == 0xA5).all()) and bool((zbuf == SENT).all()) and bool((rbuf == SENT).all())


# ---- 6. strides and bases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,lds", [(129, (140, 148, 144, 152)), (260, (272, 280, 276, 288))])
def test_four_distinct_strides_and_bases_inside_larger_buffers(width, lds):
    lib = _lib()
    ldz, ldr, lddz, lddrel = lds
    w4 = T._ld(width)
    z, rel, s, r, o, g = T._random_case(50, 5, width, 1000, seed=31 + width)
    s[7], r[9] = 50, -1
    sd, rdd, od, gd = T._ids(s), T._ids(r), T._ids(o), g.to(DEV)
    # the default layout
    zd, rd = T._input(z), T._input(rel)
    ix = lib.lp_index_build(sd, rdd, od, 50, 5)
    score = lib.lpw_score(zd, rd, sd, rdd, od)
    (_, dz), (_, drel) = T._output(50, width), T._output(5, width)
    assert _backward(zd, rd, sd, rdd, od, gd, ix, dz, drel) == 0
    gq = torch.Generator().manual_seed(width)
    a, e, rq = torch.randint(0, 50, (70,), generator=gq), torch.randint(0, 50, (70,), generator=gq), torch.randint(0, 5, (70,), generator=gq)
    fptr, fidx = T._csr(T._lists(50, 70, e, gq))
    rank = {wg: lib.lpw_rank(zd, rd, T._ids(a), T._ids(rq), T._ids(e), fptr, fidx, wg_queries=wg) for wg in SHAPES}
    # the same data behind other strides and bases
    (zb, zv), (rb, rv) = E._inside(z, ldz, NAN), E._inside(rel, ldr, NAN)
    (dzb, dzv), (drb, drv) = E._inside((50, width), lddz, SENT), E._inside((5, width), lddrel, SENT)
    assert len({zv.stride(0), rv.stride(0), dzv.stride(0), drv.stride(0), w4}) == 5
    zb0, rb0 = zb.clone(), rb.clone()
    assert torch.equal(lib.lpw_score(zv, rv, sd, rdd, od), score)
    assert _backward(zv, rv, sd, rdd, od, gd, ix, dzv, drv) == 0
    assert torch.equal(dzv, dz) and torch.equal(drv, drel)
    for wg in SHAPES:
        got = lib.lpw_rank(zv, rv, T._ids(a), T._ids(rq), T._ids(e), fptr, fidx, wg_queries=wg)
        assert torch.equal(got[0], rank[wg][0]) and torch.equal(got[1], rank[wg][1]), wg
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
    sc, cond, _ = R.score(z, rel, s, r, o)
    assert_close(score.cpu().numpy(), sc, cond, f"score width {width}")


# ---- 7. the Python layer -----------------------------------------------------------------------------------------------------------
def test_distmult_wide_on_layouts_that_have_to_be_copied():
    from scaling_rgcn_training_amd.linkpred import WIDE_MAX_WIDTH, DistMult, _padded, ranks
    width = 260
    z, rel, s, r, o, g = T._random_case(50, 5, width, 300, seed=40 + width)
    sd, rd, od, gd = T._ids(s), T._ids(r), T._ids(o), g.to(DEV)
    dec = DistMult(5, width, wide=True).to(DEV)
    assert dec.family == "lpw"
    with torch.no_grad():
        dec.rel.copy_(rel)
    results = {}
    for name, leaf, view, region, copied in E._layouts(z):
        assert view.shape == z.shape and (_padded(view.detach(), WIDE_MAX_WIDTH).data_ptr() != view.data_ptr()) == copied, name
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
    assert_close(ref[0].cpu().numpy(), sc, cond, "DistMult wide forward")
    ref_dz, ref_drel = R.backward(z, rel, s, r, o, g)
    c_dz, c_drel = R.backward_cond(z, rel, s, r, o, g)
    assert_close(ref[1].cpu().numpy(), ref_dz, c_dz, "DistMult wide dz")
    assert_close(ref[2].cpu().numpy(), ref_drel, c_drel, "DistMult wide drel")
    # the counts on random inputs: inside the float64 band, and the same for every layout (above)
    lo, hi = R.rank_band(z.numpy(), rel.numpy(), s[:70].numpy(), r[:70].numpy(), o[:70].numpy())
    assert ((_np(ref[3][0]) >= lo) & (_np(ref[3][0]) <= hi)).all()
