"""The ComplEx and TransE kernels (csrc/rgcn_kge.hip) where tests/test_gpu_kge.py stops: the ranking widths between
its four (every ``k16``, a ragged last piece in a slab, ComplEx's padded-width ladder), TransE's own filter-list, target and count
code on entries and pointers out of range and on non-finite scores, random inputs at the remaining widths, relations of exactly a
chunk at lane groups that leave idle lanes, 65,536 relations, the exact backward workspace, four distinct strides and bases, and the
layouts ``linkpred._padded`` has to copy.  The conventions and helpers are those of tests/test_gpu_linkpred.py, tests/test_gpu_kge.py
and tests/test_gpu_linkpred_edges.py: NaN in the inputs' pad columns, sentinels and a guard row around every output, float results under
``oracle.tolerance.assert_close`` with the sums on absolute values as ``cond``, everything integer EQUAL to the reference."""
import numpy as np
import pytest
import torch

from oracle.tolerance import assert_close
from tests import kge_reference as K
from tests import linkpred_reference as R
from tests import test_gpu_kge as KG
from tests import test_gpu_linkpred as T
from tests import test_gpu_linkpred_edges as E

pytestmark = pytest.mark.gpu

SENT, DEV, NAN, INF = T.SENT, T.DEV, float("nan"), float("inf")
CODE, DECS = KG.CODE, KG.DECS
SIDES = [(0, "object"), (1, "subject")]
_np = E._np


def _lib():
    return T._lib()


def _backward(dec, z, rel, s, r, o, g, ix, dz, drel, workspace=None):
    """rgcn_kge_backward into the caller's views, with the caller's workspace (tests/test_gpu_kge._backward_raw allocates its own)"""
    c = _lib().load()
    if workspace is None:
        workspace = torch.empty(max(c.rgcn_kge_backward_workspace_bytes(CODE[dec], len(s), rel.shape[0], rel.shape[1]), 1), dtype=torch.uint8,
                                device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    st = c.rgcn_kge_backward(CODE[dec], z.data_ptr(), z.stride(0), rel.data_ptr(), rel.stride(0), rel.shape[1], z.shape[0], rel.shape[0],
                             s.data_ptr(), r.data_ptr(), o.data_ptr(), len(s), g.data_ptr(), p(ix.node_ptr), p(ix.node_slot), p(ix.rel_ptr),
                             p(ix.rel_triple), p(dz), 0 if dz is None else dz.stride(0), p(drel), 0 if drel is None else drel.stride(0),
                             workspace.data_ptr(), workspace.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


def _gradients(dec, z, rel, s, r, o, g):
    """(dz, drel) on the device over sentinels, the default layout"""
    zd, rd, sd, rdd, od, gd = T._input(z), T._input(rel), T._ids(s), T._ids(r), T._ids(o), g.to(DEV)
    ix = _lib().lp_index_build(sd, rdd, od, z.shape[0], rel.shape[0])
    (_, dz), (_, drel) = T._output(*z.shape), T._output(*rel.shape)
    assert _backward(dec, zd, rd, sd, rdd, od, gd, ix, dz, drel) == 0
    return dz, drel


def _plus_zero(rows):
    return bool((rows == 0).all()) and not bool(torch.signbit(rows).any())


def _rank_raw(dec, code, z, rel, a, r, e, fptr, fidx, flen):
    """rgcn_kge_rank at the C ABI, with filter_ptr / filter_len as they are (the binding passes the length of filter_idx)"""
    c = _lib().load()
    nq = len(a)
    greater, equal = (torch.full((nq + 1,), -7, dtype=torch.int64, device=DEV) for _ in range(2))
    ws = torch.empty(c.rgcn_kge_rank_workspace_bytes(CODE[dec], nq, z.shape[0], z.shape[1]), dtype=torch.uint8, device=DEV)
    st = c.rgcn_kge_rank(CODE[dec], code, z.data_ptr(), z.stride(0), rel.data_ptr(), rel.stride(0), z.shape[1], z.shape[0], rel.shape[0],
                         a.data_ptr(), r.data_ptr(), e.data_ptr(), nq, fptr.data_ptr(), fidx.data_ptr(), flen, greater.data_ptr(),
                         equal.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0 and int(greater[nq]) == -7 and int(equal[nq]) == -7
    return _np(greater[:nq]), _np(equal[:nq])


# ---- 1. ranks: the remaining widths ------------------------------------------------------------------------------------------
def _exact_case(n_nodes, n_q, width, seed):
    """entries in [-3, 3], relations in [-1, 1]: every score of either decoder is an exact integer in fp32"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randint(-3, 4, (n_nodes, width), generator=g).float()
    rel = torch.randint(-1, 2, (3, width), generator=g).float()
    a, e = (torch.randint(0, n_nodes, (n_q,), generator=g) for _ in range(2))
    return z, rel, a, torch.randint(0, 3, (n_q,), generator=g), e, g


def _rank_equals(dec, code, side, z, rel, a, r, e, lists, what):
    fptr, fidx = T._csr(lists) if lists is not None else (None, None)
    got = _lib().kge_rank(CODE[dec], code, T._input(z), T._input(rel), T._ids(a), T._ids(r), T._ids(e), fptr, fidx)
    ref = KG._reference_counts(dec, z, rel, a, r, e, side, lists)        # (asserts |score| < 2^24 and integrality)
    for name, x, y in zip(("greater", "equal"), got, ref):
        assert np.array_equal(_np(x), y), (what, side, name, np.flatnonzero(_np(x) != y)[:10])
    return ref


# TransE: k16 = 1 (2, 5, 15, 16), 2 (18, 31), 3 (33, 48), 4 (49), 7 (100), 8 (127), with a last piece of 1, 2, 3 and 4 columns and a
# last slab of 1..4 pieces.  ComplEx: padded widths 16 (4, 14, 16), 32 (18, 30, 32), 64 (34, 62), 128 (66, 100, 126).
RANK_WIDTHS = [("transe", w) for w in (2, 5, 15, 16, 18, 31, 33, 48, 49, 100, 127)] + \
              [("complex", w) for w in (4, 14, 16, 18, 30, 32, 34, 62, 66, 100, 126)]


@pytest.mark.parametrize("dec,width", RANK_WIDTHS)
@pytest.mark.parametrize("filtered", [False, True])
def test_rank_counts_at_the_remaining_widths(dec, width, filtered):
    for n_nodes in (33, 130):
        z, rel, a, r, e, g = _exact_case(n_nodes, 70, width, seed=width + n_nodes)
        lists = T._lists(n_nodes, 70, e, g) if filtered else None
        refs = [_rank_equals(dec, code, side, z, rel, a, r, e, lists, f"{dec} width {width} N {n_nodes}") for code, side in SIDES]
        assert not np.array_equal(refs[0][0], refs[1][0])                     # the sides differ: a mix-up fails
        assert refs[0][0].sum() > 0 and refs[0][1].sum() + refs[1][1].sum() > 0


# ---- 2. filter entries and pointers out of range -------------------------------------------------------------------------------
def _filter_edge_case():
    """50 nodes, 20 queries; lists with entries < 0, >= N and equal to the target, lists with nothing in range, and lists of 78
    entries whose ids in range lie on both sides of entry 64 (TransE takes 64 entries a step, lp_rank_body 16)"""
    n_nodes, n_q = 50, 20
    z, rel, a, r, e, g = _exact_case(n_nodes, n_q, 20, seed=77)
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
    return z, rel, a, r, e, lists


@pytest.mark.parametrize("dec", DECS)
@pytest.mark.parametrize("code,side", SIDES)
def test_rank_filter_entries_out_of_range_count_nothing(dec, code, side):
    z, rel, a, r, e, lists = _filter_edge_case()
    ref_g, ref_e = _rank_equals(dec, code, side, z, rel, a, r, e, lists, "filter entries out of range")
    # the same counts as with those entries taken out
    clean = [sorted({v for v in ids if 0 <= v < 50}) for ids in lists]
    g2, e2 = KG._reference_counts(dec, z, rel, a, r, e, side, clean)
    assert np.array_equal(ref_g, g2) and np.array_equal(ref_e, e2)
    raw_g, raw_e = KG._reference_counts(dec, z, rel, a, r, e, side, None)
    assert (raw_g[1::4] == ref_g[1::4]).all() and (raw_e[1::4] == ref_e[1::4]).all() and (raw_g != ref_g).any()


@pytest.mark.parametrize("dec", DECS)
@pytest.mark.parametrize("code,side", SIDES)
def test_rank_filter_ptr_is_clamped_to_the_filter(dec, code, side):
    z, rel, a, r, e, g = _exact_case(50, 20, 20, seed=78)
    lists = [torch.randperm(50, generator=g)[:5].tolist() for _ in range(20)]
    ptr = np.zeros(21, dtype=np.int64)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    idx = np.array([v for x in lists for v in x], dtype=np.int64)
    zd, rd, ad, rdd, ed = T._input(z), T._input(rel), T._ids(a), T._ids(r), T._ids(e)

    def clamped(ptr, flen):
        p = np.clip(ptr, 0, flen)
        return [idx[p[i]:p[i + 1]].tolist() for i in range(20)]

    whole = KG._reference_counts(dec, z, rel, a, r, e, side, lists)
    for what, p, flen in (("ptr[0] < 0", np.concatenate([[-3], ptr[1:]]), len(idx)),
                          ("ptr[0] far below 0", np.concatenate([[-2 ** 40], ptr[1:]]), len(idx)),
                          ("ptr[Q] > filter_len", ptr, len(idx) - 7),          # cuts list 18 short, leaves list 19 empty
                          ("both", np.concatenate([[-1], ptr[1:]]), len(idx) - 2)):
        ref_g, ref_e = KG._reference_counts(dec, z, rel, a, r, e, side, clamped(p, flen))
        got_g, got_e = _rank_raw(dec, code, zd, rd, ad, rdd, ed, T._ids(p), T._ids(idx), flen)
        assert np.array_equal(got_g, ref_g) and np.array_equal(got_e, ref_e), what
        if flen == len(idx):
            assert np.array_equal(ref_g, whole[0]) and np.array_equal(ref_e, whole[1])
    assert clamped(ptr, len(idx) - 7)[19] == [] and len(clamped(ptr, len(idx) - 7)[18]) == 3
    # no entries, a filter_ptr of zeros: the raw ranks
    raw = KG._reference_counts(dec, z, rel, a, r, e, side, None)
    assert (raw[0] != whole[0]).any()
    zeros = torch.zeros(21, dtype=torch.int64, device=DEV)
    got_g, got_e = _rank_raw(dec, code, zd, rd, ad, rdd, ed, zeros, T._ids(idx), 0)
    assert np.array_equal(got_g, raw[0]) and np.array_equal(got_e, raw[1])


# ---- 3. non-finite scores --------------------------------------------------------------------------------------------------------
def _non_finite_case(dec):
    """integer-valued z with one +inf (row 5, column 2) and one NaN (row 7, column 1); queries whose target is the NaN row (0), the
    +inf row (1), whose anchor holds the +inf (2) and with an id out of range (3, 4, 5)"""
    n_nodes, width, inf_row, nan_row = 40, 8, 5, 7
    z, rel, a, r, e, g = _exact_case(n_nodes, 24, width, seed=21)
    rel[:, 2], rel[:, 3] = torch.tensor([1., -1., 1.]), torch.tensor([-1., 1., 1.])
    z[inf_row, 2], z[nan_row, 1] = INF, NAN
    a[(a == nan_row) | (a == inf_row)] = 9
    e[0], e[1], a[2], e[2] = nan_row, inf_row, inf_row, 3
    a[3], r[4], e[5] = n_nodes, 3, -1
    ok = np.ones(24, dtype=bool)
    ok[3:6] = False
    return z, rel, a, r, e, g, ok


def _term_classes(dec, z, rel, a, r, side):
    """(nan, pinf, ninf) [Q, N]: the class every score has whatever the order of its sum, from its terms in float64 -- NaN if a term
    is NaN or terms of both infinities meet, else the infinity that occurs.  TransE's terms are -|d_k|; ComplEx's (object side) are
    the products q_c o_c of the query row q = s o r with the candidate, column by column, as the ranking pass multiplies them."""
    zn, rn = z.double().numpy(), rel.double().numpy()
    za, rr = zn[a.numpy()][:, None, :], rn[r.numpy()][:, None, :]
    with np.errstate(invalid="ignore"):
        if dec == "transe":
            terms = -np.abs((za + rr) - zn[None]) if side == "object" else -np.abs((zn[None] + rr) - za)
        else:
            terms = K._cmul(za, rr, False, False) * zn[None]
    nan = np.isnan(terms).any(-1) | (np.isposinf(terms).any(-1) & np.isneginf(terms).any(-1))
    return nan, ~nan & np.isposinf(terms).any(-1), ~nan & np.isneginf(terms).any(-1)


# ComplEx is ranked on the object side only here: on the subject side the kernel's query row is conj(r) o o, which regroups the
# float64 restatement's (s o r) . o -- with an infinite part the two meet inf - inf in different places (inside the complex product
# in one, between two terms of the sum in the other), so the score's class is no longer a function of the inputs alone.
@pytest.mark.parametrize("dec,code,side", [("transe", 0, "object"), ("transe", 1, "subject"), ("complex", 0, "object")])
def test_rank_non_finite_scores(dec, code, side):
    """+-inf and NaN scores: sums and comparisons on them do not depend on the order of the sum, so the counts are numpy's"""
    z, rel, a, r, e, g, ok = _non_finite_case(dec)
    n_nodes = z.shape[0]
    ac, rc, ec = a.clamp(0, n_nodes - 1), r.clamp(0, 2), e.clamp(0, n_nodes - 1)
    with np.errstate(invalid="ignore"):
        sc, _ = K.rank_scores(dec, z.numpy(), rel.numpy(), ac.numpy(), rc.numpy(), side)
    nan, pinf, ninf = _term_classes(dec, z, rel, ac, rc, side)
    assert np.array_equal(np.isnan(sc), nan) and np.array_equal(np.isposinf(sc), pinf) and np.array_equal(np.isneginf(sc), ninf)
    assert nan[ok].any() and ninf[ok].any() and (dec == "complex") == bool(pinf[ok].any())
    assert np.isnan(sc[0, 7]) and not np.isfinite(sc[1, 5]) and not np.isfinite(sc[2]).any() and np.isfinite(sc[6:]).any()
    ref_g, ref_e = R.rank_counts(sc, ec.numpy())
    assert ref_g[0] == 0 and ref_e[0] == 0                         # a NaN target: nothing is greater, nothing equal
    lists = T._lists(n_nodes, 24, ec, g)
    fil_g, fil_e = R.rank_counts(sc, ec.numpy(), lists)
    for counts in (ref_g, ref_e, fil_g, fil_e):
        counts[~ok] = -1
    zd, rd = T._input(z), T._input(rel)
    got = _lib().kge_rank(CODE[dec], code, zd, rd, T._ids(a), T._ids(r), T._ids(e))
    assert np.array_equal(_np(got[0]), ref_g), (_np(got[0]), ref_g)
    assert np.array_equal(_np(got[1]), ref_e), (_np(got[1]), ref_e)
    got = _lib().kge_rank(CODE[dec], code, zd, rd, T._ids(a), T._ids(r), T._ids(e), *T._csr(lists))
    assert np.array_equal(_np(got[0]), fil_g), (_np(got[0]), fil_g)
    assert np.array_equal(_np(got[1]), fil_e), (_np(got[1]), fil_e)


# ---- 4. random inputs at the remaining widths ------------------------------------------------------------------------------------
def _pick_random_rank_case(dec, side, width):
    """tests/test_gpu_linkpred.py's condition on the inputs: the first seed below 20 whose float64 bands, with the bit copies of
    the target taken out of the candidates, are open for at most 2 % of the queries"""
    for seed in range(20):
        z, rel, a, r, e, lists = case = E._random_rank_case(width, seed)
        sc, cond = K.rank_scores(dec, z.numpy(), rel.numpy(), a.numpy(), r.numpy(), side)
        lo, hi = K.rank_band(sc, cond, e.numpy(), [sorted(set(lists[i]) | set(T._copies(z, e, i))) for i in range(len(e))])
        open_ = int((lo != hi).sum())
        if open_ <= 0.02 * len(lo):
            return case, sc, cond, lo, hi, open_, seed
    raise AssertionError("no seed gives at most 2 % open bands")


# Picked on the CPU: seed 0 in all eight cases.  Open bands of 128 queries: transe 17 object 0, subject 0; transe 127 object 0,
# subject 2; complex 18 object 0, subject 0; complex 126 object 0, subject 0.
@pytest.mark.parametrize("dec,width", [("transe", 17), ("transe", 127), ("complex", 18), ("complex", 126)])
@pytest.mark.parametrize("code,side", SIDES)
def test_rank_random_inputs_copies_and_bands_at_the_remaining_widths(dec, width, code, side):
    """N = 300, Q = 128, standard normal, 40 rows copied bit for bit onto other ids: ``equal`` counts exactly the unfiltered copies,
    ``greater`` lies in the float64 band of every query"""
    (z, rel, a, r, e, lists), sc, cond, lo, hi, open_, seed = _pick_random_rank_case(dec, side, width)
    n_q = len(e)
    assert open_ <= 0.02 * n_q
    copies = [T._copies(z, e, i) for i in range(n_q)]
    want_equal = np.array([len([v for v in copies[i] if v != int(e[i]) and v not in set(lists[i])]) for i in range(n_q)])
    assert want_equal[:20].sum() >= 10 and want_equal[:20].sum() < sum(len(c) - 1 for c in copies[:20])
    args = (CODE[dec], code, T._input(z), T._input(rel), T._ids(a), T._ids(r), T._ids(e))
    got_g, got_e = (_np(t) for t in _lib().kge_rank(*args, *T._csr(lists)))
    print(f"kge rank random {dec} {side} width {width}: seed {seed}, open bands {open_}/{n_q}, equal counted {got_e.sum()} (expected "
          f"{want_equal.sum()}), greater outside its band in {int(((got_g < lo) | (got_g > hi)).sum())} queries")
    assert np.array_equal(got_e, want_equal)
    assert ((got_g >= lo) & (got_g <= hi)).all()
    raw_g, raw_e = (_np(t) for t in _lib().kge_rank(*args))
    lo_r, hi_r = K.rank_band(sc, cond, e.numpy(), copies)
    assert ((raw_g >= lo_r) & (raw_g <= hi_r)).all() and (raw_g >= got_g).all() and (raw_e >= got_e).all()
    assert np.array_equal(raw_e, [len(c) - 1 for c in copies])


# ---- 5. score and backward: chunk edges, lane groups with idle lanes, many relations ---------------------------------------------
CHUNK_COUNTS = (0, 1, 255, 256, 257, 513, 0, 70)


def _chunk_case(width, seed=4):
    """40 nodes: node 0 in two triples of three, node 39 in none; relations of exactly CHUNK_COUNTS triples"""
    n_nodes, n_rel, n = 40, len(CHUNK_COUNTS), sum(CHUNK_COUNTS)
    z, rel, s, r, o, g = KG._case(n_nodes, n_rel, width, n, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    s, o = (torch.randint(1, n_nodes - 1, (n,), generator=gen) for _ in range(2))
    s[::3], o[1::3] = 0, 0
    r = torch.repeat_interleave(torch.arange(n_rel), torch.tensor(CHUNK_COUNTS))[torch.randperm(n, generator=gen)]
    assert tuple(torch.bincount(r, minlength=n_rel).tolist()) == CHUNK_COUNTS
    assert int(((s == 0) | (o == 0)).sum()) > n // 2 and not bool(((s == 39) | (o == 39)).any())
    return z, rel, s, r, o, g


# lane groups of G = ceil(width / 4) lanes, 64 / G per wave: 21 at 12 (63 lanes), 9 at 28 (63), 5 at 44 (55), 2 at 100 (50), 2 at
# 126 / 128 (64); relations of 1 triple leave all groups but one idle
@pytest.mark.parametrize("dec,width", [("transe", w) for w in (12, 28, 44, 100, 128)] + [("complex", w) for w in (12, 28, 44, 100, 126)])
def test_score_and_backward_with_relations_of_exactly_a_chunk(dec, width):
    z, rel, s, r, o, g = _chunk_case(width)
    KG._check_case(dec, z, rel, s, r, o, g, f"{dec} chunk edges width {width}")       # (against float64, twice, each gradient alone)
    dz, drel = _gradients(dec, z, rel, s, r, o, g)
    for row in (drel[0], drel[6], dz[39]):                    # no triple: +0 over the sentinels
        assert _plus_zero(row)
    assert bool((drel[1] != 0).any()) and bool((dz[0] != 0).any())


@pytest.mark.parametrize("width", [12, 100])
def test_transe_rows_with_d_zero_give_a_zero_gradient(width):
    """node 0 is the subject of 300 triples (0, k, 30 + k) with z[30 + k] = z[0] + rel[k] in every column, and in no other triple:
    d = 0 throughout, sign(0) = 0, so dz[0], dz[30 + k] and the gradient of relation 5, which has no other triples, are exactly +0
    -- a sign that took 0 for positive or negative would leave sums of +-g there"""
    n_nodes, n_rel = 40, 6
    z, rel, s, r, o, g = KG._case(n_nodes, n_rel, width, 900, seed=9)
    gen = torch.Generator().manual_seed(10)
    s, o = (torch.randint(1, 30, (900,), generator=gen) for _ in range(2))
    r = torch.randint(0, 5, (900,), generator=gen)
    k = torch.arange(300) % n_rel
    s[:300], r[:300], o[:300] = 0, k, 30 + k
    z[30:36] = z[0] + rel
    perm = torch.randperm(900, generator=gen)
    s, r, o = s[perm], r[perm], o[perm]
    hub = s == 0
    assert int(hub.sum()) == 300 and not bool((o == 0).any()) and bool((((z[s] + rel[r]) - z[o])[hub] == 0).all())
    assert float(z.abs().max()) <= 16 and bool((z * 16 == (z * 16).round()).all()) and bool((g[hub] != 0).all())
    ref_dz = KG._check_case("transe", z, rel, s, r, o, g, f"transe d = 0 width {width}")
    assert not ref_dz[0].any() and not ref_dz[30:36].any() and np.abs(ref_dz[1:30]).max() > 1
    dz, drel = _gradients("transe", z, rel, s, r, o, g)
    assert _plus_zero(dz[0]) and _plus_zero(dz[30:36]) and _plus_zero(drel[5]) and bool((drel[:5] != 0).any())


def test_transe_backward_with_65536_relations():
    """lp_chunk_ptr_kernel with 256 relations per thread behind kge_drel_chunk_kernel; most relations empty, three with more than
    one chunk"""
    n_rel, width, n_nodes, n = 65536, 20, 50, 4000
    z, rel, s, r, o, g = KG._case(n_nodes, n_rel, width, n, seed=n_rel + width)
    gen = torch.Generator().manual_seed(5)
    some = torch.randperm(n_rel - 2, generator=gen)[:21] + 1            # distinct, neither 0 nor R - 1
    r = some[1:][torch.randint(0, 20, (n,), generator=gen)]
    r[:300], r[300:900], r[900:1600] = 0, n_rel - 1, some[0]
    r = r[torch.randperm(n, generator=gen)]
    count = torch.bincount(r, minlength=n_rel)
    assert int(count[0]) == 300 and int(count[n_rel - 1]) == 600 and int((count > 256).sum()) == 3
    assert int((count == 0).sum()) == n_rel - 23
    KG._check_case("transe", z, rel, s, r, o, g, f"transe R {n_rel}")
    _, drel = _gradients("transe", z, rel, s, r, o, g)
    assert _plus_zero(drel[(count == 0).to(DEV)])


@pytest.mark.parametrize("dec", DECS)
def test_backward_workspace_of_exactly_the_stated_bytes(dec):
    """every relation non-empty and 257 triples each: 2 chunks per relation = T / 256 + R, the most the workspace is sized for"""
    lib = _lib()
    n_rel, width, guard = 5, 20, 4096
    n = 257 * n_rel
    z, rel, s, r, o, gr = KG._case(30, n_rel, width, n, seed=12)
    r = torch.arange(n_rel).repeat_interleave(257)[torch.randperm(n, generator=torch.Generator().manual_seed(13))]
    assert n % 256 != 0 and n // 256 + n_rel == 2 * n_rel
    zd, rd, sd, rdd, od, gd = T._input(z), T._input(rel), T._ids(s), T._ids(r), T._ids(o), gr.to(DEV)
    ix = lib.lp_index_build(sd, rdd, od, 30, n_rel)
    need = lib.load().rgcn_kge_backward_workspace_bytes(CODE[dec], n, n_rel, width)
    assert need >= 4 * (n_rel + 1) + 2 * n_rel * 20 * 4
    buf = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    (zbuf, dz), (rbuf, drel) = T._output(30, width), T._output(n_rel, width)
    assert _backward(dec, zd, rd, sd, rdd, od, gd, ix, dz, drel, workspace=buf[:need]) == 0
    assert bool((buf[need:] == 0xA5).all()), "the workspace was written behind its stated size"
    ref_dz, ref_drel = K.backward(dec, z, rel, s, r, o, gr)
    c_dz, c_drel = K.backward(dec, z, rel, s, r, o, gr, absolute=True)
    assert_close(dz.cpu().numpy(), ref_dz, c_dz, f"{dec} exact workspace dz")
    assert_close(drel.cpu().numpy(), ref_drel, c_drel, f"{dec} exact workspace drel")
    T._check_output_pads(zbuf, 30, width, "dz")
    T._check_output_pads(rbuf, n_rel, width, "drel")
    # one byte fewer: refused before anything is launched
    buf.fill_(0xA5)
    (zbuf, dz), (rbuf, drel) = T._output(30, width), T._output(n_rel, width)
    assert _backward(dec, zd, rd, sd, rdd, od, gd, ix, dz, drel, workspace=buf[:need - 1]) == -6
    assert bool((buf == 0xA5).all()) and bool((zbuf == SENT).all()) and bool((rbuf == SENT).all())


# ---- 6. strides and bases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dec,width", [("transe", 3), ("transe", 20), ("complex", 2), ("complex", 20)])
def test_four_distinct_strides_and_bases_inside_larger_buffers(dec, width):
    lib, code = _lib(), CODE[dec]
    ldz, ldr, lddz, lddrel = 24, 32, 28, 40
    w4 = T._ld(width)
    z, rel, s, r, o, g = KG._case(50, 5, width, 1000, seed=31 + width)
    s[7], r[9] = 50, -1
    sd, rdd, od, gd = T._ids(s), T._ids(r), T._ids(o), g.to(DEV)
    # the default layout
    zd, rd = T._input(z), T._input(rel)
    ix = lib.lp_index_build(sd, rdd, od, 50, 5)
    score = lib.kge_score(code, zd, rd, sd, rdd, od)
    (_, dz), (_, drel) = T._output(50, width), T._output(5, width)
    assert _backward(dec, zd, rd, sd, rdd, od, gd, ix, dz, drel) == 0
    gq = torch.Generator().manual_seed(width)
    a, e, rq = torch.randint(0, 50, (70,), generator=gq), torch.randint(0, 50, (70,), generator=gq), torch.randint(0, 5, (70,), generator=gq)
    fptr, fidx = T._csr(T._lists(50, 70, e, gq))
    rank = [lib.kge_rank(code, side, zd, rd, T._ids(a), T._ids(rq), T._ids(e), fptr, fidx) for side in (0, 1)]
    assert not torch.equal(rank[0][0], rank[1][0])
    # the same data behind other strides and bases
    (zb, zv), (rb, rv) = E._inside(z, ldz, NAN), E._inside(rel, ldr, NAN)
    (dzb, dzv), (drb, drv) = E._inside((50, width), lddz, SENT), E._inside((5, width), lddrel, SENT)
    assert len({zv.stride(0), rv.stride(0), dzv.stride(0), drv.stride(0), w4}) == 5
    zb0, rb0 = zb.clone(), rb.clone()
    assert torch.equal(lib.kge_score(code, zv, rv, sd, rdd, od), score)
    assert _backward(dec, zv, rv, sd, rdd, od, gd, ix, dzv, drv) == 0
    assert torch.equal(dzv, dz) and torch.equal(drv, drel)
    for side in (0, 1):
        got = lib.kge_rank(code, side, zv, rv, T._ids(a), T._ids(rq), T._ids(e), fptr, fidx)
        assert torch.equal(got[0], rank[side][0]) and torch.equal(got[1], rank[side][1]), side
    # nothing outside the views but the +0 pads of the last 16-byte piece
    for buf, ref, rows, what in ((dzb, dz, 50, "dz"), (drb, drel, 5, "drel")):
        want = torch.full_like(buf, SENT)
        want[2:2 + rows, 4:4 + w4] = 0
        want[2:2 + rows, 4:4 + width] = ref
        assert torch.equal(buf, want), f"{what}: written outside its view"
        assert not bool(torch.signbit(buf[2:2 + rows, 4 + width:4 + w4]).any())
    assert torch.equal(zb.view(torch.int32), zb0.view(torch.int32)) and torch.equal(rb.view(torch.int32), rb0.view(torch.int32))
    # against float64 too: the default call is not its own reference
    ref_dz, ref_drel = K.backward(dec, z, rel, s, r, o, g)
    c_dz, c_drel = K.backward(dec, z, rel, s, r, o, g, absolute=True)
    assert_close(dzv.cpu().numpy(), ref_dz, c_dz, f"{dec} strided dz width {width}")
    assert_close(drv.cpu().numpy(), ref_drel, c_drel, f"{dec} strided drel width {width}")
    assert_close(score.cpu().numpy(), K.score(dec, z, rel, s, r, o)[0], K.score(dec, z, rel, s, r, o, absolute=True)[0], f"{dec} score")


# ---- 7. the Python layer ---------------------------------------------------------------------------------------------------------
def _layouts(z):
    """tests/test_gpu_linkpred_edges._layouts with a row pad that also serves width 3 (w + 1 = 4 is a stride the kernels read as it
    lies): [(name, leaf, view, region, copied)] -- z as it is; with a base 4 bytes off a 16-byte boundary; with a row stride that is
    no multiple of 4; with a column stride that is not 1"""
    n, w = z.shape
    zd, pad = z.to(DEV), 1 if (w + 1) % 4 else 2

    def leaf_of(shape, put):
        leaf = torch.full(shape, NAN, device=DEV)
        put(leaf).copy_(zd)
        return leaf.requires_grad_(True)

    cuts = [("contiguous", (n, w), lambda t: t, w % 4 != 0),
            ("base off by 4 bytes", (n, w + 4), lambda t: t[:, 1:1 + w], True),
            ("odd row stride", (n, w + pad), lambda t: t[:, :w], True),
            ("transposed", (w, n), lambda t: t.t(), True)]
    out = [(name, leaf_of(shape, cut), cut, copied) for name, shape, cut, copied in cuts]
    out = [(name, leaf, cut(leaf), cut, copied) for name, leaf, cut, copied in out]
    views = {name: view for name, _, view, _, _ in out}
    assert views["base off by 4 bytes"].data_ptr() % 16 == 4 and views["odd row stride"].stride(0) % 4 != 0
    assert views["transposed"].stride() == (1, n)
    return out


@pytest.mark.parametrize("dec,width", [("complex", 6), ("transe", 3)])
def test_decoders_on_layouts_that_have_to_be_copied(dec, width):
    from scaling_rgcn_training_amd import linkpred as L
    z, rel, s, r, o, g = KG._case(50, 5, width, 300, seed=40 + width)
    sd, rd, od, gd = T._ids(s), T._ids(r), T._ids(o), g.to(DEV)
    module = (L.ComplEx if dec == "complex" else L.TransE)(5, width).to(DEV)
    with torch.no_grad():
        module.rel.copy_(rel)
    results = {}
    for name, leaf, view, region, copied in _layouts(z):
        assert view.shape == z.shape and (L._padded(view.detach()).data_ptr() != view.data_ptr()) == copied, name
        module.rel.grad = None
        out = module(view, sd, rd, od)
        out.backward(gd)
        assert leaf.grad.shape == leaf.shape and module.rel.grad.shape == rel.shape
        outside = torch.ones_like(leaf, dtype=torch.bool)
        region(outside).fill_(False)
        assert not bool(leaf.grad[outside].any()), f"{name}: a gradient outside the view"
        counts = [t for side in ("object", "subject") for t in L.ranks(view.detach(), module, sd[:70], rd[:70], od[:70], side)]
        results[name] = (out.detach().clone(), region(leaf.grad).clone(), module.rel.grad.clone(), *counts)
    module.check()
    ref = results["contiguous"]
    for name, got in results.items():
        for what, x, y in zip(("scores", "z.grad", "rel.grad", "greater (object)", "equal (object)", "greater (subject)", "equal (subject)"),
                              got, ref):
            assert torch.equal(x, y), f"{name}: {what}"
    assert_close(ref[0].cpu().numpy(), K.score(dec, z, rel, s, r, o)[0], K.score(dec, z, rel, s, r, o, absolute=True)[0], f"{dec} forward")
    for got, want, cond in zip(ref[1:3], K.backward(dec, z, rel, s, r, o, g), K.backward(dec, z, rel, s, r, o, g, absolute=True)):
        assert_close(got.cpu().numpy(), want, cond, f"{dec} gradient width {width}")
    # the counts: inside the float64 band (multiples of 2^-4: in fact exact), and the same for every layout (above)
    for k, side in enumerate(("object", "subject")):
        anchor, target = (s, o) if side == "object" else (o, s)
        sc, cond = K.rank_scores(dec, z.numpy(), rel.numpy(), anchor[:70].numpy(), r[:70].numpy(), side)
        lo, hi = K.rank_band(sc, cond, target[:70].numpy())
        assert ((_np(ref[3 + 2 * k]) >= lo) & (_np(ref[3 + 2 * k]) <= hi)).all(), side
