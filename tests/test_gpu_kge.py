"""The ComplEx and TransE kernels (csrc/rgcn_kge.hip) against the float64 / integer restatements of
tests/kge_reference.py, with the conventions and the buffer helpers of tests/test_gpu_linkpred.py: NaN in the inputs' pad columns,
sentinels and a guard row around every output, ``assert_close`` with the sums on absolute values as ``cond``, rank counts on
integer-valued inputs EQUAL to the reference."""
import numpy as np
import pytest
import torch

from oracle.tolerance import assert_close
from tests import kge_reference as K
from tests import linkpred_reference as R
from tests.test_gpu_linkpred import DEV, _check_output_pads, _copies, _csr, _ids, _input, _lib, _lists, _output, _random_rank_case

pytestmark = pytest.mark.gpu

CODE = {"complex": 0, "transe": 1}
WIDTHS = [("complex", w) for w in (2, 6, 20, 64, 126, 128)] + [("transe", w) for w in (1, 3, 4, 20, 68, 128)]
DECS = ["complex", "transe"]


def _case(n_nodes, n_rel, width, n_triples, seed):
    """multiples of 2^-4 in [-4, 4]: every d = (s + r) - o is exact in fp32, so TransE's signs agree with float64; triple 0 has
    d = 0 in every column"""
    g = torch.Generator().manual_seed(seed)
    z, rel = (torch.randint(-64, 65, (rows, width), generator=g).float() / 16 for rows in (n_nodes, n_rel))
    s, o = (torch.randint(0, n_nodes, (n_triples,), generator=g) for _ in range(2))
    r = torch.randint(0, n_rel, (n_triples,), generator=g)
    if n_nodes > 1 and 0 <= s[0] < n_nodes and 0 <= r[0] < n_rel:
        o[0] = (s[0] + 1) % n_nodes
        z[o[0]] = z[s[0]] + rel[r[0]]
    return z, rel, s, r, o, torch.randn(n_triples, generator=g)


def _backward_raw(dec, z, rel, s, r, o, g, ix, dz, drel):
    """rgcn_kge_backward into the caller's views (the binding's wrapper allocates its own)"""
    c = _lib().load()
    ws = torch.empty(max(c.rgcn_kge_backward_workspace_bytes(CODE[dec], len(s), rel.shape[0], rel.shape[1]), 1), dtype=torch.uint8, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    st = c.rgcn_kge_backward(CODE[dec], z.data_ptr(), z.stride(0), rel.data_ptr(), rel.stride(0), rel.shape[1], z.shape[0], rel.shape[0],
                             s.data_ptr(), r.data_ptr(), o.data_ptr(), len(s), g.data_ptr(), p(ix.node_ptr), p(ix.node_slot), p(ix.rel_ptr),
                             p(ix.rel_triple), p(dz), 0 if dz is None else dz.stride(0), p(drel), 0 if drel is None else drel.stride(0),
                             ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


def _check_case(dec, z, rel, s, r, o, g, what):
    """score and backward of one case against float64, twice (the same bits), each gradient also alone; returns the reference dz"""
    lib, (n_nodes, width), n_rel = _lib(), z.shape, rel.shape[0]
    zd, rd, sd, rdd, od, gd = _input(z), _input(rel), _ids(s), _ids(r), _ids(o), g.to(DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = lib.kge_score(CODE[dec], zd, rd, sd, rdd, od, bad)
    ref, ref_bad = K.score(dec, z, rel, s, r, o)
    assert_close(got.cpu().numpy(), ref, K.score(dec, z, rel, s, r, o, absolute=True)[0], f"kge_score {what}")
    assert int(bad.item()) == ref_bad and torch.equal(got, lib.kge_score(CODE[dec], zd, rd, sd, rdd, od))
    ix = lib.lp_index_build(sd, rdd, od, n_nodes, n_rel)
    ref_dz, ref_drel = K.backward(dec, z, rel, s, r, o, g)
    c_dz, c_drel = K.backward(dec, z, rel, s, r, o, g, absolute=True)
    first = None
    for want_z, want_rel in ((True, True), (True, True), (True, False), (False, True)):
        (zbuf, dz), (rbuf, drel) = _output(n_nodes, width), _output(n_rel, width)
        assert _backward_raw(dec, zd, rd, sd, rdd, od, gd, ix, dz if want_z else None, drel if want_rel else None) == 0
        first = first or (dz.clone(), drel.clone())
        for want, buf, out, ref_g, cond, rows, name in ((want_z, zbuf, dz, ref_dz, c_dz, n_nodes, "dz"),
                                                        (want_rel, rbuf, drel, ref_drel, c_drel, n_rel, "drel")):
            if not want:
                assert bool((buf == 777.0).all()), f"{name} was not asked for"
                continue
            assert_close(out.cpu().numpy(), ref_g, cond, f"kge_backward {name} {what}")
            _check_output_pads(buf, rows, width, name)
            assert torch.equal(out, first[0] if name == "dz" else first[1]), f"{name}: another call, other bits"
    return ref_dz


@pytest.mark.parametrize("dec,width", WIDTHS)
def test_score_and_backward_widths(dec, width):
    for n_triples in (1, 63, 65, 1000):
        z, rel, s, r, o, g = _case(50, 5, width, n_triples, seed=width * 7 + n_triples)
        _check_case(dec, z, rel, s, r, o, g, f"{dec} width {width} T {n_triples}")
    if dec == "transe" and width >= 3:
        assert (((z[s] + rel[r]) - z[o]) == 0).sum() >= width            # exact zeros of d: gradient 0 there


@pytest.mark.parametrize("dec,width", [("complex", 20), ("transe", 20), ("transe", 3)])
def test_backward_hubs_gaps_chunks_and_ends(dec, width):
    """40 nodes, relations with exactly 0, 1, 255, 256, 257 and 513 triples; node 0 in most triples, node 39 in none, ten triples with
    s = o, ids out of range.  Swapping the two ends' formulas in dz must move the result far outside the tolerance."""
    counts = [0, 1, 255, 256, 257, 516]          # (three of the last relation's triples get an id out of range: 513 are left)
    z, rel, s, r, o, g = _case(40, 6, width, sum(counts), seed=3)
    s, o = s.clamp(1, 38), o.clamp(1, 38)
    r = torch.repeat_interleave(torch.arange(6), torch.tensor(counts))[torch.randperm(sum(counts), generator=torch.Generator().manual_seed(1))]
    s[::3], o[1::3] = 0, 0
    s[100:110] = o[100:110]
    t5 = torch.nonzero(r == 5)[:3, 0]
    s[t5[0]], o[t5[1]], r[t5[2]] = 40, -1, 6
    ref_dz = _check_case(dec, z, rel, s, r, o, g, f"{dec} structured")
    assert not ref_dz[39].any() and np.bincount(r.numpy()[R.valid_triples(s, r, o, 40, 6)[0]], minlength=6).tolist() == [0, 1, 255, 256, 257, 513]
    ok = torch.as_tensor(R.valid_triples(s, r, o, 40, 6)[0])
    _, ds, _, do = K.parts(dec, *(t.double().numpy() for t in (z[s[ok]], rel[r[ok]], z[o[ok]])))
    swapped = np.zeros_like(ref_dz)
    np.add.at(swapped, s[ok].numpy(), g[ok].double().numpy()[:, None] * do)
    np.add.at(swapped, o[ok].numpy(), g[ok].double().numpy()[:, None] * ds)
    assert np.abs(swapped - ref_dz).max() > 1.0


@pytest.mark.parametrize("dec", DECS)
def test_no_triples_launch_nothing(dec):
    lib = _lib()
    z, rel, e = _input(torch.randn(7, 20)), _input(torch.randn(3, 20)), torch.zeros(0, dtype=torch.int64, device=DEV)
    assert lib.kge_score(CODE[dec], z, rel, e, e, e).shape == (0,)
    (zb, dz), (rb, drel) = _output(7, 20), _output(3, 20)
    assert _backward_raw(dec, z, rel, e, e, e, torch.zeros(0, device=DEV), lib.lp_index_build(e, e, e, 7, 3), dz, drel) == 0
    assert bool((zb == 777.0).all()) and bool((rb == 777.0).all())
    gr, eq = lib.kge_rank(CODE[dec], 0, z, rel, e, e, e)
    assert gr.shape == eq.shape == (0,)


# ---- ranks ------------------------------------------------------------------------------------------------------------------
def _reference_counts(dec, z, rel, a, r, e, side, lists):
    sc, _ = K.rank_scores(dec, z.numpy(), rel.numpy(), a.numpy(), r.numpy(), side)
    assert np.abs(sc).max() < 2 ** 24 and (sc == np.round(sc)).all()
    return R.rank_counts(sc, e.numpy(), lists)


RANK_SHAPES = [(1, 1, 0), (15, 63, 1), (17, 65, 2), (129, 130, 3), (300, 65, 1)]       # (N, Q, index into the decoder's widths)
RANK_WIDTHS = {"complex": (2, 20, 64, 128), "transe": (1, 17, 64, 128)}


@pytest.mark.parametrize("dec", DECS)
@pytest.mark.parametrize("n_nodes,n_q,wi", RANK_SHAPES)
@pytest.mark.parametrize("filtered", [False, True])
def test_rank_counts_equal_the_integer_reference(dec, n_nodes, n_q, wi, filtered):
    """entries in [-3, 3] (ComplEx relations in [-1, 1]): every score is an exact integer in fp32.  Both sides on the same arrays:
    the counts must differ between them, so a side mix-up fails."""
    width, g = RANK_WIDTHS[dec][wi], torch.Generator().manual_seed(n_nodes + n_q)
    z = torch.randint(-3, 4, (n_nodes, width), generator=g).float()
    rel = torch.randint(-1, 2, (3, width), generator=g).float()
    a, e = (torch.randint(0, n_nodes, (n_q,), generator=g) for _ in range(2))
    r = torch.randint(0, 3, (n_q,), generator=g)
    lists = _lists(n_nodes, n_q, e, g) if filtered else None      # in turn: empty, only the target, every entity, 40 entries, 3
    fptr, fidx = _csr(lists) if filtered else (None, None)
    refs = {}
    for code, side in enumerate(("object", "subject")):
        got = _lib().kge_rank(CODE[dec], code, _input(z), _input(rel), _ids(a), _ids(r), _ids(e), fptr, fidx)
        refs[side] = _reference_counts(dec, z, rel, a, r, e, side, lists)
        for name, x, y in zip(("greater", "equal"), got, refs[side]):
            assert np.array_equal(x.cpu().numpy(), y), (side, name, x.cpu().numpy(), y)
    if n_nodes >= 15:
        assert not np.array_equal(refs["object"][0], refs["subject"][0])
    if filtered and n_nodes > 1:
        assert not refs["object"][0][2::5].any() and refs["object"][1].sum() > 0        # every entity listed: 0; ties exist


@pytest.mark.parametrize("dec", DECS)
def test_rank_query_with_an_id_out_of_range(dec):
    g = torch.Generator().manual_seed(1)
    z, rel = torch.randint(-3, 4, (20, 4), generator=g).float(), torch.randint(-1, 2, (3, 4), generator=g).float()
    a, e, r = torch.randint(0, 20, (5,), generator=g), torch.randint(0, 20, (5,), generator=g), torch.randint(0, 3, (5,), generator=g)
    ref_g, ref_e = _reference_counts(dec, z, rel, a, r, e, "subject", None)
    a[1], r[2], e[3] = 20, 3, -1
    ref_g[1:4] = ref_e[1:4] = -1
    got_g, got_e = _lib().kge_rank(CODE[dec], 1, _input(z), _input(rel), _ids(a), _ids(r), _ids(e))
    assert np.array_equal(got_g.cpu().numpy(), ref_g) and np.array_equal(got_e.cpu().numpy(), ref_e)


# Seed 0 of tests/test_gpu_linkpred._random_rank_case, picked on the CPU: the float64 bands are open for (complex / object 1,
# complex / subject 0, transe / object 1, transe / subject 0) of 256 queries, and an fp32 numpy restatement that adds the columns in
# another order (kge_reference.parts on float32 arrays: numpy's pairwise ``sum`` over the row) leaves 0 counts outside their bands.
@pytest.mark.parametrize("dec", DECS)
@pytest.mark.parametrize("code,side", [(0, "object"), (1, "subject")])
def test_rank_random_inputs_copies_and_bands(dec, code, side):
    """standard normal inputs, N = 1,000, Q = 256, width 64, 60 rows copied bit for bit onto other ids: ``equal`` counts exactly the
    unfiltered copies, ``greater`` lies in the float64 band, which is open for at most 2 % of the queries"""
    z, rel, a, r, e, src, lists = _random_rank_case(0)
    copies = [_copies(z, e, i) for i in range(256)]
    sc, cond = K.rank_scores(dec, z.numpy(), rel.numpy(), a.numpy(), r.numpy(), side)
    lo, hi = K.rank_band(sc, cond, e.numpy(), [sorted(set(lists[i]) | set(copies[i])) for i in range(256)])
    assert int((lo != hi).sum()) <= 0.02 * 256
    want_equal = np.array([len([v for v in copies[i] if v != int(e[i]) and v not in set(lists[i])]) for i in range(256)])
    assert want_equal[:40].sum() > 20
    fptr, fidx = _csr(lists)
    got_g, got_e = (t.cpu().numpy() for t in _lib().kge_rank(CODE[dec], code, _input(z), _input(rel), _ids(a), _ids(r), _ids(e), fptr, fidx))
    print(f"kge rank {dec} {side}: open bands {int((lo != hi).sum())}/256, outside {int(((got_g < lo) | (got_g > hi)).sum())}")
    assert np.array_equal(got_e, want_equal)
    assert ((got_g >= lo) & (got_g <= hi)).all()


# ---- the modules ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dec,width", [("complex", 6), ("transe", 3)])
def test_decoder_autograd_and_ranks_with_a_filter_index(dec, width):
    from scaling_rgcn_training_amd import linkpred as L
    z, rel, s, r, o, g = _case(50, 5, width, 300, seed=5)
    module = (L.ComplEx if dec == "complex" else L.TransE)(5, width).to(DEV)
    with torch.no_grad():
        module.rel.copy_(rel)
    zd, (sd, rd, od) = z.to(DEV).requires_grad_(True), (_ids(t) for t in (s, r, o))
    out = module(zd, sd, rd, od)
    assert module.index_builds == {"node": 0, "relation": 0}
    out.backward(g.to(DEV))
    assert module.index_builds == {"node": 1, "relation": 1}
    assert_close(out.detach().cpu().numpy(), K.score(dec, z, rel, s, r, o)[0], K.score(dec, z, rel, s, r, o, absolute=True)[0], f"{dec} forward")
    for got, ref, cond in zip((zd.grad, module.rel.grad), K.backward(dec, z, rel, s, r, o, g), K.backward(dec, z, rel, s, r, o, g, absolute=True)):
        assert got.shape == ref.shape
        assert_close(got.cpu().numpy(), ref, cond, f"{dec} gradient")
    module.check()
    bad = sd.clone()
    bad[0] = 50
    module(zd, bad, rd, od)
    with pytest.raises(ValueError, match="node id"):
        module.check()
    # ranks + FilterIndex, both sides, on integer-valued tables
    gen = torch.Generator().manual_seed(8)
    zi, s, r, o = torch.randint(-3, 4, (50, width), generator=gen).float(), s[:70], r[:70], o[:70]
    with torch.no_grad():
        module.rel.copy_(torch.randint(-1, 2, (5, width), generator=gen).float())
    known = torch.cat([torch.stack([torch.randint(0, 50, (400,), generator=gen), torch.randint(0, 5, (400,), generator=gen),
                                    torch.randint(0, 50, (400,), generator=gen)], 1), torch.stack([s, r, o], 1)])
    filt = L.FilterIndex(known.to(DEV), 50, 5)
    for side in ("object", "subject"):
        anchor, target = (s, o) if side == "object" else (o, s)
        sets = R.filter_sets(known.numpy(), side)
        lists = [sorted(sets.get((int(anchor[i]), int(r[i])), ())) for i in range(70)]
        for f, ls in ((None, None), (filt, lists)):
            got = L.ranks(zi.to(DEV), module, _ids(s), _ids(r), _ids(o), side, f)
            ref = _reference_counts(dec, zi, module.rel.detach().cpu(), anchor, r, target, side, ls)
            assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(got, ref)), side
