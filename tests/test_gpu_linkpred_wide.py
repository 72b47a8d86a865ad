"""Link prediction on rows of 129..512 columns (csrc/rgcn_linkpred_wide.hip) against the float64 / integer restatements
of tests/linkpred_reference.py, with the conventions and helpers of tests/test_gpu_linkpred.py: NaN in the inputs' pad columns,
sentinels and a guard row around every output, ``assert_close`` with the sums on absolute values as ``cond``, rank counts on
integer-valued inputs EQUAL to the reference."""
import numpy as np
import pytest
import torch

from oracle.tolerance import assert_close
from tests import linkpred_reference as R
from tests.test_gpu_linkpred import DEV, _check_output_pads, _copies, _csr, _exact_case, _ids, _input, _lib, _lists, _output, _random_case

pytestmark = pytest.mark.gpu

WAVES = 4      # kChunkWaves: the waves that share a chunk of a relation's gradient


def _backward_raw(z, rel, s, r, o, g, ix, dz, drel):
    """rgcn_lpw_backward into the caller's views (the binding's wrapper allocates its own)"""
    c = _lib().load()
    ws = torch.empty(max(c.rgcn_lpw_backward_workspace_bytes(len(s), rel.shape[0], rel.shape[1]), 1), dtype=torch.uint8, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    st = c.rgcn_lpw_backward(z.data_ptr(), z.stride(0), rel.data_ptr(), rel.stride(0), rel.shape[1], z.shape[0], rel.shape[0],
                             s.data_ptr(), r.data_ptr(), o.data_ptr(), len(s), g.data_ptr(), p(ix.node_ptr), p(ix.node_slot),
                             p(ix.rel_ptr), p(ix.rel_triple), p(dz), 0 if dz is None else dz.stride(0), p(drel),
                             0 if drel is None else drel.stride(0), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


def _check_case(z, rel, s, r, o, g, what):
    """score and backward of one case against float64, twice with the same bits; returns (dz, drel) and the device inputs"""
    lib = _lib()
    (n_nodes, width), n_rel = z.shape, rel.shape[0]
    zd, rd, sd, rdd, od, gd = _input(z), _input(rel), _ids(s), _ids(r), _ids(o), g.to(DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = lib.lpw_score(zd, rd, sd, rdd, od, bad)
    ref, cond, ref_bad = R.score(z, rel, s, r, o)
    assert_close(got.cpu().numpy(), ref, cond, f"lpw_score {what}")
    assert int(bad.item()) == ref_bad and torch.equal(got, lib.lpw_score(zd, rd, sd, rdd, od))
    ix = lib.lp_index_build(sd, rdd, od, n_nodes, n_rel)
    ref_dz, ref_drel = R.backward(z, rel, s, r, o, g)
    c_dz, c_drel = R.backward_cond(z, rel, s, r, o, g)
    outs = []
    for _ in range(2):
        (zbuf, dz), (rbuf, drel) = _output(n_nodes, width), _output(n_rel, width)
        assert _backward_raw(zd, rd, sd, rdd, od, gd, ix, dz, drel) == 0
        _check_output_pads(zbuf, n_nodes, width, "dz")
        _check_output_pads(rbuf, n_rel, width, "drel")
        outs.append((dz, drel))
    assert_close(outs[0][0].cpu().numpy(), ref_dz, c_dz, f"lpw_backward dz {what}")
    assert_close(outs[0][1].cpu().numpy(), ref_drel, c_drel, f"lpw_backward drel {what}")
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    return outs[0], (zd, rd, sd, rdd, od, gd, ix)


# the first wide width, a full wave of pieces, the first second piece, both sides of every 128-column slab edge, a ragged last piece
@pytest.mark.parametrize("n_triples", [1, 5, 1000])
@pytest.mark.parametrize("width", [129, 132, 256, 257, 260, 384, 388, 511, 512])
def test_score_and_backward_widths(width, n_triples):
    z, rel, s, r, o, g = _random_case(50, 5, width, n_triples, seed=width * 7 + n_triples)
    _check_case(z, rel, s, r, o, g, f"width {width} T {n_triples}")


def test_backward_hubs_gaps_chunks_and_bad_ids():
    """width 260: node 0 in 1,000 triples, node 39 in none, s == o, relations with 0, 1, 255, 256, 257, 513, WAVES - 1 and WAVES + 1
    triples (1,290 in all: the counts do not fit into fewer) and 10 triples with an id out of range"""
    gen = torch.Generator().manual_seed(3)
    counts = [0, 1, 255, 256, 257, 513, WAVES - 1, WAVES + 1]
    n, n_nodes, width = sum(counts) + 10, 40, 260
    z, rel = torch.randn(n_nodes, width, generator=gen), torch.randn(len(counts), width, generator=gen)
    s, o = (torch.randint(1, n_nodes - 1, (n,), generator=gen) for _ in range(2))
    hub = torch.randperm(1200, generator=gen)[:1000]
    s[hub[:500]], o[hub[500:]] = 0, 0
    s[1210:1220] = o[1210:1220]
    r = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
    r = torch.cat([r[torch.randperm(len(r), generator=gen)], torch.zeros(10, dtype=torch.int64)])
    s[-10:-7], o[-7:-5], r[-5:-2], s[-2], r[-2], o[-1] = n_nodes, 2 ** 40, len(counts), -1, -3, -7
    perm = torch.randperm(n, generator=gen)
    s, r, o = s[perm], r[perm], o[perm]
    ok, ref_bad = R.valid_triples(s.numpy(), r.numpy(), o.numpy(), n_nodes, len(counts))
    assert ref_bad == 3 and np.bincount(r.numpy()[ok], minlength=len(counts)).tolist() == counts
    assert int((((s == 0) | (o == 0)).numpy() & ok).sum()) >= 1000 and not bool(((s == 39) | (o == 39)).any()) and bool((s == o).any())
    (dz, drel), (zd, rd, sd, rdd, od, gd, ix) = _check_case(z, rel, s, r, o, torch.randn(n, generator=gen), "structured")
    assert bool((dz[39] == 0).all()) and bool((drel[0] == 0).all())      # no triple: zero rows over the sentinels
    # one gradient only: the wanted one has the same bits (and the call takes a NULL for the other)
    (_, dz2), (_, drel2) = _output(*dz.shape), _output(*drel.shape)
    assert _backward_raw(zd, rd, sd, rdd, od, gd, ix, dz2, None) == 0 and torch.equal(dz, dz2)
    assert _backward_raw(zd, rd, sd, rdd, od, gd, ix, None, drel2) == 0 and torch.equal(drel, drel2)


# ---- ranks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("n_nodes,n_q", [(1, 1), (15, 63), (17, 64), (129, 65), (300, 130)])
@pytest.mark.parametrize("width", [129, 256, 260, 512])
def test_rank_counts_equal_the_integer_reference(width, n_nodes, n_q, filtered):
    z, rel, a, r, e, g = _exact_case(n_nodes, n_q, width, seed=n_nodes + n_q)
    lists = _lists(n_nodes, n_q, e, g) if filtered else None
    fptr, fidx = _csr(lists) if filtered else (None, None)
    sc, _ = R.rank_scores(z, rel, a, r)
    assert np.abs(sc).max() < 2 ** 24
    ref_g, ref_e = R.rank_counts(sc, e.numpy(), lists)
    for wg in (0, 32, 64):                                              # the counts do not depend on the workgroup shape
        got_g, got_e = _lib().lpw_rank(_input(z), _input(rel), _ids(a), _ids(r), _ids(e), fptr, fidx, wg_queries=wg)
        assert np.array_equal(got_g.cpu().numpy(), ref_g), (wg, got_g.cpu().numpy(), ref_g)
        assert np.array_equal(got_e.cpu().numpy(), ref_e), (wg, got_e.cpu().numpy(), ref_e)


@pytest.mark.parametrize("width", [132, 260, 512])
def test_rank_random_inputs_copies_and_bands(width):
    """N = 300, Q = 128, standard normal at seed 0; rows 240..299 are bit copies of z[cat(e[:40], 20 random ids)], some of them
    filtered: `equal` counts exactly the unfiltered copies, `greater` lies in the float64 band of EVERY query"""
    g = torch.Generator().manual_seed(0)
    z, rel = torch.randn(300, width, generator=g), torch.randn(4, width, generator=g)
    a, e = torch.randint(0, 240, (128,), generator=g), torch.randint(0, 240, (128,), generator=g)
    r = torch.randint(0, 4, (128,), generator=g)
    z[240:] = z[torch.cat([e[:40], torch.randint(0, 240, (20,), generator=g)])]
    lists = []
    for i in range(128):
        ids = torch.randperm(300, generator=g)[:int(torch.randint(0, 30, (1,), generator=g))].tolist()
        lists.append(sorted(set(ids) | {240 + i}) if i % 3 == 0 and i < 40 else ids)
    copies = [_copies(z, e, i) for i in range(128)]
    want_equal = np.array([len([v for v in copies[i] if v != int(e[i]) and v not in set(lists[i])]) for i in range(128)])
    assert want_equal[:40].sum() > 20
    out = [sorted(set(lists[i]) | set(copies[i])) for i in range(128)]      # the copies are `equal`'s to count, not the band's
    lo, hi = R.rank_band(z.numpy(), rel.numpy(), a.numpy(), r.numpy(), e.numpy(), out)
    got_g, got_e = (t.cpu().numpy() for t in _lib().lpw_rank(_input(z), _input(rel), _ids(a), _ids(r), _ids(e), *_csr(lists)))
    print(f"rank random width {width}: open bands {int((lo != hi).sum())}/128, equal counted {got_e.sum()} (expected "
          f"{want_equal.sum()}), greater outside its band in {int(((got_g < lo) | (got_g > hi)).sum())} queries")
    assert np.array_equal(got_e, want_equal)
    assert ((got_g >= lo) & (got_g <= hi)).all()


# ---- through the module ---------------------------------------------------------------------------------------------------------
def test_distmult_wide_autograd_ranks_and_narrow_bits():
    from scaling_rgcn_training_amd.linkpred import DistMult, FilterIndex, ranks
    z, rel, s, r, o, g = _random_case(50, 4, 260, 300, seed=5)
    dec = DistMult(4, 260, wide=True).to(DEV)
    with torch.no_grad():
        dec.rel.copy_(rel)
    zd = z.to(DEV).requires_grad_(True)
    out = dec(zd, _ids(s), _ids(r), _ids(o))
    out.backward(g.to(DEV))
    ref, cond, _ = R.score(z, rel, s, r, o)
    assert_close(out.detach().cpu().numpy(), ref, cond, "DistMult wide forward")
    ref_dz, ref_drel = R.backward(z, rel, s, r, o, g)
    c_dz, c_drel = R.backward_cond(z, rel, s, r, o, g)
    assert zd.grad.shape == z.shape and dec.rel.grad.shape == rel.shape
    assert_close(zd.grad.cpu().numpy(), ref_dz, c_dz, "DistMult wide dz")
    assert_close(dec.rel.grad.cpu().numpy(), ref_drel, c_drel, "DistMult wide drel")
    dec.check()
    # ranks + FilterIndex on both sides against the integer reference
    z, rel, s, r, o, gen = _exact_case(90, 70, 260, seed=8)
    rel = torch.cat([rel, rel[:1]])
    known = torch.cat([torch.stack([torch.randint(0, 90, (600,), generator=gen), torch.randint(0, 4, (600,), generator=gen),
                                    torch.randint(0, 90, (600,), generator=gen)], 1), torch.stack([s, r, o], 1)])
    with torch.no_grad():
        dec.rel.copy_(rel)
    filt = FilterIndex(known.to(DEV), 90, 4)
    for side in ("object", "subject"):
        anchor, target = (s, o) if side == "object" else (o, s)
        sets = R.filter_sets(known.numpy(), side)
        lists = [sorted(sets.get((int(anchor[i]), int(r[i])), ())) for i in range(70)]
        sc, _ = R.rank_scores(z, rel, anchor, r)
        for f, ls in ((None, None), (filt, lists)):
            got_g, got_e = ranks(z.to(DEV), dec, _ids(s), _ids(r), _ids(o), side, f)
            ref_g, ref_e = R.rank_counts(sc, target.numpy(), ls)
            assert np.array_equal(got_g.cpu().numpy(), ref_g) and np.array_equal(got_e.cpu().numpy(), ref_e), side
    # a wide decoder of at most 128 columns runs on the narrow kernels: bit for bit the decoder without the flag
    z, rel, s, r, o, g = _random_case(50, 4, 64, 300, seed=6)
    res = []
    for dec in (DistMult(4, 64, wide=True).to(DEV), DistMult(4, 64).to(DEV)):
        with torch.no_grad():
            dec.rel.copy_(rel)
        zd = z.to(DEV).requires_grad_(True)
        dec(zd, _ids(s), _ids(r), _ids(o)).backward(g.to(DEV))
        res.append((dec(zd, _ids(s), _ids(r), _ids(o)).detach(), zd.grad, dec.rel.grad, *ranks(zd, dec, _ids(s), _ids(r), _ids(o))))
    assert all(torch.equal(x, y) for x, y in zip(*res))
