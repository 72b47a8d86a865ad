"""The host side of link prediction (scaling_rgcn_training_amd/linkpred.py, the argument checks of csrc/rgcn_linkpred.hip): everything
here is answered before a kernel is launched, so it runs without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from scaling_rgcn_training_amd import _lib
from scaling_rgcn_training_amd import linkpred as L
from tests import linkpred_reference as R

NULL, WIDTH, STRIDE, PLAN, WS, ARG = -1, -2, -3, -4, -6, -11
_BUF = (ctypes.c_float * 1024)()


def _p():
    a = ctypes.addressof(_BUF)
    return a + (-a % 16)            # a 16-byte aligned host address the checks see as non-NULL and never read


# ---- FilterIndex --------------------------------------------------------------------------------------------------------------
def _known(seed=0):
    g = torch.Generator().manual_seed(seed)
    n = 1500
    known = torch.stack([torch.randint(0, 60, (n,), generator=g), torch.randint(0, 5, (n,), generator=g),
                         torch.randint(0, 60, (n,), generator=g)], 1)
    hub = torch.stack([torch.full((300,), 7), torch.full((300,), 2), torch.arange(300) % 350], 1)       # (7, 2, ?) has 300 objects
    known = torch.cat([known, hub, known[:50]])                                                        # and some rows twice
    known = known[(known[:, 0] != 11) | (known[:, 1] != 3)]                                           # (11, 3, ?) has none
    return known


@pytest.mark.parametrize("side", ["object", "subject"])
def test_filter_index_matches_a_set_lookup(side):
    known = _known()
    filt = L.FilterIndex(known, 400, 5)
    sets = R.filter_sets(known.numpy(), side)
    g = torch.Generator().manual_seed(1)
    s, o = (torch.randint(0, 60, (200,), generator=g) for _ in range(2))
    r = torch.randint(0, 5, (200,), generator=g)
    s[0], r[0] = 7, 2            # the hub
    s[1], r[1] = 11, 3           # no known triple (object side)
    s[2], r[2], o[2] = 399, 4, 399
    ptr, idx = filt.lists(s, r, o, side)
    assert ptr.dtype == idx.dtype == torch.int64 and ptr.shape == (201,) and int(ptr[0]) == 0 and int(ptr[-1]) == idx.numel()
    for i in range(200):
        key = (int(s[i]), int(r[i])) if side == "object" else (int(o[i]), int(r[i]))
        got = idx[int(ptr[i]):int(ptr[i + 1])].tolist()
        assert got == sorted(sets.get(key, ())), (i, key)            # distinct, ascending
    if side == "object":
        assert int(ptr[1] - ptr[0]) == 300 and int(ptr[2] - ptr[1]) == 0 and int(ptr[3] - ptr[2]) == 0
    e = torch.zeros(0, dtype=torch.int64)
    ptr, idx = filt.lists(e, e, e, side)
    assert ptr.tolist() == [0] and idx.numel() == 0


def test_filter_index_refusals():
    with pytest.raises(ValueError):
        L.FilterIndex(torch.zeros(5, 2, dtype=torch.int64), 10, 3)
    with pytest.raises(ValueError):
        L.FilterIndex(torch.zeros(5, 3), 10, 3)
    with pytest.raises(ValueError, match="out of range"):
        L.FilterIndex(torch.tensor([[0, 3, 1]]), 10, 3)
    with pytest.raises(ValueError, match="out of range"):
        L.FilterIndex(torch.tensor([[0, 0, 10]]), 10, 3)
    filt = L.FilterIndex(torch.zeros(0, 3, dtype=torch.int64), 10, 3)
    q = torch.tensor([1, 2])
    ptr, idx = filt.lists(q, q, q)
    assert ptr.tolist() == [0, 0, 0] and idx.numel() == 0
    with pytest.raises(ValueError, match="side"):
        filt.lists(q, q, q, "both")
    with pytest.raises(ValueError):
        filt.lists(q, q, q[:1])


# ---- metrics, inverse edges ---------------------------------------------------------------------------------------------------
def test_metrics_on_hand_made_counts():
    greater, equal = torch.tensor([0, 0, 2, 9, 10]), torch.tensor([0, 2, 0, 1, 0])
    m = L.metrics(greater, equal)                      # ranks 1, 2, 3, 10.5, 11
    assert m["mrr"] == pytest.approx((1 + 1 / 2 + 1 / 3 + 1 / 10.5 + 1 / 11) / 5, abs=1e-15)
    assert (m["hits@1"], m["hits@3"], m["hits@10"]) == (0.2, 0.6, 0.6)
    m = L.metrics(greater, equal, ks=(1, 10), ties="optimistic")      # ranks 1, 1, 3, 10, 11
    assert m["mrr"] == pytest.approx((1 + 1 + 1 / 3 + 1 / 10 + 1 / 11) / 5, abs=1e-15)
    assert (m["hits@1"], m["hits@10"]) == (0.4, 0.8) and "hits@3" not in m
    assert m == pytest.approx(R.metrics(greater.numpy(), equal.numpy(), ks=(1, 10), ties="optimistic"), abs=1e-15)
    for bad in (dict(ties="worst"),):
        with pytest.raises(ValueError):
            L.metrics(greater, equal, **bad)
    with pytest.raises(ValueError, match="out of range"):
        L.metrics(torch.tensor([1, -1]), torch.tensor([0, -1]))
    with pytest.raises(ValueError):
        L.metrics(greater, equal[:2])
    with pytest.raises(ValueError):
        L.metrics(greater[:0], equal[:0])


def test_with_inverse_edges():
    ei, et = torch.tensor([[0, 1, 2], [3, 4, 5]]), torch.tensor([0, 2, 1])
    ei2, et2 = L.with_inverse_edges(ei, et, 3)
    assert ei2.tolist() == [[0, 1, 2, 3, 4, 5], [3, 4, 5, 0, 1, 2]] and et2.tolist() == [0, 2, 1, 3, 5, 4]
    with pytest.raises(ValueError):
        L.with_inverse_edges(ei.t(), et, 3)
    with pytest.raises(ValueError):
        L.with_inverse_edges(ei, et[:2], 3)
    with pytest.raises(ValueError):
        L.with_inverse_edges(ei, et, 0)


# ---- the Python layer's refusals ------------------------------------------------------------------------------------------------
def test_distmult_arguments():
    for args in ((0, 8), (65537, 8), (3, 0), (3, 129), (True, 8), (3, 8.0)):
        with pytest.raises(ValueError):
            L.DistMult(*args)
    dec = L.DistMult(3, 8)
    assert dec.rel.shape == (3, 8) and dec.rel.requires_grad
    bound = (6 / (3 + 8)) ** 0.5                                      # xavier_uniform_
    assert float(dec.rel.detach().abs().max()) <= bound
    ids = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError):
        dec(torch.zeros(5, 7), ids, ids, ids)
    with pytest.raises(ValueError):
        dec(torch.zeros(5, 8), ids, ids, ids[:3])
    with pytest.raises(ValueError):
        dec(torch.zeros(5, 8), ids.int(), ids, ids)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # a missing GPU is an error, never a torch formulation
        dec(torch.zeros(5, 8), ids, ids, ids)
    dec.check()


def test_corrupt_and_ranks_arguments():
    ids = torch.zeros(4, dtype=torch.int64)
    for kw in (dict(num_nodes=0), dict(num_negatives=0), dict(seed=-1), dict(num_nodes=2 ** 31), dict(num_negatives=1.5), dict(seed=True)):
        args = dict(num_nodes=10, num_negatives=2, seed=0)
        args.update(kw)
        with pytest.raises(ValueError):
            L.corrupt(ids, ids, ids, **args)
    with pytest.raises(ValueError):
        L.corrupt(ids, ids[:2], ids, 10, 2, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.corrupt(ids, ids, ids, 10, 2, 0)
    dec = L.DistMult(3, 8)
    z = torch.zeros(5, 8)
    with pytest.raises(ValueError, match="side"):
        L.ranks(z, dec, ids, ids, ids, side="left")
    with pytest.raises(ValueError):
        L.ranks(z, nn_module_without_rel(), ids, ids, ids)
    with pytest.raises(ValueError):
        L.ranks(z, dec, ids, ids, ids, filter=object())
    with pytest.raises(ValueError):
        L.ranks(torch.zeros(5, 4), dec, ids, ids, ids)
    with pytest.raises(ValueError, match="another number"):
        L.ranks(z, dec, ids, ids, ids, filter=L.FilterIndex(torch.zeros(0, 3, dtype=torch.int64), 6, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.ranks(z, dec, ids, ids, ids)


def nn_module_without_rel():
    return torch.nn.Linear(2, 2)


def test_train_link_prediction_arguments():
    from scaling_rgcn_training_amd.trainer import Trainer
    t = Trainer(None, 8, 1, 8, 0.01, 0.0, verbose=False)
    tri = torch.zeros(4, 3, dtype=torch.int64)
    for kw in (dict(train_triples=tri[:, :2]), dict(train_triples=tri.int()), dict(train_triples=tri[:0]), dict(valid_triples=tri.float()),
               dict(num_negatives=0), dict(batch_size=0), dict(batch_size=2.5), dict(reg=-1.0), dict(seed=-1)):
        args = dict(train_triples=tri)
        args.update(kw)
        with pytest.raises(ValueError):
            t.train_link_prediction(None, None, None, **args)


# ---- the C ABI's refusals and workspace queries: no launch, no device --------------------------------------------------------
def test_lp_argument_refusals():
    lib, p = _lib.load(), _p()
    score = lambda z=p, ldz=16, rel=p, ldr=16, w=16, n=10, nr=3, s=p, t=5, out=p: lib.rgcn_lp_score(z, ldz, rel, ldr, w, n, nr, s, s, s, t, out,
                                                                                                  None, None)
    assert score(z=None) == NULL and score(rel=None) == NULL and score(s=None) == NULL and score(out=None) == NULL
    assert score(w=0) == WIDTH and score(w=129, ldz=256, ldr=256) == WIDTH
    assert score(ldz=12) == STRIDE and score(ldr=18) == STRIDE and score(w=5, ldz=4, ldr=8) == STRIDE and score(z=p + 4) == STRIDE
    assert score(t=-1) == ARG and score(n=-1) == ARG
    assert score(nr=65537) == PLAN and score(t=0x7FFF8001) == PLAN
    assert score(t=0) == 0 and score(t=0, s=None, out=None) == 0                                 # nothing to do: no launch
    build = lambda s=p, t=5, n=10, nr=3, np_=p, ns=p, rp=p, rt=p, ws=p, nbytes=1 << 30: lib.rgcn_lp_index_build(s, s, s, t, n, nr, np_, ns, rp,
                                                                                                                  rt, None, ws, nbytes, None)
    assert build(np_=None, rp=None) == NULL and build(s=None) == NULL and build(ns=None) == NULL and build(rt=None) == NULL
    assert build(t=-1) == ARG and build(nr=65537) == PLAN and build(t=0x7FFF8001) == PLAN
    assert build(nbytes=lib.rgcn_lp_index_workspace_bytes(5, 10, 3) - 1) == WS and build(ws=None) == NULL and build(t=0) == 0
    bwd = lambda t=5, g=p, np_=p, rp=p, dz=p, lddz=16, drel=p, lddr=16, ws=p, nbytes=1 << 30, w=16: lib.rgcn_lp_backward(
        p, 16, p, 16, w, 10, 3, p, p, p, t, g, np_, p, rp, p, dz, lddz, drel, lddr, ws, nbytes, None)
    assert bwd(g=None) == NULL and bwd(np_=None) == NULL and bwd(rp=None) == NULL and bwd(ws=None) == NULL
    assert bwd(lddz=12) == STRIDE and bwd(lddr=20, w=24) == STRIDE and bwd(dz=p + 8) == STRIDE
    assert bwd(nbytes=lib.rgcn_lp_backward_workspace_bytes(5, 3, 16) - 1) == WS
    assert bwd(t=0) == 0 and bwd(dz=None, drel=None) == 0 and bwd(t=-2) == ARG
    cor = lambda s=p, t=5, n=10, k=2, seed=0, out=p: lib.rgcn_lp_corrupt(s, s, s, t, n, k, seed, out, out, out, None)
    assert cor(s=None) == NULL and cor(out=None) == NULL
    assert cor(t=-1) == ARG and cor(n=0) == ARG and cor(k=0) == ARG and cor(seed=-1) == ARG
    assert cor(t=0x7FFF8001, k=3) == PLAN and cor(t=0) == 0
    rank = lambda a=p, q=5, fp=None, fi=None, fl=0, out=p, ws=p, nbytes=1 << 30, w=16, ld=16: lib.rgcn_lp_rank(
        p, ld, p, ld, w, 10, 3, a, a, a, q, fp, fi, fl, out, out, ws, nbytes, None)
    assert rank(a=None) == NULL and rank(out=None) == NULL and rank(ws=None) == NULL and rank(fp=p, fl=3) == NULL
    assert rank(q=-1) == ARG and rank(fp=p, fi=p, fl=-1) == ARG and rank(w=200, ld=200) == WIDTH and rank(ld=10) == STRIDE
    assert rank(nbytes=lib.rgcn_lp_rank_workspace_bytes(5, 10, 16) - 1) == WS and rank(q=0) == 0


def test_lp_workspace_queries():
    lib = _lib.load()
    a256 = lambda v: (v + 255) // 256 * 256
    # 0 on arguments the call would refuse
    for args in ((0, 10, 3), (-1, 10, 3), (5, -1, 3), (5, 10, -1), (5, 10, 65537), (0x7FFF8001, 10, 3)):
        assert lib.rgcn_lp_index_workspace_bytes(*args) == 0, args
    for args in ((0, 3, 16), (5, -1, 16), (5, 65537, 16), (5, 3, 0), (5, 3, 129), (0x7FFF8001, 3, 16)):
        assert lib.rgcn_lp_backward_workspace_bytes(*args) == 0, args
    for args in ((0, 10, 16), (-3, 10, 16), (5, -1, 16), (5, 10, 0), (5, 10, 129), (0xFFFF0001, 10, 16)):
        assert lib.rgcn_lp_rank_workspace_bytes(*args) == 0, args
    # the ranking pass writes no scores: its workspace is one float per query, whatever the number of entities
    assert lib.rgcn_lp_rank_workspace_bytes(10_000, 10 ** 3, 64) == lib.rgcn_lp_rank_workspace_bytes(10_000, 10 ** 7, 64) == a256(40_000)
    # the backward: chunk pointers and one partial row per chunk of 256 triples (at most T / 256 + R chunks)
    assert lib.rgcn_lp_backward_workspace_bytes(10_000, 32, 64) == a256(33 * 4) + a256((10_000 // 256 + 32) * 64 * 4)
    assert lib.rgcn_lp_backward_workspace_bytes(10_000, 32, 5) == a256(33 * 4) + a256((10_000 // 256 + 32) * 8 * 4)
    # monotone: a larger call's workspace holds a smaller call's
    sizes = [lib.rgcn_lp_index_workspace_bytes(t, 1000, 8) for t in (1, 100, 5000, 100_000)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    assert lib.rgcn_lp_index_workspace_bytes(100, 10 ** 7, 8) >= lib.rgcn_lp_index_workspace_bytes(100, 1000, 8)
    assert np.all(np.diff([lib.rgcn_lp_backward_workspace_bytes(t, 8, 64) for t in (1, 300, 5000)]) >= 0)
