"""The host side of link prediction on rows wider than 128 (``DistMult(..., wide=True)``, the argument checks of
csrc/rgcn_linkpred_wide.hip): everything here is answered before a kernel is launched, so it runs without a GPU."""
import ctypes

import pytest
import torch

from scaling_rgcn_training_amd import _lib
from scaling_rgcn_training_amd import linkpred as L

NULL, WIDTH, STRIDE, PLAN, WS, ARG = -1, -2, -3, -4, -6, -11
_BUF = (ctypes.c_float * 1024)()


def _p():
    a = ctypes.addressof(_BUF)
    return a + (-a % 16)            # a 16-byte aligned host address the checks see as non-NULL and never read


def test_distmult_wide_arguments():
    for args, kw in (((3, 129), {}), ((3, 129), dict(wide=False)), ((3, 513), dict(wide=True)), ((3, 0), dict(wide=True)),
                     ((3, 8), dict(wide=1)), ((3, 8), dict(wide="yes"))):
        with pytest.raises(ValueError):
            L.DistMult(*args, **kw)
    dec = L.DistMult(3, 512, wide=True)
    assert dec.rel.shape == (3, 512) and dec.rel.requires_grad and dec.family == "lpw"
    assert L.DistMult(3, 129, wide=True).family == "lpw" and L.DistMult(3, 128, wide=True).family == "lp"
    ids = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError):
        dec(torch.zeros(5, 500), ids, ids, ids)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # a missing GPU is an error, never a torch formulation
        dec(torch.zeros(5, 512), ids, ids, ids)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.ranks(torch.zeros(5, 512), dec, ids, ids, ids)
    with pytest.raises(ValueError):
        L._padded(torch.zeros(2, 129))                              # the narrow limit is the default


def test_lpw_argument_refusals():
    lib, p = _lib.load(), _p()
    score = lambda z=p, ldz=512, rel=p, ldr=512, w=500, n=10, nr=3, s=p, t=5, out=p: lib.rgcn_lpw_score(z, ldz, rel, ldr, w, n, nr, s, s, s,
                                                                                                     t, out, None, None)
    assert score(z=None) == NULL and score(rel=None) == NULL and score(s=None) == NULL and score(out=None) == NULL
    assert score(w=0) == WIDTH and score(w=513, ldz=1024, ldr=1024) == WIDTH
    assert score(ldz=498) == STRIDE and score(ldr=496) == STRIDE and score(w=129, ldz=128) == STRIDE and score(z=p + 4) == STRIDE
    assert score(t=-1) == ARG and score(n=-1) == ARG and score(nr=65537) == PLAN and score(t=0x7FFF8001) == PLAN
    assert score(t=0) == 0 and score(t=0, s=None, out=None) == 0 and score(t=0, w=512) == 0      # nothing to do: no launch
    bwd = lambda t=5, g=p, np_=p, rp=p, dz=p, lddz=512, drel=p, lddr=512, ws=p, nbytes=1 << 30, w=500: lib.rgcn_lpw_backward(
        p, 512, p, 512, w, 10, 3, p, p, p, t, g, np_, p, rp, p, dz, lddz, drel, lddr, ws, nbytes, None)
    assert bwd(g=None) == NULL and bwd(np_=None) == NULL and bwd(rp=None) == NULL and bwd(ws=None) == NULL
    assert bwd(w=513) == WIDTH and bwd(w=0) == WIDTH
    assert bwd(lddz=496) == STRIDE and bwd(lddr=502) == STRIDE and bwd(dz=p + 8) == STRIDE and bwd(drel=p + 4) == STRIDE
    assert bwd(nbytes=lib.rgcn_lpw_backward_workspace_bytes(5, 3, 500) - 1) == WS
    assert bwd(t=0) == 0 and bwd(dz=None, drel=None) == 0 and bwd(t=-2) == ARG and bwd(t=0x7FFF8001) == PLAN
    rank = lambda a=p, q=5, fp=None, fi=None, fl=0, out=p, ws=p, nbytes=1 << 30, w=500, ld=512, wg=0: lib.rgcn_lpw_rank(
        p, ld, p, ld, w, 10, 3, a, a, a, q, fp, fi, fl, out, out, wg, ws, nbytes, None)
    assert rank(a=None) == NULL and rank(out=None) == NULL and rank(ws=None) == NULL and rank(fp=p, fl=3) == NULL
    assert rank(q=-1) == ARG and rank(fp=p, fi=p, fl=-1) == ARG and rank(wg=16) == ARG and rank(wg=-1) == ARG
    assert rank(w=513, ld=1024) == WIDTH and rank(w=0) == WIDTH and rank(ld=498) == STRIDE and rank(w=300, ld=296) == STRIDE
    assert rank(q=0xFFFF0001) == PLAN
    assert rank(nbytes=lib.rgcn_lpw_rank_workspace_bytes(5, 10, 500) - 1) == WS and rank(q=0) == 0 and rank(q=0, wg=32) == 0


def test_lpw_workspace_queries():
    lib = _lib.load()
    a256 = lambda v: (v + 255) // 256 * 256
    for args in ((0, 3, 500), (5, -1, 500), (5, 65537, 500), (5, 3, 0), (5, 3, 513), (0x7FFF8001, 3, 500)):
        assert lib.rgcn_lpw_backward_workspace_bytes(*args) == 0, args
    for args in ((0, 10, 500), (-3, 10, 500), (5, -1, 500), (5, 10, 0), (5, 10, 513), (0xFFFF0001, 10, 500)):
        assert lib.rgcn_lpw_rank_workspace_bytes(*args) == 0, args
    # the ranking pass writes no scores: one float per query, whatever the number of entities
    assert lib.rgcn_lpw_rank_workspace_bytes(10_000, 10 ** 3, 500) == lib.rgcn_lpw_rank_workspace_bytes(10_000, 10 ** 7, 500) == a256(40_000)
    # the backward: chunk pointers and one partial row per chunk of 256 triples (at most T / 256 + R chunks)
    assert lib.rgcn_lpw_backward_workspace_bytes(10_000, 32, 512) == a256(33 * 4) + a256((10_000 // 256 + 32) * 512 * 4)
    assert lib.rgcn_lpw_backward_workspace_bytes(10_000, 32, 257) == a256(33 * 4) + a256((10_000 // 256 + 32) * 260 * 4)
