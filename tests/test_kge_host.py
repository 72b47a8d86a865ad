"""The host side of the ComplEx and TransE decoders (``linkpred.ComplEx`` / ``TransE``, the argument checks of csrc/rgcn_kge.hip;
DESIGN.md 22): everything here is answered before a kernel is launched, so it runs without a GPU.  The counterpart of
tests/test_linkpred_wide_host.py, with its host-pointer trick.  One argument is changed per call, so nothing is pinned about the order
of the checks beyond what include/rgcn_mi355x.h states."""
import ctypes

import pytest
import torch

from scaling_rgcn_training_amd import _lib
from scaling_rgcn_training_amd import linkpred as L

NULL, WIDTH, STRIDE, PLAN, WS, ARG = -1, -2, -3, -4, -6, -11
CX, TE = _lib.KGE_COMPLEX, _lib.KGE_TRANSE_L1
DECODERS = [CX, TE]
_BUF = (ctypes.c_float * 1024)()


def _p():
    a = ctypes.addressof(_BUF)
    return a + (-a % 16)            # a 16-byte aligned host address the checks see as non-NULL and never read


def _score(dec, z="p", ldz=16, rel="p", ldr=16, w=16, n=10, nr=3, s="p", t=5, out="p"):
    p = _p()
    z, rel, s, out = (p if v == "p" else v for v in (z, rel, s, out))
    return _lib.load().rgcn_kge_score(dec, z, ldz, rel, ldr, w, n, nr, s, s, s, t, out, None, None)


def _bwd(dec, z="p", ldz=16, rel="p", ldr=16, w=16, n=10, nr=3, s="p", t=5, g="p", np_="p", ns="p", rp="p", rt="p", dz="p", lddz=16,
         drel="p", lddr=16, ws="p", nbytes=1 << 30):
    p = _p()
    z, rel, s, g, np_, ns, rp, rt, dz, drel, ws = (p if v == "p" else v for v in (z, rel, s, g, np_, ns, rp, rt, dz, drel, ws))
    return _lib.load().rgcn_kge_backward(dec, z, ldz, rel, ldr, w, n, nr, s, s, s, t, g, np_, ns, rp, rt, dz, lddz, drel, lddr, ws, nbytes,
                                         None)


def _rank(dec, side=0, z="p", ld=16, rel="p", w=16, n=10, nr=3, a="p", q=5, fp=None, fi=None, fl=0, out="p", ws="p", nbytes=1 << 30):
    p = _p()
    z, rel, a, out, ws = (p if v == "p" else v for v in (z, rel, a, out, ws))
    return _lib.load().rgcn_kge_rank(dec, side, z, ld, rel, ld, w, n, nr, a, a, a, q, fp, fi, fl, out, out, ws, nbytes, None)


@pytest.mark.parametrize("dec", DECODERS)
def test_kge_score_refusals(dec):
    p = _p()
    assert _score(dec, z=None) == NULL and _score(dec, rel=None) == NULL and _score(dec, s=None) == NULL and _score(dec, out=None) == NULL
    assert _score(dec, w=0) == WIDTH and _score(dec, w=129, ldz=256, ldr=256) == WIDTH
    assert _score(dec, ldz=12) == STRIDE and _score(dec, ldr=18) == STRIDE and _score(dec, w=6, ldz=4, ldr=8) == STRIDE
    assert _score(dec, z=p + 4) == STRIDE and _score(dec, rel=p + 8) == STRIDE
    assert _score(dec, t=-1) == ARG and _score(dec, n=-1) == ARG and _score(dec, nr=-1) == ARG
    assert _score(dec, nr=65537) == PLAN and _score(dec, t=0x7FFF8001) == PLAN
    assert _score(dec, t=0) == 0 and _score(dec, t=0, s=None, out=None) == 0 and _score(dec, t=0, w=128, ldz=128, ldr=128) == 0


@pytest.mark.parametrize("dec", DECODERS)
def test_kge_backward_refusals(dec):
    p, lib = _p(), _lib.load()
    assert _bwd(dec, z=None) == NULL and _bwd(dec, rel=None) == NULL and _bwd(dec, s=None) == NULL and _bwd(dec, g=None) == NULL
    assert _bwd(dec, np_=None) == NULL and _bwd(dec, ns=None) == NULL and _bwd(dec, rp=None) == NULL and _bwd(dec, rt=None) == NULL
    assert _bwd(dec, ws=None) == NULL
    assert _bwd(dec, w=0) == WIDTH and _bwd(dec, w=129, ldz=256, ldr=256, lddz=256, lddr=256) == WIDTH
    assert _bwd(dec, ldz=12) == STRIDE and _bwd(dec, ldr=18) == STRIDE and _bwd(dec, lddz=12) == STRIDE and _bwd(dec, lddr=18) == STRIDE
    assert _bwd(dec, lddr=20, w=24, ldz=24, ldr=24, lddz=24) == STRIDE
    assert _bwd(dec, z=p + 4) == STRIDE and _bwd(dec, dz=p + 8) == STRIDE and _bwd(dec, drel=p + 4) == STRIDE
    assert _bwd(dec, t=-2) == ARG and _bwd(dec, n=-1) == ARG and _bwd(dec, nr=65537) == PLAN and _bwd(dec, t=0x7FFF8001) == PLAN
    assert _bwd(dec, nbytes=lib.rgcn_kge_backward_workspace_bytes(dec, 5, 3, 16) - 1) == WS
    assert _bwd(dec, t=0) == 0 and _bwd(dec, dz=None, drel=None) == 0 and _bwd(dec, t=0, s=None, g=None, np_=None, rp=None, ws=None) == 0
    # a NULL gradient asks for nothing of its half: no index pointers, no stride, and (dz alone) no workspace
    assert _bwd(dec, dz=None, np_=None, ns=None, lddz=0, nbytes=0) == WS and _bwd(dec, dz=None, drel=None, ws=None, nbytes=0) == 0


@pytest.mark.parametrize("dec", DECODERS)
def test_kge_rank_refusals(dec):
    p, lib = _p(), _lib.load()
    assert _rank(dec, z=None) == NULL and _rank(dec, rel=None) == NULL and _rank(dec, a=None) == NULL and _rank(dec, out=None) == NULL
    assert _rank(dec, ws=None) == NULL and _rank(dec, fp=p, fl=3) == NULL
    assert _rank(dec, w=0) == WIDTH and _rank(dec, w=129, ld=256) == WIDTH and _rank(dec, w=200, ld=200) == WIDTH
    assert _rank(dec, ld=10) == STRIDE and _rank(dec, w=20, ld=16) == STRIDE and _rank(dec, z=p + 4) == STRIDE
    assert _rank(dec, side=-1) == ARG and _rank(dec, side=2) == ARG and _rank(dec, side=1, q=0) == 0
    assert _rank(dec, q=-1) == ARG and _rank(dec, fp=p, fi=p, fl=-1) == ARG and _rank(dec, n=-1) == ARG
    assert _rank(dec, q=0xFFFF0001) == PLAN and _rank(dec, nr=65537) == PLAN
    for side in (0, 1):
        assert _rank(dec, side=side, nbytes=lib.rgcn_kge_rank_workspace_bytes(dec, 5, 10, 16) - 1) == WS
        assert _rank(dec, side=side, q=0) == 0 and _rank(dec, side=side, q=0, a=None, out=None, ws=None, nbytes=0) == 0


def test_kge_decoder_and_width():
    """an unknown decoder is RGCN_ERR_ARG at every entry point; ComplEx refuses odd widths (a column pair per component), TransE
    takes every width 1..128"""
    for call in (_score, _bwd, _rank):
        assert call(-1) == ARG and call(2) == ARG and call(0x7FFFFFFF) == ARG
        for w in (1, 5, 15, 127):
            ld = (w + 3) // 4 * 4
            kw = dict(ld=ld) if call is _rank else dict(ldz=ld, ldr=ld)
            if call is _bwd:
                kw.update(lddz=ld, lddr=ld)
            zero = dict(q=0) if call is _rank else dict(t=0)
            assert call(CX, w=w, **kw) == WIDTH and call(CX, w=w, **kw, **zero) == WIDTH
            assert call(TE, w=w, **kw, **zero) == 0                # no WIDTH error; nothing to do, so no launch either
            assert call(CX, w=w + 1, **kw, **zero) == 0
        assert call(TE, w=129, **(dict(ld=256) if call is _rank else dict(ldz=256, ldr=256))) == WIDTH


def test_kge_workspace_queries():
    lib = _lib.load()
    a256 = lambda v: (v + 255) // 256 * 256
    for dec in DECODERS:
        # 0 on arguments the call would refuse
        for args in ((0, 3, 16), (-1, 3, 16), (5, -1, 16), (5, 65537, 16), (5, 3, 0), (5, 3, 129), (0x7FFF8001, 3, 16)):
            assert lib.rgcn_kge_backward_workspace_bytes(dec, *args) == 0, args
        for args in ((0, 10, 16), (-3, 10, 16), (5, -1, 16), (5, 10, 0), (5, 10, 129), (0xFFFF0001, 10, 16)):
            assert lib.rgcn_kge_rank_workspace_bytes(dec, *args) == 0, args
        # where they accept: rgcn_lp_*'s formulas -- one float per query whatever the number of entities; chunk pointers and one
        # partial row per chunk of 256 triples (at most T / 256 + R chunks)
        for q, n in ((1, 10), (5, 10), (10_000, 10 ** 3), (10_000, 10 ** 7)):
            assert lib.rgcn_kge_rank_workspace_bytes(dec, q, n, 64) == lib.rgcn_lp_rank_workspace_bytes(q, n, 64) == a256(4 * q)
        assert lib.rgcn_kge_rank_workspace_bytes(dec, 10_000, 10 ** 3, 2) == lib.rgcn_kge_rank_workspace_bytes(dec, 10_000, 2 ** 31 - 1, 128)
        for t, r, w in ((1, 1, 2), (10_000, 32, 64), (10_000, 32, 6), (257 * 5, 5, 20), (300, 65536, 128)):
            assert lib.rgcn_kge_backward_workspace_bytes(dec, t, r, w) == lib.rgcn_lp_backward_workspace_bytes(t, r, w) \
                == a256((r + 1) * 4) + a256((t // 256 + r) * ((w + 3) // 4 * 4) * 4), (t, r, w)
    # an unknown decoder, an odd ComplEx width (TransE takes it)
    for dec in (-1, 2, 7):
        assert lib.rgcn_kge_backward_workspace_bytes(dec, 5, 3, 16) == 0 and lib.rgcn_kge_rank_workspace_bytes(dec, 5, 10, 16) == 0
    for w in (1, 5, 127):
        assert lib.rgcn_kge_backward_workspace_bytes(CX, 5, 3, w) == 0 and lib.rgcn_kge_rank_workspace_bytes(CX, 5, 10, w) == 0
        assert lib.rgcn_kge_backward_workspace_bytes(TE, 5, 3, w) == lib.rgcn_lp_backward_workspace_bytes(5, 3, w) > 0
        assert lib.rgcn_kge_rank_workspace_bytes(TE, 5, 10, w) == a256(20)


def test_kge_module_arguments():
    for make, args in ((L.ComplEx, (3, 5)), (L.ComplEx, (3, 130)), (L.ComplEx, (3, 0)), (L.TransE, (3, 0)), (L.TransE, (3, 129)),
                       (L.TransE, (0, 8)), (L.ComplEx, (0, 8)), (L.TransE, (65537, 8)), (L.TransE, (3, 8.0)), (L.ComplEx, (3, "8")),
                       (L.TransE, (3, True)), (L.ComplEx, (True, 8)), (L._KgeDecoder, (3, 0)), (L._KgeDecoder, (3.0, 8))):
        with pytest.raises(ValueError):
            make(*args)
    bound = (6 / (3 + 8)) ** 0.5                                      # xavier_uniform_
    for make, code in ((L.ComplEx, CX), (L.TransE, TE)):
        dec = make(3, 8)
        assert dec.rel.shape == (3, 8) and dec.rel.requires_grad and dec.code == code and float(dec.rel.detach().abs().max()) <= bound
        assert dec.index_builds == {"node": 0, "relation": 0}
        ids = torch.zeros(4, dtype=torch.int64)
        for z in (torch.zeros(5, 7), torch.zeros(5, 8, 1), torch.zeros(8), torch.zeros(5, 8, dtype=torch.float64),
                  torch.zeros(5, 8, dtype=torch.float16), [[0.0] * 8]):
            with pytest.raises(ValueError):
                dec(z, ids, ids, ids)
        with pytest.raises(ValueError):
            dec(torch.zeros(5, 8), ids, ids, ids[:3])
        with pytest.raises(ValueError):
            dec(torch.zeros(5, 8), ids.int(), ids, ids)
        with pytest.raises(RuntimeError, match="no CPU fallback"):      # a missing GPU is an error, never a torch formulation
            dec(torch.zeros(5, 8), ids, ids, ids)
        for side in ("object", "subject"):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                L.ranks(torch.zeros(5, 8), dec, ids, ids, ids, side)
        with pytest.raises(ValueError, match="side"):
            L.ranks(torch.zeros(5, 8), dec, ids, ids, ids, side="both")
        with pytest.raises(ValueError):
            L.ranks(torch.zeros(5, 6), dec, ids, ids, ids)
        with pytest.raises(ValueError, match="another number"):
            L.ranks(torch.zeros(5, 8), dec, ids, ids, ids, filter=L.FilterIndex(torch.zeros(0, 3, dtype=torch.int64), 6, 3))
        dec.check()
    assert L.TransE(3, 7).rel.shape == (3, 7) and L.ComplEx(3, 128).rel.shape == (3, 128) and L.TransE(65536, 1).rel.shape == (65536, 1)
