"""The argument contract of ``rgcn_nt_*`` (include/rgcn_mi355x.h): every refusal is answered before any launch -- the calls below
pass host dummy pointers or sizes with no memory behind them -- and the additions leave the ABI version alone."""
import ctypes as C

import pytest

from scaling_rgcn_training_amd import _lib

pytestmark = pytest.mark.gpu
NULL, PLAN, WORKSPACE, ARG = -1, -4, -6, -11
LIMIT = 0xFFFF0000
_DUMMY = (C.c_int64 * 64)()


def _p():
    return C.addressof(_DUMMY)


def test_size_queries():
    lib = _lib.load()
    for n in (0, 1, 4095, 4096, 4097, 10 ** 6, LIMIT):
        assert lib.rgcn_nt_lines_workspace_bytes(n) > 0 and lib.rgcn_nt_lines_workspace_bytes(n) % 256 == 0
    assert lib.rgcn_nt_lines_workspace_bytes(-1) == 0 and lib.rgcn_nt_lines_workspace_bytes(LIMIT + 1) == 0
    for n, lines in ((0, 0), (14, 1), (10 ** 6, 2049), (LIMIT, 10 ** 7)):
        got = lib.rgcn_nt_tokenize_workspace_bytes(n, lines)
        assert got > 0 and got % 256 == 0
    for n, lines in ((-1, 0), (10, -1), (10, 11), (LIMIT + 1, 5)):
        assert lib.rgcn_nt_tokenize_workspace_bytes(n, lines) == 0
    sizes = [lib.rgcn_nt_workspace_bytes(t) for t in (0, 1, 682, 683, 2048, 10 ** 6, LIMIT // 3)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes)
    assert lib.rgcn_nt_workspace_bytes(-1) == 0 and lib.rgcn_nt_workspace_bytes(LIMIT // 3 + 1) == 0


def test_lines_refusals():
    lib, p, out = _lib.load(), _p(), C.c_int64(-7)
    need = lib.rgcn_nt_lines_workspace_bytes(100)
    assert lib.rgcn_nt_lines(None, 100, p, need, C.byref(out), None) == NULL
    assert lib.rgcn_nt_lines(p, 100, p, need, None, None) == NULL
    assert lib.rgcn_nt_lines(p, 100, None, need, C.byref(out), None) == NULL
    assert lib.rgcn_nt_lines(p, -1, p, need, C.byref(out), None) == ARG
    assert lib.rgcn_nt_lines(p, LIMIT + 1, p, 1 << 40, C.byref(out), None) == PLAN          # no memory behind it
    assert lib.rgcn_nt_lines(p, 100, p, need - 1, C.byref(out), None) == WORKSPACE
    assert out.value == -7


def test_tokenize_refusals():
    lib, p = _lib.load(), _p()
    info = (C.c_int64 * 4)(-7, -7, -7, -7)
    need = lib.rgcn_nt_tokenize_workspace_bytes(100, 5)
    assert lib.rgcn_nt_tokenize(None, 100, 5, p, p, p, need, info, None) == NULL
    assert lib.rgcn_nt_tokenize(p, 100, 5, None, p, p, need, info, None) == NULL
    assert lib.rgcn_nt_tokenize(p, 100, 5, p, None, p, need, info, None) == NULL
    assert lib.rgcn_nt_tokenize(p, 100, 5, p, p, None, need, info, None) == NULL
    assert lib.rgcn_nt_tokenize(p, 100, 5, p, p, p, need, None, None) == NULL
    assert lib.rgcn_nt_tokenize(p, 100, -1, p, p, p, need, info, None) == ARG
    assert lib.rgcn_nt_tokenize(p, 100, 101, p, p, p, 1 << 40, info, None) == ARG
    assert lib.rgcn_nt_tokenize(p, LIMIT + 1, 5, p, p, p, 1 << 40, info, None) == PLAN
    assert lib.rgcn_nt_tokenize(p, 100, 5, p, p, p, need - 1, info, None) == WORKSPACE
    assert list(info) == [-7] * 4


def test_build_refusals():
    lib, p = _lib.load(), _p()
    counts = (C.c_int64 * 8)(*[-7] * 8)
    need = lib.rgcn_nt_workspace_bytes(10)

    def build(text=p, nbytes=100, off=p, length=p, t=10, max_len=8, bits=64, seed=0, ws=p, wsb=need, out=counts):
        return lib.rgcn_nt_build(text, nbytes, off, length, t, max_len, bits, seed, ws, wsb, out, None)

    assert build(text=None) == NULL and build(off=None) == NULL and build(length=None) == NULL and build(out=None) == NULL
    assert build(ws=None) == NULL
    for bits in (0, -1, 65, 1 << 20):
        assert build(bits=bits) == ARG
    assert build(nbytes=-1) == ARG and build(t=-1) == ARG and build(max_len=-1) == ARG and build(seed=-1) == ARG
    assert build(nbytes=LIMIT + 1, wsb=1 << 40) == PLAN                                     # no memory behind it
    assert build(t=LIMIT // 3 + 1, wsb=1 << 50) == PLAN
    assert build(wsb=need - 1) == WORKSPACE
    assert build(bits=1, wsb=need - 1) == WORKSPACE and build(bits=64, wsb=need - 1) == WORKSPACE       # 1 and 64 are accepted
    assert list(counts) == [-7] * 8


def test_emit_refusals():
    lib, p = _lib.load(), _p()
    need = lib.rgcn_nt_workspace_bytes(10)

    def emit(counts=(12, 8, 2, 1, 6, 2), t=10, ei=p, et=p, li=p, lb=p, tabs=(p,) * 6, ws=p, wsb=need):
        c = None if counts is None else (C.c_int64 * 8)(*counts, 0, 0)
        return lib.rgcn_nt_emit(t, c, ei, et, li, lb, *tabs, ws, wsb, None)

    assert emit(counts=None) == NULL and emit(ei=None) == NULL and emit(et=None) == NULL and emit(li=None) == NULL
    assert emit(lb=None) == NULL and emit(ws=None) == NULL
    for i in range(6):
        assert emit(tabs=tuple(None if j == i else p for j in range(6))) == NULL
    assert emit(t=-1) == ARG
    for bad in ((31, 8, 2, 1, 6, 2), (12, 13, 2, 1, 6, 2), (12, 8, 13, 1, 6, 2), (12, 8, 2, 13, 6, 2), (12, 8, 2, 1, 7, 2),
                (12, 8, 2, 1, 22, 2), (12, 8, 2, 1, 6, 9), (-1, 8, 2, 1, 6, 2), (12, 8, 2, 1, -2, 2)):
        assert emit(counts=bad) == ARG, bad
    assert emit(t=LIMIT // 3 + 1, wsb=1 << 50) == PLAN
    assert emit(wsb=need - 1) == WORKSPACE


def test_abi_version_and_status_string():
    lib = _lib.load()
    assert lib.rgcn_abi_version() == 19 == _lib.ABI_VERSION
    assert b"hash" in lib.rgcn_status_string(-12)
