"""Ranking sweeps past their first turn.  The grid of a ranking sweep is (query blocks, entity slices) with
``slices = min(ceil(1024 / qblocks), ceil(tiles / waves))`` (``rank_slices`` in csrc/rgcn_lp_shared.h, its copy in ``launch_rank`` of
csrc/rgcn_linkpred_wide.hip), and a wave comes back for another entity tile only where ``ceil(1024 / qblocks) < ceil(tiles / waves)``:
with at least 512 query blocks.  Every other ranking test stays below that, so the hand-over between two tiles -- ``te_tile`` leaving
slab 0 of ``next_rows`` in ``ent``, ``lpw_rank_kernel`` loading ``row_of(t + step)`` behind a tile's last slab -- only ever hands over
"no rows" there.  Here every case recomputes the launch numbers and asserts, before the kernel runs, that every wave takes at least
three turns (one slice) or that the two slices take different numbers of turns (two slices).

The reference stays small by a query pool: 300 distinct (anchor, r, target) queries on integer-valued tables, each with a short filter
list (none, only the target, three ids), ranked once by tests/linkpred_reference.py; the Q queries of a launch are pool entries drawn
with replacement, and every one of the Q outputs must EQUAL its entry's counts.  Queries with an id out of range (counts -1) sit in the
first, a middle and the last query block."""
import functools

import numpy as np
import pytest
import torch

from tests import kge_reference as K
from tests import linkpred_reference as R
from tests import test_gpu_linkpred as T
from tests.test_gpu_linkpred_edges import _short_lists

pytestmark = pytest.mark.gpu

BLOCKS = 1024            # kRankBlocks: the workgroups a launch aims at
POOL = 300
# (entity rows of a step, waves that share a slice's tiles): TransE's four waves all take every step of their workgroup
SWEEP = {"transe": (64, 1), "complex": (16, 8), "lp": (16, 8), "lpw": (16, 8)}


def _launch(n_q, n_nodes, wg_queries, rows, waves):
    """(qblocks, tiles, slices, step, turns[slice][wave]) of a sweep, from the launch formulas"""
    qblocks, tiles = -(-n_q // wg_queries), -(-n_nodes // rows)
    slices = max(1, min(-(-BLOCKS // qblocks), -(-tiles // waves)))
    step = slices * waves
    return qblocks, tiles, slices, step, [[len(range(y * waves + w, tiles, step)) for w in range(waves)] for y in range(slices)]


# Per kind of sweep and regime: (N, what the recomputed numbers must be).  Q is the smallest that gives the regime, plus 4 so that
# the last query block is ragged: 1,023 * QW + 5 (1,024 blocks, one slice) or 511 * QW + 5 (512 blocks, two slices).
#   64-row steps (TransE)
#     one      N 327 = 64 * 5 + 7:    6 tiles, step 1, 6 turns, the last of 7 rows
#     whole    N 256:                 4 tiles, step 1, 4 turns, no ragged tail
#     two      N 391 = 64 * 6 + 7:    7 tiles, step 2, slice 0 takes 4 turns, slice 1 takes 3 (the last of 7 rows is slice 0's)
#   16-row tiles, 8 waves (lp_rank_body: DistMult, ComplEx; lpw_rank_kernel)
#     one      N 421 = 128 * 3 + 37:  27 tiles, step 8, waves 0..2 take 4 turns, waves 3..7 take 3, the last tile has 5 rows
#     whole    N 384 = 128 * 3:       24 tiles, step 8, every wave 3 turns
#     two      N 677 = 16 * 42 + 5:   43 tiles, step 16, slice 0: 3 turns per wave (24), slice 1: 3, 3, 3, 2, 2, 2, 2, 2 (19)
NODES = {64: {"one": 327, "whole": 256, "two": 391}, 16: {"one": 421, "whole": 384, "two": 677}}
EXPECT = {(64, "one"): (6, 1, [[6]]), (64, "whole"): (4, 1, [[4]]), (64, "two"): (7, 2, [[4], [3]]),
          (16, "one"): (27, 8, [[4, 4, 4, 3, 3, 3, 3, 3]]), (16, "whole"): (24, 8, [[3] * 8]),
          (16, "two"): (43, 16, [[3] * 8, [3, 3, 3, 2, 2, 2, 2, 2]])}


def _shape(family, regime, wg_queries):
    rows, waves = SWEEP[family]
    n_nodes = NODES[rows][regime]
    n_q = (511 if regime == "two" else 1023) * wg_queries + 5
    qblocks, tiles, slices, step, turns = _launch(n_q, n_nodes, wg_queries, rows, waves)
    assert (tiles, step, turns) == EXPECT[rows, regime]
    if regime == "two":
        assert slices == 2 and 512 <= qblocks < BLOCKS and sum(turns[0]) != sum(turns[1]) and min(min(t) for t in turns) >= 2
        assert n_nodes % rows != 0
    else:
        assert slices == 1 and qblocks >= BLOCKS and min(turns[0]) >= 3
        assert (n_nodes % (rows * step) == 0) == (regime == "whole") and (n_nodes % rows != 0) == (regime == "one")
    assert n_q % wg_queries == 5                                   # a ragged last query block
    return n_q, n_nodes, qblocks


@functools.lru_cache(maxsize=None)
def _pool(family, side, width, n_nodes):
    """integer-valued tables, 300 distinct queries with short lists, and their exact counts"""
    g = torch.Generator().manual_seed(1000 * width + n_nodes)
    z = torch.randint(-3, 4, (n_nodes, width), generator=g).float()
    rel = torch.randint(-1, 2, (3, width), generator=g).float()
    q = torch.stack([torch.randint(0, n_nodes, (2 * POOL,), generator=g), torch.randint(0, 3, (2 * POOL,), generator=g),
                     torch.randint(0, n_nodes, (2 * POOL,), generator=g)], 1).numpy()
    _, first = np.unique(q, axis=0, return_index=True)
    q = q[np.sort(first)[:POOL]]
    assert q.shape == (POOL, 3) and len(np.unique(q, axis=0)) == POOL
    a, r, e = q[:, 0], q[:, 1], q[:, 2]
    lists = _short_lists(n_nodes, POOL, e, seed=width + n_nodes)
    if family in ("transe", "complex"):
        sc, _ = K.rank_scores(family, z.numpy(), rel.numpy(), a, r, side)
    else:
        sc, _ = R.rank_scores(z, rel, a, r)
    assert np.abs(sc).max() < 2 ** 24 and (sc == np.round(sc)).all()
    greater, equal = R.rank_counts(sc, e, lists)
    assert greater.max() > 10 and equal.sum() > 0 and len(np.unique(greater)) > 20
    lens = np.array([len(x) for x in lists])
    padded = np.zeros((POOL, 3), dtype=np.int64)
    for i, ids in enumerate(lists):
        padded[i, :len(ids)] = ids
    return z, rel, a, r, e, lens, padded, greater, equal


def _queries(pool, n_q, n_nodes, qblocks, wg_queries):
    """Q draws from the pool, their CSR lists and expected counts; ids out of range in the first, a middle and the last block"""
    z, rel, a, r, e, lens, padded, greater, equal = pool
    pick = np.random.default_rng(n_q + n_nodes).integers(0, POOL, n_q)
    a, r, e, want_g, want_e = a[pick].copy(), r[pick].copy(), e[pick].copy(), greater[pick].copy(), equal[pick].copy()
    ptr = np.zeros(n_q + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(lens[pick])
    idx = padded[pick][np.arange(3)[None, :] < lens[pick][:, None]]
    assert len(idx) == ptr[-1]
    mid = (qblocks // 2) * wg_queries
    bad = [0, 5, wg_queries - 1, mid + 3, mid + 17, n_q - 4, n_q - 1]
    assert bad[2] // wg_queries == 0 and bad[3] // wg_queries == qblocks // 2 and bad[5] // wg_queries == qblocks - 1
    for j, i in enumerate(bad):
        kind = j % 4
        if kind == 0:
            a[i] = n_nodes
        elif kind == 1:
            r[i] = 3
        elif kind == 2:
            e[i] = -1
        else:
            a[i], e[i] = 2 ** 40, n_nodes + 15
        want_g[i] = want_e[i] = -1
    return a, r, e, ptr, idx, want_g, want_e


def _check(family, side, width, regime, wg_queries, call):
    n_q, n_nodes, qblocks = _shape(family, regime, wg_queries)
    pool = _pool(family, side, width, n_nodes)
    a, r, e, ptr, idx, want_g, want_e = _queries(pool, n_q, n_nodes, qblocks, wg_queries)
    got_g, got_e = call(T._input(pool[0]), T._input(pool[1]), T._ids(a), T._ids(r), T._ids(e), T._ids(ptr), T._ids(idx))
    got_g, got_e = got_g.cpu().numpy(), got_e.cpu().numpy()
    for name, got, want in (("greater", got_g, want_g), ("equal", got_e, want_e)):
        wrong = np.flatnonzero(got != want)
        assert len(wrong) == 0, (f"{family} {side} width {width} {regime}: {name} differs for {len(wrong)} of {n_q} queries", wrong[:8],
                                 got[wrong[:8]], want[wrong[:8]])


REGIMES = ["one", "whole", "two"]


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("width", [20, 128])
@pytest.mark.parametrize("code,side", [(0, "object"), (1, "subject")])
def test_transe_sweep_takes_several_turns(code, side, width, regime):
    lib = T._lib()
    _check("transe", side, width, regime, 64, lambda *args: lib.kge_rank(lib.KGE_TRANSE_L1, code, *args))


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("code,side", [(0, "object"), (1, "subject")])
def test_complex_sweep_takes_several_turns(code, side, regime):
    lib = T._lib()
    _check("complex", side, 20, regime, 64, lambda *args: lib.kge_rank(lib.KGE_COMPLEX, code, *args))


# one slab with a ragged last step (k16 = 9), two slabs (17), four slabs (25)
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("wg_queries", [32, 64])
@pytest.mark.parametrize("width", [132, 260, 388])
def test_wide_sweep_takes_several_turns(width, wg_queries, regime):
    lib = T._lib()
    _check("lpw", "object", width, regime, wg_queries, lambda *args: lib.lpw_rank(*args, wg_queries=wg_queries))


@pytest.mark.parametrize("regime", REGIMES)
def test_narrow_sweep_takes_several_turns(regime):
    _check("lp", "object", 20, regime, 64, T._lib().lp_rank)
