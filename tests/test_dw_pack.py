"""plan.dw_pack, the torch twin of dw_pack_kernel (csrc/rgcn_plan.hip): the tile-major weight-gradient plan with the heads of every
(relation, walker range) stream packed across tile boundaries -- on the CPU, at the headline density (Poisson(0.3125) edges per
(destination, relation)) with 520 tiles of 320 rows, about 8 per walker range."""
import numpy as np
import pytest
import torch

from oracle import rgcn_oracle as O
from scaling_rgcn_training_amd import plan as P
from tests import dw_pack_checks as C
from tests.plan_emulator import emulate_dw

N, E, R, T = 166_400, 1_664_000, 32, 320
# A unit is closed early only where a stream's next head lies more than one tile past the unit's first -- a relation absent from a
# whole tile.  Here a (tile, relation) group expects 100 edges: none is empty, so no unit may close early.
EARLY_CLOSED_CAP = 0


@pytest.fixture(scope="module")
def packed():
    ei, et = O.synthetic_graph(N, E, R, seed=11)
    w = P.edge_weights(ei[0], ei[1], et, R)
    before = P.dw_pairs(P.build_plan(ei[0], ei[1], et, w, N, R, T, chunk=64))
    plan = P.build_plan(ei[0], ei[1], et, w, N, R, T, chunk=64, split=5)
    return ei, et, before, plan


def test_every_unit_meets_the_invariants(packed):
    _, _, _, plan = packed
    assert plan.layout == 5 and plan.tile == T and plan.n_tiles == 520
    assert C.check_units(plan) > 1000, "hardly a unit straddles: the case tests nothing"


def test_streams_are_dense(packed):
    _, _, before, plan = packed
    stats = C.stream_stats(plan)
    assert len(stats) == R * P.DW_WALKERS
    for heads, halves, early in stats:
        assert halves <= -(-heads // 32) + 1 + early, (heads, halves, early)
    assert sum(s[2] for s in stats) <= EARLY_CLOSED_CAP
    hb, ha = C.total_halves(before), C.total_halves(plan)
    print(f"halves: {hb} before packing, {ha} after ({ha / hb:.3f})")
    assert ha < 0.93 * hb      # ~3.12 -> ~2.8 halves per (tile, relation) group


def test_packed_plan_computes_the_weight_gradient(packed):
    ei, et, _, plan = packed
    w, root, bias = O.synthetic_params(R, 64, 64, seed=3)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, 64, generator=g)
    dg = torch.randn(N, 64, generator=g)
    _, gr = O.rgcn_conv_segments(x.numpy(), ei.numpy(), et.numpy(), w.numpy(), root.numpy(), bias.numpy(), dg.numpy())
    dw = emulate_dw(plan, x.numpy(), dg.numpy(), R + 1, 64, 64)
    ref = np.asarray(gr["weight"], np.float64)
    # float64 sums on both sides; the plan's weights are 1 / count rounded to fp32 (relative error <= 2^-24 each) where the oracle
    # divides in float64: every product is off by at most 2^-24 of its magnitude, their sum by 2^-24 of the sum of magnitudes
    # (abs_condition).  1e-9: two float64 summation orders of ~50,000 products of magnitude ~1.
    from oracle.tolerance import abs_condition
    _, c = abs_condition(x, ei, et, w, root, bias, dg)
    err = np.abs(dw[:R] - ref)
    print(f"packed plan against the oracle: worst error {err.max():.3e}, bound there {(2.0 ** -24 * c['weight'] + 1e-9).flat[err.argmax()]:.3e}")
    assert (err <= 2.0 ** -24 * np.asarray(c["weight"], np.float64) + 1e-9).all()
    # (the root pseudo relation, id R: its units are not the tile-major kernel's and stay unpacked -- weight 1, exact)
    assert (np.abs(dw[R] - np.asarray(gr["root"], np.float64)) <= 1e-9).all()


def test_short_ranges_stay_as_dw_pairs_left_them():
    """fewer tiles than walkers: every walker range holds one tile at most, nothing to pack -- every array bit for bit"""
    n, e, r = 6000, 60000, 32
    ei, et = O.synthetic_graph(n, e, r, seed=n + e)
    w = P.edge_weights(ei[0], ei[1], et, r)
    a = P.dw_pairs(P.build_plan(ei[0], ei[1], et, w, n, r, T, chunk=64))
    b = P.build_plan(ei[0], ei[1], et, w, n, r, T, chunk=64, split=5)
    for f in ("tile_ptr", "chunk_rel", "chunk_cnt", "chunk_tile", "chunk_flags", "rel_order", "slot_src", "slot_w", "slot_row", "slot_src2"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
