"""What every unit of a packed tile-major weight-gradient plan (layout 5 after ``plan.dw_pack`` / ``dw_pack_kernel``) must satisfy,
and the per-stream count of halves (test helper, CPU only; used by test_dw_pack.py and test_gpu_dw_pack.py)."""
import numpy as np

from scaling_rgcn_training_amd import plan as P

PAIR_SLOTS = (0, 1, 2, 3, 32, 33, 34, 35)


def _np(plan):
    g = lambda f: getattr(plan, f).cpu().numpy()       # noqa: E731
    return {f: g(f) for f in ("slot_src", "slot_w", "slot_row", "slot_src2", "chunk_cnt", "chunk_tile", "chunk_flags", "chunk_rel",
                              "rel_order")}


def check_units(plan, walkers=P.DW_WALKERS):
    """The invariants of every unit in ``rel_order``; returns the number of units that straddle two tiles."""
    a, T, n_tiles = _np(plan), plan.tile, plan.n_tiles
    bounds = np.arange(walkers + 1) * n_tiles // walkers
    straddling = 0
    assert len(set(a["rel_order"].tolist())) == a["rel_order"].size
    for u in a["rel_order"].astype(np.int64):
        src, w, row = (a[f][64 * u:64 * u + 64] for f in ("slot_src", "slot_w", "slot_row"))
        s2, t, cnt = a["slot_src2"][8 * u:8 * u + 8], int(a["chunk_tile"][u]), int(a["chunk_cnt"][u])
        valid = src < plan.n_nodes
        assert valid.any() and cnt % 16 == 0 and 0 < cnt <= 64
        last = int(np.nonzero(valid)[0][-1])
        assert cnt - 16 <= last < cnt, (u, last, cnt)
        # padding: weight 0, row n_owned, source n_nodes
        assert (src[~valid] == plan.n_nodes).all() and (w[~valid] == 0).all() and (row[~valid] == plan.n_owned).all()
        assert (row[valid] >= 0).all() and (row[valid] < plan.n_owned).all() and (w[valid] != 0).all()
        # two tiles at most: chunk_tile = the earliest row's, and the next -- inside ONE walker range
        tiles = row[valid] // T
        assert tiles.min() == t and tiles.max() <= t + 1, (u, t, tiles.min(), tiles.max())
        p = np.searchsorted(bounds, t, side="right") - 1
        assert tiles.max() < bounds[p + 1], "a unit crosses a walker-range boundary"
        # half order: once half 0 holds a row of t + 1, half 1 holds nothing else
        h = [tiles[np.nonzero(valid)[0] < 32], tiles[np.nonzero(valid)[0] >= 32]]
        if (h[0] == t + 1).any():
            assert (h[1] == t + 1).all()
        # pairs: second rows only on the pair places, only where the place holds a head
        for k, pos in enumerate(PAIR_SLOTS):
            assert 0 <= s2[k] <= plan.n_nodes
            if s2[k] < plan.n_nodes:
                assert valid[pos]
        # chunk_flags bits 28-30 say which halves hold rows of t + 1
        a0, b0 = (h[0] == t).any(), (h[0] == t + 1).any()
        a1, b1 = (h[1] == t).any(), (h[1] == t + 1).any()
        want = ((P.DW_FLAG_H0_STRADDLES if a0 and b0 else 0) | (P.DW_FLAG_H1_STRADDLES if a1 and b1 else 0)
                | (P.DW_FLAG_H1_NEXT if b1 and not a1 and not b0 else 0))
        assert int(a["chunk_flags"][u]) & (7 << 28) == want, (u, hex(int(a["chunk_flags"][u])), hex(want))
        straddling += tiles.max() > t
    # units outside rel_order hold nothing
    used = np.zeros(plan.n_chunks, bool)
    used[a["rel_order"]] = True
    assert (a["chunk_cnt"][~used] == 0).all()
    assert (a["slot_src"].reshape(-1, 64)[~used] == plan.n_nodes).all() and (a["slot_src2"][:8 * plan.n_chunks].reshape(-1, 8)[~used] == plan.n_nodes).all()
    return straddling


def stream_stats(plan, walkers=P.DW_WALKERS):
    """Per stream (relation, walker range) of at least two tiles: (heads, non-empty halves, units closed early).  A unit that is
    not the stream's last and holds fewer than 64 heads was closed early (by the two-tile rule: nothing else closes one)."""
    a, n_tiles = _np(plan), plan.n_tiles
    order = a["rel_order"].astype(np.int64)
    key = a["chunk_rel"].astype(np.int64)[order] * max(n_tiles, 1) + a["chunk_tile"].astype(np.int64)[order]
    valid = (a["slot_src"] < plan.n_nodes).reshape(-1, 2, 32)
    out = []
    for r in range(plan.num_relations):
        for p in range(walkers):
            t0, t1 = p * n_tiles // walkers, (p + 1) * n_tiles // walkers
            if t1 - t0 < 2:
                continue
            i0, i1 = np.searchsorted(key, [r * n_tiles + t0, r * n_tiles + t1])
            v = valid[order[i0:i1]]
            per_unit = v.sum(axis=(1, 2))
            out.append((int(v.sum()), int(v.any(axis=2).sum()), int((per_unit[:-1] < 64).sum()) if len(per_unit) else 0))
    return out


def total_halves(plan):
    """32-slot halves the kernel walks: per unit in ``rel_order``, ceil(chunk_cnt / 32)"""
    c = plan.chunk_cnt.cpu().numpy().astype(np.int64)[plan.rel_order.cpu().numpy().astype(np.int64)]
    return int(((c + 31) // 32).sum())
