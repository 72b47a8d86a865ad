"""RGCNConv(aggr="max") past 2^24 segments and 4 GiB: the only layer whose edge-parallel kernels gather a matrix that large.

A max layer has one row of H, T, Z and dH per (destination, relation) SEGMENT and one row of C per edge, so with N <= 2^24 nodes
(the most build_max_plan admits) the matrix rgcn_ep_transform and rgcn_bwd_dw gather from -- H -- passes 2^24 rows and 4 GiB
while x does not.  Those two pick buffer descriptors (32-bit offsets, __umul24 rows) or 64-bit pointers from buffer_bytes(rows,
ld); rgcn_segment_max / rgcn_segment_max_bwd address every row with 64-bit offsets.  Here the real size of H, not a flag, picks
the path (S = segments, N = nodes):

  A1 / A2  N 2^22, S 2^24 - 3 / 2^24 - 2, 64 -> 64   H the last addressable / first unaddressable matrix: the bf16 x 3 transform
                                                     and the direct d_weight kernel / the exact transform and the ring d_weight
                                                     kernel with pointers; with split_producers and without
  B        N 2^22, S 2^24 + 4099, 16 -> 16           H is 1 GiB: the row rule alone keeps it off the descriptors; integer features
                                                     (ties, maxima of 0: N = T + 1 at scale)
  C        N 2^23, S 2^25 + 4099, 64 -> 64           more than 2^31 elements in H, T, dH and C
  D        N 2^24, 64 -> 64                          the largest N: x is exactly 4 GiB and not addressable, the backward pseudo slots
                                                     pad with 2^24; one more node is refused
  E1 / E2  N 8,388,606 / 8,388,607, 16 -> 128        x addressable, g addressable / not by its width (the dH transform gathers g)

A to C: tests/max_reference.py exact_segment_graph (S exact to the row, one segment of 70,000 rows and one source with 70,000
out-edges -- three levels of PIECE = 256 each way --, the last node as source and destination, the last segment not empty,
duplicate triples, a dead relation); D and E: make_graph of tests/test_gpu_past_4gib.py.  Each case asserts its regime from its
inputs, then compares WHOLE tensors on the device, in row blocks:

  1. H and T of every segment, bit for bit, against torch's fp32 scatter_reduce amax and the plain count of the edges that attain it;
  2. C of every segment row from rgcn_segment_max_bwd on a random dH: equal (as values, no NaN) to
     where(x[src] == H[s], (w dH[seg_dh[s]]) / (T[s] + (H[s] == 0)), 0) by torch ops -- one correctly rounded fp32 product and one
     correctly rounded fp32 quotient on either side, in the same order;
  3. the module with its defaults against float64 (max_reference.blocked_layer: per relation, torch autograd's tie rule, nothing
     shared with the plans): out, d_x, d_weight, d_root, d_bias under check() of tests/test_gpu_past_4gib.py.

Raw-ABI outputs start as NaN; every case prints its peak device memory."""
import pytest
import torch

from tests import kernel_variants as K
from tests import max_reference as M
from tests.test_gpu_past_4gib import BLK, SPLIT, Ref, _dev, _release, check, make_features, make_graph, make_params, nan_like

pytestmark = pytest.mark.gpu

EXTRA = 200_000             # rows beyond one per segment (exact_segment_graph), + 2 x 70,000 hub rows + 50,000 duplicates
EXTRA_TIES = 4_000_000      # the 16-column case: a fifth of the segments hold two rows or more, so T > 1 is common


@pytest.fixture(autouse=True)
def _free_between_cases():
    """every case holds tens of GB: nothing of the previous one may stay alive"""
    _release()
    torch.cuda.reset_peak_memory_stats()
    yield
    print(f"\npeak device memory: {torch.cuda.max_memory_allocated() / 1e9:.1f} GB")
    _release()


# ---- check 1: H and T ---------------------------------------------------------------------------------------------------------
def check_h_t(mp, G, x, din, h, t):
    """H, T [n_seg, ld] of _lib.max_aggregate against torch, relation by relation (segments are sorted by (relation, destination)),
    as int32 views: every segment, every column"""
    hh, n, r = mp.ep.heavy, G["n"], G["r"]
    sd = mp.seg_dh.long()
    rel = hh.unit_rel.repeat_interleave(64)[sd].long()
    dst = hh.slot_row[sd].long()
    del sd
    assert bool((rel[1:] * n + dst[1:] > rel[:-1] * n + dst[:-1]).all()), "segments sorted by (relation, destination), all distinct"
    seg_cnt = torch.bincount(rel, minlength=r).tolist()
    del rel
    assert h.shape[0] == t.shape[0] == mp.n_seg == sum(seg_cnt)
    lo = 0
    for q, (elo, ehi) in enumerate(G["bounds"]):
        hi = lo + seg_cnt[q]
        if ehi == elo:
            assert hi == lo, f"relation {q} has segments without an edge"
            continue
        src, de = G["src_s"][elo:ehi], G["dst_s"][elo:ehi]
        xs = x[src][:, :din]
        href = x.new_zeros(n, din).scatter_reduce(0, de[:, None].expand(-1, din), xs, "amax", include_self=False)
        tref = torch.zeros_like(href).index_add_(0, de, (xs == href[de]).float())
        d = dst[lo:hi]
        assert int(torch.bincount(de, minlength=n).count_nonzero()) == hi - lo, f"relation {q}: segments against destinations"
        bad_h = int((h[lo:hi, :din].view(torch.int32) != href[d].view(torch.int32)).sum())
        bad_t = int((t[lo:hi, :din].view(torch.int32) != tref[d].view(torch.int32)).sum())
        assert bad_h == 0 and bad_t == 0, f"relation {q}, segments [{lo}, {hi}): {bad_h} elements of H, {bad_t} of T differ from torch"
        del xs, href, tref, d
        lo = hi
    assert lo == mp.n_seg


# ---- check 2: C -----------------------------------------------------------------------------------------------------------------
def check_c(mp, xp, din, h, t, seed, seg_dh=True, row_w=True):
    """rgcn_segment_max_bwd through the raw entry point on a random dH [pseudo slots, ld], C pre-filled with NaN, against the same
    two fp32 operations by torch ops in row blocks: equality of values, NaN fails, every row; the pad columns +0.0.
    seg_dh / row_w False: NULL (dH indexed by the segment itself, weights 1)"""
    from scaling_rgcn_training_amd import _lib
    lib, dev = _lib.load(), xp.device
    hh, ld = mp.ep.heavy, h.stride(0)
    g = torch.Generator(device=dev).manual_seed(seed)
    dh = torch.randn(hh.n_units * 64, ld, generator=g, device=dev)
    dh[:, din:] = 0.0                            # (an input: zeros in its pad columns)
    c = nan_like(mp.n_hrows, ld, dev)
    assert dh.shape[0] >= mp.n_seg and int(mp.seg_dh.max()) < dh.shape[0] and int(mp.row_seg.max()) == mp.n_seg - 1
    assert int(mp.row_src.max()) < xp.shape[0] and mp.row_src.numel() == mp.row_seg.numel() == mp.row_w.numel() == mp.n_hrows
    with torch.cuda.device(dev):
        st = lib.rgcn_segment_max_bwd(xp.data_ptr(), xp.stride(0), h.data_ptr(), t.data_ptr(), ld, dh.data_ptr(), ld,
                                      mp.row_src.data_ptr(), mp.row_seg.data_ptr(), mp.seg_dh.data_ptr() if seg_dh else None,
                                      mp.row_w.data_ptr() if row_w else None, mp.n_hrows, din, c.data_ptr(), ld,
                                      torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    assert st == 0, st
    bad, hits = 0, 0
    for lo in range(0, mp.n_hrows, BLK):
        s = mp.row_seg[lo:lo + BLK].long()
        hs = h[s, :din]
        d = dh[mp.seg_dh[s].long() if seg_dh else s, :din]
        if row_w:
            d = mp.row_w[lo:lo + BLK, None] * d
        hit = xp[mp.row_src[lo:lo + BLK].long(), :din] == hs
        want = torch.where(hit, d / (t[s, :din] + (hs == 0)), torch.zeros_like(d))
        bad += int((~(c[lo:lo + BLK, :din] == want)).sum())
        hits += int(hit.sum())
        del s, hs, d, hit, want
    assert hits >= mp.n_seg * din, "every segment column has a row that attains its max"
    assert bad == 0, f"rgcn_segment_max_bwd: {bad} of {mp.n_hrows * din} elements of C differ from (w dH) / N by torch"
    if ld > din:
        assert bool((c[:, din:(din + 3) // 4 * 4].view(torch.int32) == 0).all()), "pad columns of C are +0.0"
    return c


# ---- check 3: the module ----------------------------------------------------------------------------------------------------------
def _layer_plan(G, builder):
    """the plan RGCNConv(aggr="max") caches for this graph (conv._forward_max's own key)"""
    from scaling_rgcn_training_amd.plan import cached_graph_plans
    return cached_graph_plans(G["ei"], G["et"], G["n"], G["r"], 0, "max", paths=("ep", "ep"), extra_key=("max",), builder=builder)


def _module(G, x, dg, params, din, dout, split, mp):
    """RGCNConv(din, dout, r, aggr="max") forward and backward on the cached plan ``mp`` -> the conv (gradients set), out, d_x"""
    from scaling_rgcn_training_amd import eplan as E
    from scaling_rgcn_training_amd.conv import RGCNConv
    w, root, bias = params
    conv = RGCNConv(din, dout, G["r"], aggr="max").to(x.device)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.root.copy_(root)
        conv.bias.copy_(bias)
    assert conv.kernel_flags == 0 and conv.split_producers, "the module's defaults"
    conv.split_producers = split
    xg = x.detach().requires_grad_(True)          # (the same storage: x stays the reference's input)
    builds = []
    real, E.build_max_plan = E.build_max_plan, lambda *a, **k: builds.append(a) or real(*a, **k)
    try:
        out = conv(xg, G["ei"], G["et"])
    finally:
        E.build_max_plan = real
    out.backward(dg)
    torch.cuda.synchronize()
    assert not builds and _layer_plan(G, None) is mp, "the layer ran on the plan the other checks walked"
    return conv, out.detach(), xg.grad


def check_module(G, x, dg, params, conv, out, dx, tag):
    w, root, bias = params
    refs = [M.blocked_layer(G, x, dg, w, root, bias, dt, a) for dt, a in ((torch.float64, False), (torch.float64, True),
                                                                         (torch.float32, False))]
    got = (out, dx, conv.weight.grad, conv.root.grad, conv.bias.grad)
    for i, name in enumerate(("out", "d_x", "d_weight", "d_root", "d_bias")):
        check(f"max module {name} {tag}", got[i], Ref.of(refs, i))
    assert bool((conv.weight.grad[G["r"] - 1] == 0).all()), "the dead relation"


def _regime(mp, din, dout, ld_h, splits, h_addr, x_addr, g_addr):
    """what each launch of the layer must pick, from the sizes of its operands: the pseudo rows over H (forward; d_weight), the
    root rows over x, dH and the root rows over g"""
    from scaling_rgcn_training_amd import _lib
    n, s = mp.n_nodes, mp.n_seg
    assert _lib.buffer_addressable(s, ld_h) == h_addr, ("H", s, ld_h)
    assert _lib.buffer_addressable(n, ld_h) == x_addr, ("x", n, ld_h)
    assert _lib.buffer_addressable(n, (dout + 3) // 4 * 4) == g_addr, ("g", n, dout)
    tp = mp.ep.heavy_tile_plan()
    assert tp.n_nodes == s and tp.layout == 2
    w64 = din == dout == 64
    for split in splits:
        flags = SPLIT if split and w64 else 0
        for name, addr, a, b in (("H", h_addr, din, dout), ("x", x_addr, din, dout), ("g", g_addr, dout, din)):
            want = ("ep3",) if w64 and flags and addr else ("ep", K.padded_width(a), K.padded_width(b))
            assert K.ep_transform(a, b, 16, 64, 0, 2, flags, addr, 1) == want, (name, split, want)
        dw = K.bwd_dw(din, dout, tp.tile, tp.chunk, tp.chunk_rows, tp.layout, flags, h_addr and g_addr, tp.n_tiles, tp.n_units)
        if w64 and h_addr and g_addr:
            assert dw[0] == "dw_direct", dw
        else:
            assert dw[0] in ("dw", "dw_wide") and dw[4] is (h_addr and g_addr), dw      # the ring kernel; pointers unless both fit


def _case(G, din, dout, feat, splits, h_addr, x_addr, g_addr, seeds, tag, levels3):
    """the three checks of one case on the layer's own (cached) plan; returns the plan"""
    from scaling_rgcn_training_amd import _lib, eplan as E
    dev = G["ei"].device
    n, r = G["n"], G["r"]
    if feat == "ties":
        g = torch.Generator(device=dev).manual_seed(seeds[0])
        x = torch.randint(-2, 3, (n, din), generator=g, device=dev).float()
    else:
        x = make_features(n, din, dev, seeds[0])
    assert x.stride(0) == din and din % 4 == 0                # the layer's H has the stride of x
    mp = _layer_plan(G, lambda paths: E.build_max_plan(G["ei"], G["et"], n, r))
    _regime(mp, din, dout, din, splits, h_addr, x_addr, g_addr)
    if levels3:
        assert len(mp.ep.heavy.levels) >= 3 and len(mp.bwd_levels) >= 3, (len(mp.ep.heavy.levels), len(mp.bwd_levels))
    h, t = _lib.max_aggregate(mp, x, din, with_t=True)
    assert h.stride(0) == din and h.shape[0] == mp.n_seg
    check_h_t(mp, G, x, din, h, t)
    if feat == "ties":
        zero, tied = int((h == 0).sum()), int((t > 1).sum())
        assert zero > h.numel() // 10 and tied > h.numel() // 100, ("maxima of 0 and ties are common", zero, tied, h.numel())
    check_c(mp, x, din, h, t, seeds[3])
    del h, t
    dg = make_features(n, dout, dev, seeds[1])
    params = make_params(r, din, dout, dev, seeds[2])
    for split in splits:
        _release_but_plans()
        conv, out, dx = _module(G, x, dg, params, din, dout, split, mp)
        check_module(G, x, dg, params, conv, out, dx, f"{tag} split_producers={split}")
        del conv, out, dx
    return mp


def _release_but_plans():
    import gc
    gc.collect()
    torch.cuda.empty_cache()


# ---- the cases -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [(1 << 24) - 3, (1 << 24) - 2], ids=["A1-S=2^24-3", "A2-S=2^24-2"])
def test_h_at_the_last_addressable_row(s):
    """64 -> 64, N = 2^22: H is the last matrix a descriptor reaches (offsets up to 4 GiB - 512) and, one segment more, the first
    it does not -- rgcn_ep_transform3 and rgcn_bwd_dw's direct kernel on one side, the exact transform and the ring d_weight kernel
    with 64-bit pointers on the other; the module with split_producers (its default) and without"""
    dev = _dev()
    n, r = 1 << 22, 9
    addressable = s == (1 << 24) - 3
    if addressable:
        assert (s + 1) * 64 * 4 == (1 << 32) - 512
    G = M.exact_segment_graph(n, r, s, EXTRA, dev, seed=s)
    mp = _case(G, 64, 64, "normal", (True, False), addressable, True, True, (51, 52, 53, 54), f"[S={s} N=2^22 64x64]", True)
    assert mp.n_seg == s


def test_h_rows_past_2_24_at_16_columns():
    """16 -> 16, N = 2^22, S = 2^24 + 4099: H is 1 GiB, by bytes a descriptor would do -- the row rule alone sends the pseudo rows
    to the pointer path.  Integer features in -2 .. 2: ties and maxima of 0 everywhere (N = T + 1)"""
    dev = _dev()
    n, r, s = 1 << 22, 9, (1 << 24) + 4099
    assert (s + 1) * 16 * 4 < 0xFFFFFF00
    G = M.exact_segment_graph(n, r, s, EXTRA_TIES, dev, seed=s)
    mp = _case(G, 16, 16, "ties", (True,), False, True, True, (61, 62, 63, 64), f"[S={s} N=2^22 16x16 ties]", True)
    assert mp.n_seg == s


def test_h_past_2_31_elements():
    """64 -> 64, N = 2^23, S = 2^25 + 4099: H, T, dH and C hold more than 2^31 elements each"""
    dev = _dev()
    n, r, s = 1 << 23, 9, (1 << 25) + 4099
    assert s * 64 > 1 << 31
    G = M.exact_segment_graph(n, r, s, EXTRA, dev, seed=s)
    mp = _case(G, 64, 64, "normal", (True,), False, True, True, (71, 72, 73, 74), f"[S={s} N=2^23 64x64]", True)
    assert mp.n_seg == s and mp.n_hrows * 64 > 1 << 31 and mp.ep.heavy.n_units * 64 * 64 > 1 << 31


def test_the_most_nodes_a_max_plan_admits():
    """64 -> 64, N = 2^24 (EP_MAX_OWNED): x is exactly 4 GiB and not addressable while H is; the backward pseudo slots pad with
    N = 2^24; one more node is refused before anything is built"""
    from scaling_rgcn_training_amd import eplan as E
    from scaling_rgcn_training_amd.plan import _CACHE
    dev = _dev()
    n, r = 1 << 24, 8
    assert n == E.EP_MAX_OWNED and n * 64 * 4 == 1 << 32
    G = make_graph(n, r, dev, seed=n, skew=True)
    s = int(torch.unique(G["ei"][1] * r + G["et"]).numel())
    assert s < 1 << 24
    mp = _case(G, 64, 64, "normal", (True,), True, False, False, (81, 82, 83, 84), f"[N=2^24 S={s} 64x64]", False)
    assert mp.n_seg == s and mp.n_nodes == n
    assert int(mp.bwd_slot_src.max()) == n and bool((mp.bwd_slot_src == n).any()), "the pseudo slots' padding gathers row N = 2^24"
    del mp
    n_cached = len(_CACHE)
    with pytest.raises(ValueError, match="EP_MAX_OWNED"):
        E.build_max_plan(G["ei"], G["et"], n + 1, r)
    assert len(_CACHE) == n_cached


@pytest.mark.parametrize("n", [8_388_606, 8_388_607], ids=["E1-8388606", "E2-8388607"])
def test_g_at_4gib_by_its_width(n):
    """16 -> 128: x (16 columns) is addressable; g (128 columns) is at 8,388,606 rows and is not one row later -- the dH
    transform and the root rows of the backward gather g"""
    from scaling_rgcn_training_amd import _lib
    dev = _dev()
    r = 8
    g_addr = n == 8_388_606
    assert _lib.buffer_addressable(n, 16) and _lib.buffer_addressable(n, 128) == g_addr
    G = make_graph(n, r, dev, seed=n)
    s = int(torch.unique(G["ei"][1] * r + G["et"]).numel())
    mp = _case(G, 16, 128, "normal", (True,), True, True, g_addr, (91, 92, 93, 94), f"[N={n} S={s} 16x128]", False)
    assert mp.n_seg == s
