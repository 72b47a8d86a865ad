"""The real edge-partitioned HIP path with 2 ranks sharing the one GPU of the test box (gloo backend
moving CUDA tensors; RCCL refuses two ranks on one device).  The driver measures true multi-GPU scaling
at round end with bench.py; this checks that the partitioned layer equals the single-rank layer."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, ret, dw_direct):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle import rgcn_oracle as O
    from scaling_rgcn_training_amd import _lib, dist as rdist
    from scaling_rgcn_training_amd.conv import RGCNConv
    dev = torch.device("cuda:0")
    # "0" / "2": pin the relation-major dW kernel (ring / direct) on every piece; "tiles": the default of 64 x 64 layers on
    # large graphs -- every piece on the tile-major kernel with its own T = 320 plan -- reached here by lowering the
    # edge-count threshold; "skew": the same on a hub graph, whose cut follows the edge counts (unequal blocks, broadcasts)
    from scaling_rgcn_training_amd import conv as C
    flags = {"0": _lib.FLAG_DW_RING, "2": _lib.FLAG_DW_DIRECT}.get(dw_direct, 0)
    # "skew-ep": the hub graph with the path choice left to the layer -- every piece's forward on the edge-parallel kernels
    # "needed": the opt-in exchange in which a rank receives only the rows its plans read (all_to_all_single with split sizes);
    # unread rows are poisoned with NaN here and the read ones must be bit-identical to the single-rank layer
    # "options": the tile path with a basis decomposition, sum aggregation and no bias -- the dense d_W is all-reduced BEFORE
    # rgcn_basis_backward turns it into d_bases / d_comp (taken from a rank's partial d_W and never reduced, they would be that
    # rank's share alone); with sum aggregation every slot weight of the layout-3 and pair plans is a small integer
    options = dw_direct == "options"
    if dw_direct in ("tiles", "skew", "skew-ep", "needed", "needed-skew", "options"):
        C.DW_TILES_MIN_EDGES = 1
    skew = "skew" in dw_direct
    needed = dw_direct.startswith("needed")
    n, e, r, din, dout = 3000, 40000, 6, 64, 64
    ei, et = O.synthetic_graph(n, e, r, seed=2, skew=skew)
    w, root, bias = O.synthetic_params(r, din, dout, seed=2)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, din, generator=g)
    dg = torch.randn(n, dout, generator=g)

    def make_options_layer():
        torch.manual_seed(17)       # the layer's own glorot parameters, the same in every run and on every rank
        return RGCNConv(din, dout, r, num_bases=3, aggr="sum", bias=False)

    def run(partitioned):
        conv = (make_options_layer() if options else RGCNConv(din, dout, r)).to(dev)
        conv.kernel_flags = flags
        if dw_direct != "skew-ep":
            conv.path = "ring"      # tile kernels in both runs: a rank's tiles are the single-rank tiles, bit for bit
        if not options:
            with torch.no_grad():
                conv.weight.copy_(w)
                conv.root.copy_(root)
                conv.bias.copy_(bias + 0.25)
        if partitioned:
            rdist.attach(conv, n, e, edge_index=ei, exchange="needed" if needed else "full", edge_type=et)
            assert conv.dist is not None and conv.dist.world == world
            assert conv.dist.uniform == (not skew)
            conv.dist.poison_unread = needed
        xd = x.to(dev).requires_grad_(True)
        out = conv(xd, ei.to(dev), et.to(dev))
        out.backward(dg.to(dev))
        torch.cuda.synchronize()
        if partitioned and dw_direct in ("tiles", "skew", "options"):
            # full exchange: x and g are replicated, so a rank's d_weight is ONE tile-major launch over a contiguous range of its own
            assert conv.dist.stats.get("dw_tiles_rank", 0) == 1 and conv.dist.stats.get("dw_tiles_pieces", 0) == 0
        if partitioned and needed:
            owned = sum(1 for pc in conv._plans(xd, ei.to(dev), et.to(dev)).pieces if pc.fwd.n_owned > 0)
            assert conv.dist.stats.get("dw_tiles_pieces", 0) == owned > 0, "needed rows: every piece's d_weight on the tile-major kernel with its own plan"
        if partitioned and needed:
            pl = conv._plans(xd, ei.to(dev), et.to(dev))
            dctx = conv.dist
            masks = []
            for need in (pl.needed_fwd, pl.needed_bwd):
                read = torch.zeros(n, dtype=torch.bool)
                for s_ in range(dctx.pieces):
                    b_, e_ = dctx.node_range(s_, n)
                    read[b_:e_] = True
                    read[need.recv_idx[s_].cpu()] = True
                masks.append(read.numpy())
            o, gx = out.detach().cpu().numpy(), xd.grad.cpu().numpy()
            assert np.isnan(o[~masks[0]]).all() and np.isnan(gx[~masks[1]]).all(), "unread rows are not written"
            assert 0 < pl.needed_fwd.rows_needed <= pl.needed_fwd.rows_remote
            return (o, gx, conv.weight.grad.cpu().numpy(), conv.root.grad.cpu().numpy(), conv.bias.grad.cpu().numpy(), masks)
        if dw_direct == "skew-ep":
            pl = conv._plans(xd, ei.to(dev), et.to(dev))
            pcs = pl.pieces if partitioned else [pl]
            assert all(pc.ep_fwd is not None for pc in pcs if pc.fwd is None) and any(pc.ep_fwd is not None for pc in pcs)
            if partitioned:      # hubs split across ranks: the heavy segments of the whole graph, an equal share of their rows per rank
                sh = pl.shared_fwd
                assert sh is not None and sh.n_seg > 0 and 0 < sh.row_hi - sh.row_lo <= sh.n_rows // world + 1
                assert all(pc.ep_fwd.heavy is None or pc.ep_fwd.heavy.shared is sh for pc in pcs)
                assert conv.dist.stats.get("shared_heavy_rows", 0) >= sh.row_hi - sh.row_lo
                bc = conv.dist.block_costs.sum(0) + conv.dist.shared_rows_per_rank
                assert float(bc.max() / bc.mean()) <= 1.3, "rows walked per rank max / mean with the hubs split across the ranks"
        if options:
            pl = conv._plans(xd, ei.to(dev), et.to(dev))
            assert all(pc.fwd.layout == 3 for pc in (pl.pieces if partitioned else [pl])), "the tile path: layout-3 plans"
            assert (pl.dw_rank[0] if partitioned else pl.dw) is not None, "d_weight on the tile-major kernel's own plan"
            assert conv.comp.grad is not None and conv.bias is None
            return (out.detach().cpu().numpy(), xd.grad.cpu().numpy(), conv.weight.grad.cpu().numpy(), conv.comp.grad.cpu().numpy(),
                    conv.root.grad.cpu().numpy())
        return (out.detach().cpu().numpy(), xd.grad.cpu().numpy(), conv.weight.grad.cpu().numpy(),
                conv.root.grad.cpu().numpy(), conv.bias.grad.cpu().numpy())

    single = run(False)
    part = run(True)
    if rank == 0:
        if dw_direct == "skew-ep":      # per-destination sums in slot order: a piece's units pack differently from the whole graph's
            np.testing.assert_allclose(part[0], single[0], rtol=2e-5, atol=2e-5 * max(1.0, float(np.abs(single[0]).max())))
            np.testing.assert_allclose(part[1], single[1], rtol=2e-5, atol=2e-5 * max(1.0, float(np.abs(single[1]).max())))
        elif needed:
            mf, mb = part[5]
            assert np.array_equal(single[0][mf], part[0][mf]), "owned + read rows of the forward output bit-identical"
            assert np.array_equal(single[1][mb], part[1][mb]), "owned + read rows of dX bit-identical"
        else:
            assert np.array_equal(single[0], part[0]), "partitioned forward must be bit-identical (tile-aligned ranges)"
            assert np.array_equal(single[1], part[1]), "partitioned dX must be bit-identical"
        if options:
            # the gradients of the layer's own parameters (bases, comp, root) of both runs against float64, both bounds of
            # oracle/tolerance.py (tests/layer_options.py); the output and d_x of the single-rank run too
            from tests import layer_options as L
            ref = L.Reference(make_options_layer(), x, ei, et, dg)
            ref.check("out", single[0], "options single")
            ref.check("x", single[1], "options single")
            for tag, res in (("options single", single), ("options 2 ranks", part)):
                ref.check("weight", res[2], tag)
                ref.check("comp", res[3], tag)
                ref.check("root", res[4], tag)
            ret.put("ok")
            dist.destroy_process_group()
            return
        # weight grads: per-rank partial sums all-reduced -> summation order differs; both must meet the
        # parity criterion against the float64 oracle
        from oracle.tolerance import abs_condition, assert_close
        _, gr = O.rgcn_conv_segments(x.numpy(), ei.numpy(), et.numpy(), w.numpy(), root.numpy(),
                                     (bias + 0.25).numpy(), dg.numpy())
        _, c = abs_condition(x, ei, et, w, root, bias + 0.25, dg)
        for res in (single, part):
            assert_close(res[2], gr["weight"], c["weight"], "d_weight")
            assert_close(res[3], gr["root"], c["root"], "d_root")
            assert_close(res[4], gr["bias"], c["bias"], "d_bias")
        ret.put("ok")
    dist.destroy_process_group()


@pytest.mark.parametrize("dw_direct", ["0", "2", "tiles", "skew", "skew-ep", "needed", "needed-skew", "options"])
def test_two_ranks_one_gpu_partitioned_layer_equals_single_rank(dw_direct):
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, ret, dw_direct)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert ret.get(timeout=5) == "ok"


@pytest.mark.parametrize("exchange", ["full", "needed"])
def test_emulated_world_8_ranks_stitch_to_the_single_rank_layer(exchange):
    """``dist.attach(..., emulate=(world, rank))`` (bench.py --emulate-world): ONE process builds rank r's plans of the world-8
    cut and launches rank r's kernels with the collectives skipped.  The eight ranks' owned rows, stitched, are the
    single-GPU layer bit for bit (forward and dX); the eight partial weight gradients add up to the single-GPU ones."""
    from oracle import rgcn_oracle as O
    from scaling_rgcn_training_amd import conv as C, dist as rdist
    from scaling_rgcn_training_amd.conv import RGCNConv
    from scaling_rgcn_training_amd.plan import clear_plan_cache
    dev = torch.device("cuda:0")
    old = C.DW_TILES_MIN_EDGES
    C.DW_TILES_MIN_EDGES = 1
    try:
        n, e, r, d, world = 20000, 300000, 6, 64, 8
        ei, et = O.synthetic_graph(n, e, r, seed=9)
        w, root, bias = O.synthetic_params(r, d, d, seed=9)
        g = torch.Generator().manual_seed(1)
        x = torch.randn(n, d, generator=g).to(dev)
        dg = torch.randn(n, d, generator=g).to(dev)
        eid, etd = ei.to(dev), et.to(dev)

        def run(emulate):
            conv = RGCNConv(d, d, r).to(dev)
            conv.path = "ring"
            with torch.no_grad():
                conv.weight.copy_(w)
                conv.root.copy_(root)
                conv.bias.copy_(bias + 0.5)
            if emulate is not None:
                rdist.attach(conv, n, e, edge_index=eid, pieces=2, exchange=exchange, emulate=emulate)
                assert conv.dist.emulate and conv.dist.world == world and conv.dist.rank == emulate[1]
            xd = x.clone().requires_grad_(True)
            out = conv(xd, eid, etd)
            out.backward(dg)
            torch.cuda.synchronize()
            return conv, out.detach(), xd.grad, conv.weight.grad, conv.root.grad, conv.bias.grad

        _, o1, gx1, gw1, gr1, gb1 = run(None)
        o8, gx8 = torch.full_like(o1, float("nan")), torch.full_like(gx1, float("nan"))
        gw8, gr8, gb8 = torch.zeros_like(gw1), torch.zeros_like(gr1), torch.zeros_like(gb1)
        for rk in range(world):
            conv, o, gx, gw, gr, gb = run((world, rk))
            for s in range(conv.dist.pieces):
                b, e_ = conv.dist.node_range(s, n)
                o8[b:e_], gx8[b:e_] = o[b:e_], gx[b:e_]
            gw8 += gw
            gr8 += gr
            gb8 += gb
        assert torch.equal(o8, o1) and torch.equal(gx8, gx1), "the ranks' owned rows are the single-GPU rows"
        for a, b_, what in ((gw8, gw1, "d_weight"), (gr8, gr1, "d_root"), (gb8, gb1, "d_bias")):
            tol = 2e-5 * max(1.0, float(b_.abs().max()))
            assert float((a - b_).abs().max()) <= tol, what
    finally:
        C.DW_TILES_MIN_EDGES = old
        clear_plan_cache()


# ---- a partitioned TWO-layer stack against the float64 oracle ---------------------------------------------------------------
# Only a layer that reads another partitioned layer's output can see a row the exchange failed to deliver (layer 1 reads the
# replicated x).  conv1 (64 -> 64, bf16 x 3 on 128-slot chunks) -> ReLU -> conv2 (64 -> 16, exact fp32) on a graph with hubs on
# BOTH sides and 45 relations (AIFB-like: path="auto" takes the edge-parallel path in both directions, so the heavy segments of
# both directions are split across the ranks), every exchange / path / split_hubs case with unread rows poisoned with NaN.
STACK_N, STACK_R = 4000, 45
STACK_CASES = [(ex, path, split) for ex in ("full", "needed") for path in ("ring", "ep", "auto") for split in (True, False)]


def _stack_graph():
    from oracle import rgcn_oracle as O
    a, ta = O.synthetic_graph(STACK_N, 30000, STACK_R, seed=3, skew=True)      # hubs at destinations
    b, tb = O.synthetic_graph(STACK_N, 30000, STACK_R, seed=4, skew=True)      # ... and, flipped, at sources
    return torch.cat([a, b.flip(0)], 1), torch.cat([ta, tb])


def _stack_params():
    from oracle import rgcn_oracle as O
    w1, r1, _ = O.synthetic_params(STACK_R, 64, 64, seed=11)
    w2, r2, _ = O.synthetic_params(STACK_R, 64, 16, seed=12)
    g = torch.Generator().manual_seed(13)
    return [(w1, r1, 0.1 * torch.randn(64, generator=g)), (w2, r2, 0.1 * torch.randn(16, generator=g))]


def _oracle_stack(x, ei, et, params, dg, dtype):
    """relu(conv1(x)) -> conv2 through tests.twins.OracleConv under autograd on the CPU: (out, d_x, [(d_W, d_root, d_bias)] * 2)"""
    from tests.twins import OracleConv

    class _P:       # the parameters OracleConv copies
        def __init__(self, w, r, b):
            self.weight, self.root, self.bias = (torch.nn.Parameter(t.clone()) for t in (w, r, b))

    convs = [OracleConv(_P(*p)).to(dtype) for p in params]
    xd = x.detach().to(dtype).clone().requires_grad_(True)
    out = convs[1](torch.relu(convs[0](xd, ei, et)), ei, et)
    out.backward(dg.to(dtype))
    return out.detach(), xd.grad, [(c.weight.grad, c.root.grad, c.bias.grad) for c in convs]


def _stack_worker(rank, world, port, ret):
    import datetime
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    # a rank that raises must not leave its peers waiting in a collective for gloo's default half hour
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    from scaling_rgcn_training_amd import dist as rdist
    from scaling_rgcn_training_amd.conv import RGCNConv
    from scaling_rgcn_training_amd.eplan import decide_paths
    dev = torch.device("cuda:0")
    n, r = STACK_N, STACK_R
    ei, et = _stack_graph()
    e = int(et.shape[0])
    eid, etd = ei.to(dev), et.to(dev)
    params = _stack_params()
    g = torch.Generator().manual_seed(14)
    x = torch.randn(n, 64, generator=g)
    dg = torch.randn(n, 16, generator=g)
    # the oracle and the fp32 CPU loop (its own error sets the bound, as in test_gpu_shapes._two_layer_case), once per graph
    ref = _oracle_stack(x, ei, et, params, dg, torch.float64)
    r32 = _oracle_stack(x, ei, et, params, dg, torch.float32)
    names = ["out", "d_x"] + [f"conv{i + 1}.{k}" for i in range(2) for k in ("d_weight", "d_root", "d_bias")]
    flat = lambda res: [res[0], res[1]] + [t for grads in res[2] for t in grads]      # noqa: E731
    ref_l, cpu_err = flat(ref), [float((a.double() - b).abs().max()) for a, b in zip(flat(r32), flat(ref))]
    errs = []

    def run(exchange, path, split):
        convs = [RGCNConv(64, 64, r).to(dev), RGCNConv(64, 16, r).to(dev)]
        for c, (w, rt, b) in zip(convs, params):
            c.path = path
            with torch.no_grad():
                c.weight.copy_(w)
                c.root.copy_(rt)
                c.bias.copy_(b)
        if exchange is not None:
            rdist.attach(torch.nn.ModuleList(convs), n, e, edge_index=ei, exchange=exchange, edge_type=et, split_hubs=split)
            for c in convs:
                assert c.dist is not None and c.dist.world == world and c.dist.exchange == exchange and c.dist.split_hubs == split
                c.dist.poison_unread = True
            # a needed exchange feeds the next layer the rows ITS plans read: both layers must cut the graph alike
            assert convs[0].dist.bounds == convs[1].dist.bounds
        xd = x.to(dev).requires_grad_(True)
        h = convs[0](xd, eid, etd, _activation="relu", _grad_premasked=True)
        out = convs[1](h, eid, etd, _input_relu=True)
        out.backward(dg.to(dev))
        torch.cuda.synchronize()
        res = [out.detach().cpu(), xd.grad.cpu()] + [p.grad.cpu() for c in convs for p in (c.weight, c.root, c.bias)]
        return convs, (xd, h), res

    single_ring = run(None, "ring", True)[2]
    for exchange, path, split in STACK_CASES:
        case = f"world {world} rank {rank} {exchange} {path} split_hubs={split}"
        convs, (xd, h), res = run(exchange, path, split)
        dctx = convs[0].dist
        owned = torch.zeros(n, dtype=torch.bool)
        for s_ in range(dctx.pieces):
            b_, e_ = dctx.node_range(s_, n)
            owned[b_:e_] = True
        # which kernels actually ran, per layer
        for c, inp in zip(convs, (xd, h)):
            pl = c._plans(inp, eid, etd)
            live = [pc for s_, pc in enumerate(pl.pieces) if c.dist.node_range(s_, n)[1] > c.dist.node_range(s_, n)[0]]
            ep = path != "ring"
            if path == "auto":
                tile, chunk = c.layout(n, e)
                assert decide_paths(eid, n, r, c.in_channels, c.out_channels, tile, chunk) == ("ep", "ep"), "auto takes ep here"
            assert live and all((pc.ep_fwd is not None) == ep and (pc.fwd is None) == ep for pc in live), case
            assert all((pc.ep_bwd is not None) == ep and (pc.bwd is None) == ep for pc in live), case
            assert (pl.shared_fwd is not None) == (ep and split) and (pl.shared_bwd is not None) == (ep and split), case
            assert (pl.needed_fwd is not None) == (exchange == "needed"), case
        # owned rows of the output and of d_x, every weight gradient: finite, and within the oracle bound
        got = [res[0][owned], res[1][owned]] + res[2:]
        want = [ref_l[0][owned], ref_l[1][owned]] + ref_l[2:]
        for nm, a, b, ce in zip(names, got, want, cpu_err):
            if not bool(torch.isfinite(a).all()):
                errs.append(f"{case}: {nm} has {int((~torch.isfinite(a)).sum())} non-finite entries")
                continue
            excess = float(((a.double() - b).abs() - (1e-5 + 1e-5 * b.abs())).max())
            if excess > 2 * ce:
                errs.append(f"{case}: {nm} excess over flat 1e-5 {excess:.3e} > 2 x fp32 CPU loop error {ce:.3e}")
        # weight gradients are all-reduced: every rank holds the same bits
        mine = torch.cat([t.reshape(-1) for t in res[2:]])
        every = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        if not all(torch.equal(t, every[0]) for t in every):
            errs.append(f"{case}: weight gradients differ across ranks")
        if exchange == "full" and path == "ring":
            # tile-aligned blocks: a rank's tiles are the single-rank tiles, bit for bit
            for nm, a, b in zip(names[:2], res[:2], single_ring[:2]):
                if not torch.equal(a[owned], b[owned]):
                    errs.append(f"{case}: owned rows of {nm} differ from the single-rank stack")
    ret.put((rank, errs))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_partitioned_two_layer_stack_matches_the_float64_oracle(world):
    """Every case of STACK_CASES inside ONE spawn of ``world`` ranks (processes and plan cache set up once): owned rows of the
    output and of d_x and both layers' weight gradients against a float64 OracleConv stack, no NaN (unread rows are poisoned),
    weight gradients bit-equal across ranks, ring + full exchange bit-identical to the single-rank stack."""
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_stack_worker, args=(r, world, port, ret)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    for p in procs:
        if p.is_alive():
            p.kill()
            p.join(10)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    errs = [m for _ in range(world) for m in ret.get(timeout=5)[1]]
    assert not errs, "\n".join(errs)
