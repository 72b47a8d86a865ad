"""The option matrix of RGCNConv's base family (float features, mean / sum, at most 128 columns per side) through the module:
the case table of tests/test_gpu_layer_options.py, the route every case claims, and the float64 reference all of them are
compared with.  No GPU is needed to import this module; tests/test_layer_options.py holds the table to a pairwise cover and
to the routes it claims (``RGCNConv._route`` needs no device).

Routes of the family on one GPU (ROUTES): how a layer is steered there and what ``_route`` / the plans must then say.

  ring-exact    path "ring", a side outside the 64-column class: rgcn_tile_kernel (exact fp32), relation-major d_weight
  ring-split    64 x 64 class, path "ring", small graph: rgcn_tile3p_kernel (bf16 x 3) on layout-0 plans, relation-major d_weight
  tiles-split   64 x 64 class, at most 32 relations, conv.DW_TILES_MIN_EDGES lowered: rgcn_tile3p_kernel on layout-3 plans,
                rgcn_dw_tile_kernel<true, true> on the pair plan, streaming d_root / d_bias
  tiles-exact   the same with split_producers = False: the exact-fp32 kernel on layout 3, rgcn_dw_tile_kernel<false, true>
  tiles-side    tiles-split with conv._SIDE_STREAM_MIN_ROWS lowered below n: the root kernel on the side stream beside dX
  ep            path "ep" on a hub graph with 45 .. 89 relations: rgcn_ep_transform* (bf16 x 3 at 64 x 64 on 128-slot routes),
                segment sums in levels, heavy segments, d_weight over the dense units + the heavy pseudo rows
  ep-ring       one direction on each: path ("ep", "ring") or ("ring", "ep")
  dw-direct / dw-ring / pointer     kernel_flags FLAG_DW_DIRECT / FLAG_DW_RING / FLAG_POINTER_GATHER at 64 x 64

Options: mode (full / basis / block), aggr (mean / sum), (root_weight, bias), and the trainable set ``frozen``:
  none: everything trains; weight / comp: that parameter frozen; root+bias: both (whichever exist) frozen; params: every
  parameter frozen (dX alone); x: x without a gradient (the reference's e_freeze configuration), every parameter trains.

The table is a PAIRWISE cover: every (route, mode), (route, aggr), (route, root/bias), (route, frozen), (mode, aggr),
(mode, root/bias) and (mode, frozen) pair that ``pair_admitted`` lets through occurs in a case.  Not admitted:
  * frozen = comp outside basis mode (there is no comp);
  * tiles-side without a root and a bias, with root and bias frozen, with every parameter frozen or without a gradient for x:
    the side stream runs the d_root / d_bias kernel beside dX, so without one of the two it is the tiles-split route;
and, case by case rather than pair by pair: block mode at widths without a common divisor, frozen = root+bias on a layer with
neither, the tiles-* routes above 32 relations (kDwTileMaxRel), tiles-exact at densities where the exact-fp32 kernel's layout
falls to 64-slot chunks (layout 0: another route).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from oracle import rgcn_oracle as O
from oracle.tolerance import abs_condition, assert_close, cpu32_reference

FLAG_POINTER_GATHER, FLAG_DW_RING, FLAG_DW_DIRECT = 1, 2, 4        # include/rgcn_mi355x.h (checked in test_layer_options.py)

MODES = ("full", "basis", "block")
AGGRS = ("mean", "sum")
ROOT_BIAS = ((True, True), (False, False), (True, False), (False, True))
FROZEN = ("none", "weight", "comp", "root+bias", "params", "x")

# what steers a layer onto a route (path, kernel flags, split_producers, the two thresholds lowered) and what _route and the
# plans must say there: plan layout, d_weight on its own tile-major plan, edge-parallel (forward, dX)
_R = namedtuple("_R", "path flags split_producers min_edges side_rows layout dw ep")
ROUTES = {
    "ring-exact": _R("ring", 0, True, None, None, 0, False, (False, False)),
    "ring-split": _R("ring", 0, True, None, None, 0, False, (False, False)),
    "tiles-split": _R("ring", 0, True, 1, None, 3, True, (False, False)),
    "tiles-exact": _R("ring", 0, False, 1, None, 3, True, (False, False)),
    "tiles-side": _R("ring", 0, True, 1, 1, 3, True, (False, False)),
    "ep": _R("ep", 0, True, None, None, 0, False, (True, True)),
    "ep-ring": _R(("ep", "ring"), 0, True, None, None, 0, False, (True, False)),
    "dw-direct": _R("ring", FLAG_DW_DIRECT, True, None, None, 0, False, (False, False)),
    "dw-ring": _R("ring", FLAG_DW_RING, True, None, None, 0, False, (False, False)),
    "pointer": _R("ring", FLAG_POINTER_GATHER, True, None, None, 0, False, (False, False)),
}

# k: num_bases / num_blocks (None in full mode).  chunk, split: the slots per chunk and FLAG_SPLIT_PRODUCERS that _route gives the
# case (split on the ep routes: rgcn_ep_transform3_kernel instead of the exact transform).  swap: ep-ring as ("ring", "ep")
Case = namedtuple("Case", "route din dout n e r mode k aggr root bias frozen chunk split swap", defaults=(False,))

S, M = (3000, 40000), (6000, 80000)        # nodes, edges
D = (3000, 80000)                          # dense enough for 128-slot chunks at 45 relations
CASES = [
    # ---- ring-exact: every padded width class on either side, odd widths on both sides
    Case("ring-exact", 63, 16, *S, 9, "full", None, "mean", True, True, "none", 128, False),
    Case("ring-exact", 7, 33, *S, 9, "basis", 1, "sum", False, False, "weight", 128, False),           # B = 1
    Case("ring-exact", 32, 32, *S, 9, "basis", 12, "mean", True, False, "comp", 128, False),           # B > R
    Case("ring-exact", 50, 128, *S, 9, "block", 2, "sum", False, True, "root+bias", 64, False),        # blocks of 25 x 64
    Case("ring-exact", 128, 24, *S, 9, "block", 4, "mean", True, True, "params", 64, False),           # blocks of 32 x 6
    Case("ring-exact", 16, 16, *S, 9, "block", 16, "sum", True, False, "x", 128, False),               # blocks of 1 x 1
    Case("ring-exact", 12, 24, *S, 9, "block", 4, "mean", False, True, "none", 128, False),            # blocks of 3 x 6
    Case("ring-exact", 128, 128, *M, 9, "full", None, "sum", False, False, "none", 64, False),
    Case("ring-exact", 33, 7, *S, 9, "basis", 3, "mean", True, True, "root+bias", 128, False),
    # ---- ring-split
    Case("ring-split", 64, 64, *S, 9, "full", None, "sum", True, True, "weight", 128, True),
    Case("ring-split", 63, 50, *S, 6, "basis", 3, "mean", False, True, "none", 128, True),
    Case("ring-split", 64, 64, *M, 9, "basis", 2, "sum", False, False, "comp", 128, True),
    Case("ring-split", 64, 64, *S, 9, "block", 1, "mean", True, False, "root+bias", 128, True),        # num_blocks = 1
    Case("ring-split", 50, 60, *S, 6, "block", 10, "sum", True, True, "x", 128, True),                 # blocks of 5 x 6
    Case("ring-split", 63, 63, *S, 9, "full", None, "mean", False, True, "params", 128, True),
    # ---- tiles-split
    Case("tiles-split", 64, 64, *S, 6, "full", None, "mean", True, True, "none", 128, True),
    Case("tiles-split", 64, 64, *M, 9, "basis", 12, "sum", True, False, "weight", 128, True),          # B > R
    Case("tiles-split", 63, 50, *S, 6, "basis", 3, "mean", False, True, "comp", 128, True),
    Case("tiles-split", 64, 64, *S, 32, "block", 4, "sum", True, True, "root+bias", 128, True),        # kDwTileMaxRel relations
    Case("tiles-split", 60, 50, *S, 6, "block", 10, "mean", False, False, "params", 128, True),        # blocks of 6 x 5
    Case("tiles-split", 64, 64, *S, 9, "full", None, "sum", False, True, "x", 128, True),
    Case("tiles-split", 64, 64, 60000, 1200000, 16, "full", None, "sum", True, True, "none", 112, True),   # seven-row-tile ring slots
    # ---- tiles-exact
    Case("tiles-exact", 64, 64, *S, 9, "block", 8, "sum", False, False, "none", 128, False),
    Case("tiles-exact", 64, 64, *S, 6, "full", None, "mean", True, False, "weight", 128, False),
    Case("tiles-exact", 50, 63, *S, 9, "basis", 1, "sum", True, True, "comp", 128, False),             # B = 1
    Case("tiles-exact", 64, 64, *M, 9, "full", None, "sum", False, True, "root+bias", 128, False),
    Case("tiles-exact", 64, 64, *S, 6, "basis", 3, "mean", True, True, "params", 128, False),
    Case("tiles-exact", 63, 63, *S, 9, "block", 9, "mean", True, False, "x", 128, False),              # blocks of 7 x 7
    # ---- tiles-side
    Case("tiles-side", 64, 64, *S, 6, "full", None, "mean", True, True, "none", 128, True),
    Case("tiles-side", 64, 64, *M, 9, "block", 2, "sum", True, False, "weight", 128, True),
    Case("tiles-side", 63, 50, *S, 6, "basis", 4, "sum", False, True, "comp", 128, True),
    # ---- ep
    Case("ep", 63, 16, *S, 89, "full", None, "mean", True, True, "none", 64, False),
    Case("ep", 32, 32, *S, 45, "basis", 30, "sum", False, False, "weight", 64, False),                 # B = 30
    Case("ep", 64, 64, *D, 45, "basis", 30, "mean", True, False, "comp", 128, True),                   # bf16 x 3 transform
    Case("ep", 100, 128, *S, 45, "block", 4, "sum", False, True, "root+bias", 64, False),              # blocks of 25 x 32
    Case("ep", 64, 64, *S, 60, "block", 4, "mean", True, True, "params", 64, False),                   # exact transform at 64 x 64
    Case("ep", 128, 33, *S, 50, "full", None, "sum", True, True, "x", 64, False),
    Case("ep", 50, 64, *D, 45, "full", None, "sum", True, True, "none", 128, True),                    # bf16 x 3, padded rows, sum
    # ---- ep-ring
    Case("ep-ring", 63, 16, *S, 89, "full", None, "sum", True, False, "none", 64, False),
    Case("ep-ring", 32, 32, *S, 45, "basis", 30, "mean", True, True, "weight", 64, False, True),
    Case("ep-ring", 64, 64, *D, 45, "basis", 5, "sum", False, True, "comp", 128, True),
    Case("ep-ring", 64, 64, *D, 45, "block", 4, "mean", True, True, "root+bias", 128, True, True),
    Case("ep-ring", 128, 24, *S, 45, "block", 4, "sum", False, False, "params", 64, False),
    Case("ep-ring", 16, 128, *S, 45, "full", None, "mean", True, True, "x", 64, False, True),
    # ---- dw-direct
    Case("dw-direct", 64, 64, *S, 9, "full", None, "mean", False, False, "none", 128, True),
    Case("dw-direct", 64, 64, *S, 9, "block", 4, "sum", True, True, "weight", 128, True),
    Case("dw-direct", 63, 50, *S, 9, "basis", 3, "mean", True, False, "comp", 128, True),
    Case("dw-direct", 64, 64, *M, 9, "basis", 12, "sum", False, True, "root+bias", 128, True),
    Case("dw-direct", 64, 64, *S, 9, "full", None, "sum", True, True, "params", 128, True),
    Case("dw-direct", 50, 60, *S, 9, "block", 2, "mean", True, True, "x", 128, True),
    # ---- dw-ring
    Case("dw-ring", 64, 64, *S, 9, "basis", 3, "sum", True, True, "none", 128, True),
    Case("dw-ring", 64, 64, *S, 9, "full", None, "mean", False, True, "weight", 128, True),
    Case("dw-ring", 64, 64, *S, 9, "basis", 1, "sum", False, False, "comp", 128, True),
    Case("dw-ring", 63, 63, *S, 9, "block", 3, "mean", True, False, "root+bias", 128, True),
    Case("dw-ring", 64, 64, *M, 9, "block", 4, "sum", True, True, "params", 128, True),
    Case("dw-ring", 63, 50, *S, 9, "basis", 5, "mean", True, True, "x", 128, True),
    # ---- pointer
    Case("pointer", 64, 64, *S, 9, "block", 4, "mean", True, True, "none", 128, True),
    Case("pointer", 63, 50, *S, 9, "basis", 3, "sum", False, False, "weight", 128, True),
    Case("pointer", 64, 64, *S, 9, "basis", 12, "mean", False, True, "comp", 128, True),
    Case("pointer", 64, 64, *M, 9, "full", None, "sum", True, False, "root+bias", 128, True),
    Case("pointer", 64, 64, *S, 9, "full", None, "mean", True, True, "params", 128, True),
    Case("pointer", 64, 64, *S, 9, "block", 8, "sum", True, True, "x", 128, True),
]


def case_id(c: Case) -> str:
    rb = ("root" if c.root else "") + ("+" if c.root and c.bias else "") + ("bias" if c.bias else "") or "bare"
    k = "" if c.k is None else str(c.k)
    return f"{c.route}{'-swap' if c.swap else ''}-{c.din}x{c.dout}-r{c.r}-{c.mode}{k}-{c.aggr}-{rb}-freeze_{c.frozen}"


def pair_admitted(a: str, av, b: str, bv) -> bool:
    """whether the pair (field a = av, field b = bv) can occur at all (module docstring: what is not admitted and why)"""
    f = {a: av, b: bv}
    if f.get("frozen") == "comp" and f.get("mode", "basis") != "basis":
        return False
    if f.get("route") == "tiles-side":
        if f.get("root_bias") == (False, False) or f.get("frozen") in ("root+bias", "params", "x"):
            return False
    return True


def case_fields(c: Case) -> dict:
    return {"route": c.route, "mode": c.mode, "aggr": c.aggr, "root_bias": (c.root, c.bias), "frozen": c.frozen}


DOMAINS = {"route": tuple(ROUTES), "mode": MODES, "aggr": AGGRS, "root_bias": ROOT_BIAS, "frozen": FROZEN}
PAIR_FIELDS = [("route", "mode"), ("route", "aggr"), ("route", "root_bias"), ("route", "frozen"), ("mode", "aggr"),
               ("mode", "root_bias"), ("mode", "frozen")]


# ---- building a case ---------------------------------------------------------------------------------------------------------
def paths_of(c: Case):
    p = ROUTES[c.route].path
    return tuple(reversed(p)) if c.swap else p


def make_layer(c: Case, monkeypatch):
    """the case's RGCNConv (CPU), steered onto its route; glorot parameters of the layer's own reset, a non-zero bias, the
    frozen set applied.  Lowers the two module thresholds through ``monkeypatch`` where the route asks for it."""
    from scaling_rgcn_training_amd import conv as conv_mod
    rt = ROUTES[c.route]
    kw = {"basis": {"num_bases": c.k}, "block": {"num_blocks": c.k}, "full": {}}[c.mode]
    torch.manual_seed(1000 + CASES.index(c))
    conv = conv_mod.RGCNConv(c.din, c.dout, c.r, aggr=c.aggr, root_weight=c.root, bias=c.bias, **kw)
    if conv.bias is not None:
        with torch.no_grad():
            conv.bias.uniform_(-1, 1)
    conv.path, conv.kernel_flags, conv.split_producers = paths_of(c), rt.flags, rt.split_producers
    conv.merge_runs, conv.dw_tiles = True, True
    if rt.min_edges is not None:
        monkeypatch.setattr(conv_mod, "DW_TILES_MIN_EDGES", rt.min_edges)
    else:
        assert c.e < conv_mod.DW_TILES_MIN_EDGES
    if rt.side_rows is not None:
        monkeypatch.setattr(conv_mod, "_SIDE_STREAM_MIN_ROWS", rt.side_rows)
    else:
        assert c.n < conv_mod._SIDE_STREAM_MIN_ROWS
    frozen = {"none": (), "x": (), "weight": ("weight",), "comp": ("comp",), "root+bias": ("root", "bias"),
              "params": ("weight", "comp", "root", "bias")}[c.frozen]
    for name in frozen:
        p = getattr(conv, name)
        if p is not None:
            p.requires_grad_(False)
    return conv


def assert_route(c: Case, route) -> None:
    """``route`` = conv._route(n, e, True) of the case's layer: the kernels the table entry claims"""
    rt = ROUTES[c.route]
    want = (c.chunk, rt.layout, rt.dw, c.split, paths_of(c) if isinstance(paths_of(c), tuple) else (paths_of(c),) * 2)
    got = (route.chunk, route.layout, route.dw_tiles, route.split_producers, tuple(route.paths))
    assert got == want, f"{case_id(c)}: (chunk, layout, dw_tiles, split_producers, paths) = {got}, the table claims {want}"


def make_graph(c: Case):
    """O.synthetic_graph over the first r - 1 relations (the last one has no edge), hubs on the edge-parallel routes; 60 duplicate
    triples and 40 self loops"""
    ei, et = O.synthetic_graph(c.n, c.e, c.r - 1, seed=c.n + c.r + c.din, skew=ROUTES[c.route].ep != (False, False))
    ei[:, 100:160] = ei[:, 20:80]
    et[100:160] = et[20:80]
    ei[1, 200:240] = ei[0, 200:240]
    return ei, et


# ---- the reference -------------------------------------------------------------------------------------------------------------
class Reference:
    """float64 values, their conditions (the same sums on absolute values) and the fp32 CPU loop's values of one layer on one
    input: ``ref`` / ``cond`` / ``cpu32`` keyed "out", "x", "root", "bias", "weight", "comp" -- "weight" / "comp" are the
    gradients of the layer's OWN parameters (bases, blocks)."""

    def __init__(self, conv, x, ei, et, g):
        r, din, dout, aggr = conv.num_relations, conv.in_channels, conv.out_channels, conv.aggr
        cpu = lambda p: None if p is None else p.detach().cpu()      # noqa: E731
        w32, comp32, root32, bias32 = cpu(conv.weight), cpu(conv.comp), cpu(conv.root), cpu(conv.bias)
        w = w32.double()
        comp = None if comp32 is None else comp32.double()
        root = None if root32 is None else root32.double().numpy()
        bias = None if bias32 is None else bias32.double().numpy()
        wf = O.effective_weight(w, comp, r, conv.num_blocks, din, dout).numpy()
        xn, gn, ein, etn = x.double().numpy(), g.double().numpy(), ei.numpy(), et.numpy()
        out, rg = O.rgcn_conv_segments(xn, ein, etn, wf, root, bias, gn, aggr=aggr)
        c_out, cg = abs_condition(xn, ein, etn, wf, root, bias, gn, aggr=aggr)
        cpu_out, cpu_g = cpu32_reference(xn, ein, etn, wf, root, bias, gn, aggr=aggr)
        self.ref = {"out": out, "x": rg["x"], "weight": rg["weight"]}
        self.cond = {"out": c_out, "x": cg["x"], "weight": cg["weight"]}
        self.cpu32 = {"out": cpu_out, "x": cpu_g["x"], "weight": cpu_g["weight"]}
        for name, there in (("root", root is not None), ("bias", bias is not None)):
            if there:
                self.ref[name], self.cond[name], self.cpu32[name] = rg[name], cg[name], cpu_g[name]
        if comp is None and conv.num_blocks is None:
            return

        # a decomposition: the float64 dense d_W pushed through effective_weight by float64 autograd, the condition the same
        # push on absolute values; the fp32 CPU value by fp32 autograd of the loop form on the layer's own parameters
        def push(wv, cv, dw):
            wv = wv.clone().requires_grad_(True)
            cv = None if cv is None else cv.clone().requires_grad_(True)
            full = O.effective_weight(wv, cv, r, conv.num_blocks, din, dout)
            return torch.autograd.grad(full, [t for t in (wv, cv) if t is not None], torch.from_numpy(np.ascontiguousarray(dw)))

        want = push(w, comp, rg["weight"])
        cond = push(w.abs(), None if comp is None else comp.abs(), np.abs(cg["weight"]))
        t32 = lambda a: None if a is None else a.float().clone().requires_grad_(True)      # noqa: E731
        xv, wv, cv, rv, bv = t32(x), t32(w32), t32(comp32), t32(root32), t32(bias32)
        O.rgcn_conv_loop(xv, ei, et, wv, rv, bv, comp=cv, num_blocks=conv.num_blocks, aggr=aggr).backward(g.float())
        self.ref["weight"], self.cond["weight"], self.cpu32["weight"] = want[0].numpy(), cond[0].numpy(), wv.grad.numpy()
        if comp is not None:
            self.ref["comp"], self.cond["comp"], self.cpu32["comp"] = want[1].numpy(), cond[1].numpy(), cv.grad.numpy()

    def check(self, name: str, got, tag: str) -> None:
        """oracle/tolerance.py, both bounds: (1) with the condition sums, (2) no worse than 2 x the fp32 CPU loop"""
        got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
        assert got.shape == self.ref[name].shape, (tag, name, got.shape, self.ref[name].shape)
        assert_close(got, self.ref[name], self.cond[name], f"{'d_' if name != 'out' else ''}{name} [{tag}]", cpu32=self.cpu32[name])


def check_layer(conv, x, ei, et, g, out, dx, grads, tag: str) -> Reference:
    """``out``, ``dx`` (None: x had no gradient) and ``grads`` (name -> gradient of every parameter that trains) of one
    forward + backward of ``conv`` against the float64 reference; frozen and absent parameters must have no gradient"""
    ref = Reference(conv, x, ei, et, g)
    ref.check("out", out, tag)
    if dx is not None:
        ref.check("x", dx, tag)
    for name in ("weight", "comp", "root", "bias"):
        p = getattr(conv, name)
        if p is None or not p.requires_grad:
            assert name not in grads and (p is None or p.grad is None), f"{tag}: {name} is frozen or absent and has a gradient"
        else:
            assert name in grads, f"{tag}: {name} trains and has no gradient"
            ref.check(name, grads[name], tag)
    return ref
