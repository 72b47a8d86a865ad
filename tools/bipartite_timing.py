#!/usr/bin/env python3
"""Bipartite RGCNConv (``x = (x_src, x_dst)``): HIP-event medians of forward + backward on one MI355X, beside the
homogeneous layer's step on the FULL graph in the same process (what a caller who needs only some rows has to run without it):
  * target rows (``target_block``) on 1M nodes / 10M edges / 32 relations at 64 -> 64, rows = 1 % and 10 % of the nodes;
  * the AM-like shape (1.5M / 6M / 267, 30 bases, 32 -> 32) with 1,000 rows;
  * a hop block ``(x, x[:N_dst])`` with N_dst = N_src / 4 on the 1M graph;
and rgcn_rows_transform / rgcn_rows_dw alone at 1M rows (64 x 64 and 128 x 128) with their fraction of 6.3 TB/s by the byte models
rows x (din + 2 dout) x 4 (transform: x and add read, y written) and rows x (din + dout) x 4 (d_w).
    python tools/bipartite_timing.py [--cases ...] [--steps 10]
Prints one JSON line per case.  The bipartite step includes the caller's ``x[rows]`` and its backward.  Kernel-only times of a step:
run under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name: (nodes, edges, relations, in, out, bases, rows: a fraction of the nodes, a count, or "hop")
CASES = {"1m_1pct": (1_000_000, 10_000_000, 32, 64, 64, None, 0.01), "1m_10pct": (1_000_000, 10_000_000, 32, 64, 64, None, 0.10),
         "am_1000": (1_500_000, 6_000_000, 267, 32, 32, 30, 1000), "hop_quarter": (1_000_000, 10_000_000, 32, 64, 64, None, "hop")}
KERNEL_ROWS = 1_000_000
KERNEL_WIDTHS = ((64, 64), (128, 128))
PEAK_BYTES = 6.3e12


def median_ms(fn, steps):
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def layer_case(case, steps, dev):
    from oracle import rgcn_oracle as O
    from scaling_rgcn_training_amd.conv import RGCNConv, target_block
    from scaling_rgcn_training_amd.plan import clear_plan_cache
    n, e, r, din, dout, nb, what = CASES[case]
    ei, et = O.synthetic_graph(n, e, r, seed=0)
    ei, et = ei.to(dev), et.to(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(n, din, device=dev, generator=gen).requires_grad_(True)
    if what == "hop":
        rows = torch.arange(n // 4, device=dev)
    else:
        k = what if isinstance(what, int) else int(n * what)
        rows = torch.randperm(n, device=dev, generator=gen)[:k]
    sub, typ = target_block(ei, et, rows, n)
    g_full = torch.randn(n, dout, device=dev, generator=gen)
    g_rows = g_full[rows].contiguous()
    full = RGCNConv(din, dout, r, num_bases=nb).to(dev)
    bip = RGCNConv((din, din), dout, r, num_bases=nb).to(dev)

    def reset(conv):
        x.grad = None
        for p in conv.parameters():
            p.grad = None

    def full_step():
        reset(full)
        full(x, ei, et).backward(g_full)

    def bip_step():
        reset(bip)
        xd = x[:rows.shape[0]] if what == "hop" else x[rows]
        bip((x, xd), sub, typ).backward(g_rows)

    rec = {"case": case, "nodes": n, "edges": e, "relations": r, "in": din, "out": dout, "bases": nb, "rows": int(rows.shape[0]),
           "block_edges": int(typ.shape[0])}
    for name, step in (("full_layer_step_ms", full_step), ("bipartite_step_ms", bip_step)):
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        rec[name] = round(median_ms(step, steps), 4)
    rec["full_over_bipartite"] = round(rec["full_layer_step_ms"] / rec["bipartite_step_ms"], 2)
    clear_plan_cache()
    return rec


def kernel_case(din, dout, steps, dev):
    from scaling_rgcn_training_amd import _lib
    rows = KERNEL_ROWS
    x, g = torch.randn(rows, din, device=dev), torch.randn(rows, dout, device=dev)
    w, bias = torch.randn(din, dout, device=dev), torch.randn(dout, device=dev)
    y = torch.zeros(rows, dout, device=dev)
    tf = lambda: _lib.rows_transform(x, din, w, dout, add=y, bias=bias, y=y)
    dw = lambda: _lib.rows_dw(x, din, g, dout)
    rec = {"case": f"kernels_{din}x{dout}", "rows": rows}
    for name, fn, nbytes in (("rows_transform", tf, rows * (din + 2 * dout) * 4), ("rows_dw", dw, rows * (din + dout) * 4)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = median_ms(fn, steps)
        rec[f"{name}_ms"] = round(ms, 4)
        rec[f"{name}_frac_6p3TBs"] = round(nbytes / (ms * 1e-3) / PEAK_BYTES, 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(list(CASES) + ["kernels"]))
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    dev = torch.device("cuda:0")
    for case in args.cases.split(","):
        if case == "kernels":
            for din, dout in KERNEL_WIDTHS:
                print(json.dumps(kernel_case(din, dout, args.steps, dev)), flush=True)
        else:
            print(json.dumps(layer_case(case, args.steps, dev)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
