#!/usr/bin/env python3
"""Featureless RGCNConv (csrc/rgcn_featureless.hip): ms per forward and per backward at two shapes, against the byte model of
DESIGN.md "Featureless layers":
  forward  = gathered rows slots x round4(out) x 4 (x B with bases) + 12 B of plan per slot + N x out x 4 of output
  backward = the dense d_weight store R' x in x out x 4 (bases: B x in x out x 4 of d_V) + the transposed walk (g rows + plan)
    python tools/featureless_timing.py [--shapes aifb,am] [--steps 20]
Prints one JSON line per (shape, weights): HIP-event medians of the forward call and of the backward call, and the fraction of
8 TB/s the model's bytes take in that time.  Kernel-only times: run under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"aifb": (8285, 58086, 90), "am": (1_500_000, 6_000_000, 267)}
PEAK = 8.0e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="aifb,am")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", type=int, default=16)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from scaling_rgcn_training_amd.conv import RGCNConv
    dev = torch.device("cuda:0")
    for shape in args.shapes.split(","):
        n, e, r = SHAPES[shape]
        gen = torch.Generator(device=dev).manual_seed(0)
        ei = torch.randint(0, n, (2, e), device=dev, generator=gen)
        et = torch.randint(0, r, (e,), device=dev, generator=gen)
        for nb in (None, 30):
            conv = RGCNConv(n, args.out, r, num_bases=nb, featureless=True).to(dev)
            out = conv(None, ei, et)
            gout = torch.randn_like(out)
            out.backward(gout)
            torch.cuda.synchronize()
            fwd_ms = median_ms(lambda: conv(None, ei, et), args.steps)
            out = conv(None, ei, et)

            def bwd():
                for p in conv.parameters():
                    p.grad = None
                torch.autograd.backward(out, gout, retain_graph=True)
            bwd_ms = median_ms(bwd, args.steps)
            d4 = (args.out + 3) // 4 * 4
            slots = e + n                       # edges + root pseudo edges (duplicates of random graphs: negligible)
            b = 1 if nb is None else nb
            fwd_bytes = slots * d4 * 4 * b + 12 * slots + n * args.out * 4
            tables = r if nb is None else nb
            bwd_bytes = tables * n * args.out * 4 + slots * (d4 * 4 + 12) + n * args.out * 4
            print(json.dumps({"shape": shape, "nodes": n, "edges": e, "relations": r, "out": args.out,
                              "weights": "full" if nb is None else f"basis{nb}", "fwd_ms": round(fwd_ms, 4),
                              "bwd_ms": round(bwd_ms, 4), "fwd_model_bytes": fwd_bytes, "bwd_model_bytes": bwd_bytes,
                              "fwd_frac_8TBs": round(fwd_bytes / (fwd_ms * 1e-3) / PEAK, 3),
                              "bwd_frac_8TBs": round(bwd_bytes / (bwd_ms * 1e-3) / PEAK, 3)}), flush=True)
            del conv, out, gout
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
