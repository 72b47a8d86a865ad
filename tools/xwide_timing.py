#!/usr/bin/env python3
"""RGCNConv wider than 128 (``wide=True``, csrc/rgcn_xwide.hip): ms per forward, per backward and per step (forward + backward,
dX included) at the shapes of DESIGN.md §10, against the FLOP and byte models there and against the same step through PyG's
per-relation loop in torch ops (``oracle.rgcn_conv_loop`` under autograd on the GPU: what a user has without this feature).
  useful FLOP  = 2 (E + N) in out per direction (forward, dX) + the same for d_W            (slots: E + N, root pseudo edges)
  bytes        = forward: slots (in x 4 + 12) + N out 4; dX: slots (out x 4 + 12) + N in 4; d_W: slots (in + out) 4 + 12 slots
    python tools/xwide_timing.py [--cases aifb_256_256,...] [--steps 10]
Prints one JSON line per case: HIP-event medians, fractions of 155 TF (fp32 MFMA, MI355X_MICROARCH.md) and of 6.3 TB/s.
Kernel-only times: run under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GRAPHS = {"aifb": (8285, 58086, 90), "1m": (1_000_000, 10_000_000, 32)}
CASES = {"aifb_256_256": ("aifb", 256, 256), "aifb_256_4": ("aifb", 256, 4), "1m_256_256": ("1m", 256, 256),
         "1m_512_64": ("1m", 512, 64), "1m_64_512": ("1m", 64, 512)}
PEAK_FLOPS, PEAK_BYTES = 155e12, 6.3e12


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
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--loop-steps", type=int, default=3)
    ap.add_argument("--no-loop", action="store_true", help="skip the torch loop baseline")
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from oracle.rgcn_oracle import rgcn_conv_loop
    from scaling_rgcn_training_amd.conv import RGCNConv
    dev = torch.device("cuda:0")
    for case in args.cases.split(","):
        gname, din, dout = CASES[case]
        n, e, r = GRAPHS[gname]
        gen = torch.Generator(device=dev).manual_seed(0)
        ei = torch.randint(0, n, (2, e), device=dev, generator=gen)
        et = torch.randint(0, r, (e,), device=dev, generator=gen)
        x = torch.randn(n, din, device=dev, generator=gen).requires_grad_(True)
        gout = torch.randn(n, dout, device=dev, generator=gen)
        conv = RGCNConv(din, dout, r, wide=True).to(dev)
        assert conv.xwide or max(din, dout) <= 128

        def step():
            x.grad = None
            for p in conv.parameters():
                p.grad = None
            conv(x, ei, et).backward(gout)

        step()
        torch.cuda.synchronize()
        fwd_ms = median_ms(lambda: conv(x, ei, et), args.steps)
        out = conv(x, ei, et)

        def bwd():
            x.grad = None
            for p in conv.parameters():
                p.grad = None
            torch.autograd.backward(out, gout, retain_graph=True)
        bwd_ms = median_ms(bwd, args.steps)
        step_ms = median_ms(step, args.steps)
        del out
        loop_ms = None
        if not args.no_loop:
            def loop_step():
                x.grad = None
                for p in conv.parameters():
                    p.grad = None
                rgcn_conv_loop(x, ei, et, conv.weight, conv.root, conv.bias).backward(gout)
            loop_step()
            torch.cuda.synchronize()
            loop_ms = median_ms(loop_step, args.loop_steps)
        slots = e + n
        flop_dir = 2.0 * slots * din * dout
        step_flop = 3 * flop_dir
        fwd_bytes = slots * (din * 4 + 12) + n * dout * 4
        bwd_bytes = slots * (dout * 4 + 12) + n * din * 4 + slots * (din + dout) * 4 + 12 * slots
        rec = {"case": case, "nodes": n, "edges": e, "relations": r, "in": din, "out": dout,
               "fwd_ms": round(fwd_ms, 4), "bwd_ms": round(bwd_ms, 4), "step_ms": round(step_ms, 4),
               "torch_loop_step_ms": None if loop_ms is None else round(loop_ms, 3),
               "speedup_vs_loop": None if loop_ms is None else round(loop_ms / step_ms, 2),
               "step_useful_gflop": round(step_flop / 1e9, 2),
               "fwd_frac_155TF": round(flop_dir / (fwd_ms * 1e-3) / PEAK_FLOPS, 3),
               "bwd_frac_155TF": round(2 * flop_dir / (bwd_ms * 1e-3) / PEAK_FLOPS, 3),
               "step_frac_155TF": round(step_flop / (step_ms * 1e-3) / PEAK_FLOPS, 3),
               "step_model_bytes": fwd_bytes + bwd_bytes,
               "step_frac_6p3TBs": round((fwd_bytes + bwd_bytes) / (step_ms * 1e-3) / PEAK_BYTES, 3)}
        print(json.dumps(rec), flush=True)
        del conv, x, gout, ei, et
        from scaling_rgcn_training_amd.plan import clear_plan_cache
        clear_plan_cache()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
