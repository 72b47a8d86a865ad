#!/usr/bin/env python3
"""The softmax link-prediction loss (scaling_rgcn_training_amd/linkpred.py ``softmax_loss``, csrc/rgcn_lp_softmax.hip)
against its torch formulation (``matmul`` + ``logsumexp`` + autograd on [Q, N] logits), on one MI355X, in one process, in the manner
of tools/kge_timing.py: wall-clock medians after two warm-ups, host clock around calls that end in a synchronise.  DistMult, 1M
entities, 32 relations, dim 64 and 128:
  * Q = 1,024: forward, and forward + backward, both arms; the two sweeps also alone, with their achieved fp32 MFMA rate (forward
    2 Q N dim flop; backward, dq and dz with two products each, 8 Q N dim) beside ``lp_rank``'s of profiles/linkpred_timing.txt;
  * Q = 10,000: the kernels only, and the bytes the torch formulation would need for its logits and their gradient.
    python tools/lp_softmax_timing.py [--steps 10] [--out profiles/lp_softmax_timing.txt]
Writes one JSON line per measurement."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from linkpred_timing import NODES, RELATIONS, wall_ms  # noqa: E402

LP_RANK_TFLOPS = 86.33      # hip_raw_tflops_fp32 of the "ranks" line of profiles/linkpred_timing.txt (dim 64, 10,000 queries)
LPW_RANK_TFLOPS = 112.0     # lpw_rank's sweep at 512 columns (profiles/linkpred_wide_timing.txt)


def torch_loss(z, rel, s, r, o):
    logits = (z[s] * rel[r]) @ z.t()
    return torch.logsumexp(logits, 1) - logits.gather(1, o[:, None])[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_softmax_timing.txt"))
    ap.add_argument("--dim", type=int, nargs="+", default=[64, 128],
                    help="widths to time; above 128 a DistMult(..., wide=True) on csrc/rgcn_lp_softmax_wide.hip (DESIGN.md 24)")
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from scaling_rgcn_training_amd import _lib
    from scaling_rgcn_training_amd.linkpred import DistMult, softmax_loss
    assert torch.cuda.is_available(), "the timing needs the MI355X"
    dev, steps = torch.device("cuda:0"), args.steps
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [json.dumps({"steps": steps, "method": "host clock around calls that end in a synchronise, median after two warm-ups",
                         "device": torch.cuda.get_device_name(0), "entities": NODES, "relations": RELATIONS, "decoder": "distmult",
                         "lp_rank_tflops_fp32_dim64": LP_RANK_TFLOPS, "lpw_rank_tflops_fp32_dim512": LPW_RANK_TFLOPS})]

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for dim in args.dim:
        z = (torch.randn(NODES, dim, device=dev, generator=gen) * 0.3).requires_grad_(True)
        dec = DistMult(RELATIONS, dim, wide=dim > 128).to(dev)
        for queries in (1024, 10000):
            s, o = (torch.randint(0, NODES, (queries,), device=dev, generator=gen) for _ in range(2))
            r = torch.randint(0, RELATIONS, (queries,), device=dev, generator=gen)
            gout = torch.randn(queries, device=dev, generator=gen)

            def fb(loss_fn):
                z.grad = dec.rel.grad = None
                loss_fn().backward(gout)

            ours = lambda: softmax_loss(z, dec, s, r, o, wide=True)
            rec = {"case": "softmax_loss", "dim": dim, "queries": queries, "hip_forward_ms": wall_ms(lambda: ours().detach(), steps),
                   "hip_forward_backward_ms": wall_ms(lambda: fb(ours), steps)}
            mine = (ours().detach(), z.grad.clone(), dec.rel.grad.clone())
            zp, rp = z.detach(), dec.rel.detach()
            qrows, qt = _lib.lpsm_query(_lib.LPSM_DISTMULT, 0, zp, rp, s, r, o)
            lse, _, _ = _lib.lpsm_forward(qrows, zp, qt)
            pair_columns = queries * NODES * dim
            rec["hip_forward_sweep_ms"] = wall_ms(lambda: _lib.lpsm_forward(qrows, zp, qt), steps)
            rec["hip_backward_sweeps_ms"] = wall_ms(lambda: _lib.lpsm_backward(qrows, zp, qt, lse, gout), steps)
            rec["hip_dq_sweep_ms"] = wall_ms(lambda: _lib.lpsm_backward(qrows, zp, qt, lse, gout, False), steps)
            rec["forward_sweep_tflops_fp32"] = round(2 * pair_columns / (rec["hip_forward_sweep_ms"] * 1e-3) / 1e12, 2)
            rec["backward_sweeps_tflops_fp32"] = round(8 * pair_columns / (rec["hip_backward_sweeps_ms"] * 1e-3) / 1e12, 2)
            if queries == 1024:
                theirs = lambda: torch_loss(z, dec.rel, s, r, o)
                rec["torch_forward_ms"] = wall_ms(lambda: theirs().detach(), steps)
                rec["torch_forward_backward_ms"] = wall_ms(lambda: fb(theirs), steps)
                rec["torch_over_hip_forward"] = round(rec["torch_forward_ms"] / rec["hip_forward_ms"], 2)
                rec["torch_over_hip_forward_backward"] = round(rec["torch_forward_backward_ms"] / rec["hip_forward_backward_ms"], 2)
                rec["max_abs_diff_loss"] = float((theirs().detach() - mine[0]).abs().max())
                rec["max_abs_diff_dz_over_max"] = float((z.grad - mine[1]).abs().max() / z.grad.abs().max())
                rec["max_abs_diff_drel_over_max"] = float((dec.rel.grad - mine[2]).abs().max() / dec.rel.grad.abs().max())
            else:       # not allocated: the logits, and as much again for their gradient
                rec["torch_logits_bytes_not_allocated"] = 4 * queries * NODES
                rec["torch_logits_and_gradient_bytes_not_allocated"] = 8 * queries * NODES
            emit(rec)
            z.grad = dec.rel.grad = None
            torch.cuda.empty_cache()
        dec.check()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
