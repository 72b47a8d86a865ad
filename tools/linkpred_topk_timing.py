#!/usr/bin/env python3
"""``linkpred.topk`` (csrc/rgcn_lp_topk.hip) on one MI355X, in one process, on 1M entities / 32 relations: DistMult at
dim 64 and 128, k = 10 and 64, 1,024 and 10,000 queries, unfiltered.  Beside it, in the same run and in turn with it, call by call:
  * ``torch``: chunks of 256 queries x 1M scores by ``matmul``, then ``torch.topk`` (the [Q, N] formulation, a chunk at a time);
  * ``ranks``: ``linkpred.ranks`` of the same queries, unfiltered, with arbitrary targets -- the same sweep without the selection, so
    the difference is what the selection costs.
Wall-clock medians after two warm-ups of every call, host clock around calls that end in a synchronise (tools/linkpred_timing.py's
method).  ``rows_equal_torch`` counts the queries whose k ids equal torch's (torch's matmul sums in another order, so near-ties may
differ); nothing here is a pass / fail criterion.
    python tools/linkpred_topk_timing.py [--steps 7] [--out profiles/linkpred_topk_timing.txt]
Writes one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NODES, RELATIONS, CHUNK = 1_000_000, 32, 256


def torch_topk(z, rel, a, r, k):
    ids, scores = [], []
    for c0 in range(0, a.shape[0], CHUNK):
        v, i = torch.topk((z[a[c0:c0 + CHUNK]] * rel[r[c0:c0 + CHUNK]]) @ z.t(), k, dim=1)
        ids.append(i)
        scores.append(v)
    return torch.cat(ids), torch.cat(scores)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linkpred_topk_timing.txt"))
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from scaling_rgcn_training_amd.linkpred import DistMult, ranks, topk
    assert torch.cuda.is_available(), "the timing needs the MI355X"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [json.dumps({"steps": args.steps, "method": "host clock around calls that end in a synchronise, median after two warm-ups, "
                         "the three calls of a case in turn", "device": torch.cuda.get_device_name(0), "entities": NODES,
                         "relations": RELATIONS, "torch_chunk_queries": CHUNK})]
    for dim in (64, 128):
        z = torch.randn(NODES, dim, device=dev, generator=gen)
        dec = DistMult(RELATIONS, dim).to(dev)
        rel = dec.rel.detach()
        for queries in (1024, 10_000):
            a = torch.randint(0, NODES, (queries,), device=dev, generator=gen)
            r = torch.randint(0, RELATIONS, (queries,), device=dev, generator=gen)
            t = torch.randint(0, NODES, (queries,), device=dev, generator=gen)
            for k in (10, 64):
                calls = {"hip_topk": lambda: topk(z, dec, a, r, k), "torch": lambda: torch_topk(z, rel, a, r, k),
                         "hip_ranks_raw": lambda: ranks(z, dec, a, r, t)}
                ts = {name: [] for name in calls}
                for step in range(-2, args.steps):              # two warm-ups of every call
                    for name, fn in calls.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        if step >= 0:
                            ts[name].append((time.perf_counter() - t0) * 1e3)
                rec = {"case": "topk", "dim": dim, "queries": queries, "k": k}
                for name in calls:
                    rec[name + "_ms"] = round(sorted(ts[name])[args.steps // 2], 4)
                    rec[name + "_ms_min_max"] = [round(min(ts[name]), 4), round(max(ts[name]), 4)]
                rec["torch_over_hip_topk"] = round(rec["torch_ms"] / rec["hip_topk_ms"], 2)
                rec["hip_topk_over_ranks_raw"] = round(rec["hip_topk_ms"] / rec["hip_ranks_raw_ms"], 2)
                rec["rows_equal_torch"] = int((topk(z, dec, a, r, k)[0] == torch_topk(z, rel, a, r, k)[0]).all(1).sum())
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
        del z
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
