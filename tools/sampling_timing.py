#!/usr/bin/env python3
"""Neighbour sampling (scaling_rgcn_training_amd/sampling.py) on one MI355X, on the 1M-node / 10M-edge / 32-relation
graph of tools/bipartite_timing.py: wall-clock medians (a hop synchronises once, so the host's share is part of its cost) of
  * the index build;
  * every hop and the whole ``sample()`` for 1,024 and 10,000 seeds at fan-outs (10, 10) and (25, 10);
  * the same blocks made by the torch form of tests/sampling_reference.py (``vectorised=True``) on the same GPU, checked equal;
  * one ``train_minibatch``-shaped step (Emb_Layers 64 -> 64 -> 16, 1,024 seeds, fan-outs (10, 10)) cut into sampling, building the
    blocks' graph plans, and the rest (gather, two layers forward + backward, Adam).
    python tools/sampling_timing.py [--steps 10] [--out profiles/sampling_timing.txt]
Writes one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NODES, EDGES, RELATIONS = 1_000_000, 10_000_000, 32
SEEDS = (1024, 10_000)
FANOUTS = ((10, 10), (25, 10))


def wall_ms(fn, steps, warmup=2):
    out = None
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return round(ts[len(ts) // 2], 4), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling_timing.txt"))
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from oracle import rgcn_oracle as O
    from scaling_rgcn_training_amd import _lib
    from scaling_rgcn_training_amd.layers import Emb_Layers
    from scaling_rgcn_training_amd.plan import clear_plan_cache
    from scaling_rgcn_training_amd.sampling import NeighborSampler
    from tests import sampling_reference as R
    dev = torch.device("cuda:0")
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    ei, et = O.synthetic_graph(NODES, EDGES, RELATIONS, seed=0)
    ei, et = ei.to(dev), et.to(dev)
    emit({"graph": {"nodes": NODES, "edges": EDGES, "relations": RELATIONS}, "device": torch.cuda.get_device_name(0), "steps": args.steps})
    ms, sampler = wall_ms(lambda: NeighborSampler(ei, et, NODES, RELATIONS), max(args.steps // 2, 3), warmup=1)
    ms_t, ix = wall_ms(lambda: R.build_index(ei, et, NODES), max(args.steps // 2, 3), warmup=1)
    emit({"case": "index_build", "hip_ms": ms, "torch_ms": ms_t})

    gen = torch.Generator(device=dev).manual_seed(0)
    for n_seeds in SEEDS:
        seeds = torch.randperm(NODES, device=dev, generator=gen)[:n_seeds]
        for fanouts in FANOUTS:
            hip_ms, blocks = wall_ms(lambda: sampler.sample(seeds, fanouts, 7), args.steps)
            torch_ms, ref = wall_ms(lambda: R.sample(ix, seeds, fanouts, 7, vectorised=True), args.steps)
            equal = all(torch.equal(getattr(a, f), getattr(b, f)) for a, b in zip(blocks, ref) for f in ("edge_index", "edge_type", "src_nodes"))
            rec = {"case": f"sample_{n_seeds}_{fanouts[0]}_{fanouts[1]}", "hip_sample_ms": hip_ms, "torch_sample_ms": torch_ms,
                   "torch_over_hip": round(torch_ms / hip_ms, 2), "blocks_equal": equal,
                   "blocks": [{"n_src": b.n_src, "n_dst": b.n_dst, "edges": int(b.edge_type.shape[0])} for b in blocks]}
            # every hop alone, on the destinations the whole call gives it (layer 1 from the seeds, layer 0 from layer 1's sources)
            for layer, dst in ((1, seeds), (0, blocks[1].src_nodes)):
                k = fanouts[layer]
                rec[f"hip_hop{layer}_ms"], _ = wall_ms(lambda: _lib.sample_hop(sampler._index, dst, k, 7, layer, sampler._map), args.steps)
                rec[f"torch_hop{layer}_ms"], _ = wall_ms(lambda: R.sample_block(ix, dst, k, 7, layer, vectorised=True), args.steps)
            emit(rec)

    # one mini-batch step, cut into its parts
    torch.manual_seed(0)
    model = Emb_Layers(RELATIONS, 64, 16, NODES, 64, None).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    seeds_all = torch.randperm(NODES, device=dev, generator=gen)
    target = torch.rand(1024, 16, device=dev)
    parts = {"sample": [], "plans": [], "rest": []}
    for step in range(args.steps + 2):
        seeds = seeds_all[step * 1024:(step + 1) * 1024]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        blocks = sampler.sample(seeds, (10, 10), step)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for conv, b in ((model.rgcn1, blocks[0]), (model.rgcn2, blocks[1])):      # (the forward below then finds them in the cache)
            conv._bipartite_plans(b.edge_index, b.edge_type, b.n_src, b.n_dst)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        opt.zero_grad()
        loss = torch.nn.functional.binary_cross_entropy(model.forward_blocks(blocks, torch.sigmoid), target)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if step >= 2:
            for name, dt in (("sample", t1 - t0), ("plans", t2 - t1), ("rest", t3 - t2)):
                parts[name].append(dt * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in parts.items()}
    total = sum(med.values())
    emit({"case": "minibatch_step_1024_10_10", "sample_ms": round(med["sample"], 4), "plans_ms": round(med["plans"], 4),
          "rest_ms": round(med["rest"], 4), "step_ms": round(total, 4), "sample_share": round(med["sample"] / total, 3),
          "plans_share": round(med["plans"] / total, 3)})
    clear_plan_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
