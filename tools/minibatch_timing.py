#!/usr/bin/env python3
"""Mini-batch layers straight from sampled blocks (RGCNConv.forward_block, csrc/rgcn_minibatch.hip) against the
bipartite layer on graph plans, on one MI355X, on the graph and the four sample cases of profiles/sampling_timing.txt (1M nodes /
10M edges / 32 relations; 1,024 and 10,000 seeds at fan-outs (10, 10) and (25, 10)).  Wall-clock medians of 10 after two warm-ups,
host clock around calls that end in a synchronise (tools/sampling_timing.py's method).  Per case:
  * the index build of each block (``sampling.block_index``);
  * each layer's forward + backward (layer 0: 64 -> 64 on blocks[0], layer 1: 64 -> 16 on blocks[1]; x requires a gradient)
      - ``block_ms``: ``forward_block`` building its own index -- what a step pays;
      - ``block_prebuilt_ms``: the same with the index given -- the kernels alone;
      - ``bipartite_fresh_ms``: ``conv((x, x[:n_dst]), ...)`` on fresh block tensors, plan build included -- what a step pays today;
      - ``bipartite_warm_ms``: the same on tensors whose plans are cached -- the kernels alone.
``minibatch_step_1024_10_10``: the whole Emb_Layers 64 -> 64 -> 16 step (sampling, plans or nothing, the rest) both ways.
Every case runs in a child process of its own under a time limit; the first one that fails ends the run.
    python tools/minibatch_timing.py [--steps 10] [--out profiles/minibatch_timing.txt]
Writes one JSON line per measurement."""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NODES, EDGES, RELATIONS = 1_000_000, 10_000_000, 32
CASES = [(1024, (10, 10)), (1024, (25, 10)), (10_000, (10, 10)), (10_000, (25, 10))]
STEP_CASE = "minibatch_step_1024_10_10"
CASE_LIMIT_S = 240


def wall_ms(fn, steps, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return round(ts[len(ts) // 2], 4)


def _setup():
    import __graft_entry__ as g
    g.build()
    from oracle import rgcn_oracle as O
    from scaling_rgcn_training_amd.sampling import NeighborSampler
    dev = torch.device("cuda:0")
    ei, et = O.synthetic_graph(NODES, EDGES, RELATIONS, seed=0)
    ei, et = ei.to(dev), et.to(dev)
    return dev, NeighborSampler(ei, et, NODES, RELATIONS)


def sample_case(n_seeds, fanouts, steps):
    from scaling_rgcn_training_amd.conv import RGCNConv
    from scaling_rgcn_training_amd.plan import clear_plan_cache
    from scaling_rgcn_training_amd.sampling import Block, block_index
    dev, sampler = _setup()
    gen = torch.Generator(device=dev).manual_seed(0)
    seeds = torch.randperm(NODES, device=dev, generator=gen)[:n_seeds]
    blocks = sampler.sample(seeds, fanouts, 7)
    rec = {"case": f"sample_{n_seeds}_{fanouts[0]}_{fanouts[1]}", "layers": []}
    torch.manual_seed(0)
    for layer, (b, (din, dout)) in enumerate(zip(blocks, ((64, 64), (64, 16)))):
        conv = RGCNConv(din, dout, RELATIONS).to(dev)
        x = torch.randn(b.n_src, din, device=dev, requires_grad=True)
        g = torch.randn(b.n_dst, dout, device=dev)
        ix = block_index(b, RELATIONS)

        def block_step(index=None):
            conv.zero_grad()
            x.grad = None
            conv.forward_block(x, b, index).backward(g)

        def bipartite_step(blk):
            conv.zero_grad()
            x.grad = None
            conv((x, x[:blk.n_dst]), blk.edge_index, blk.edge_type).backward(g)

        def fresh():      # new tensors, as every step's sample() returns them: the plan cache cannot hit
            bipartite_step(Block(b.edge_index.clone(), b.edge_type.clone(), b.n_src, b.n_dst, b.src_nodes))

        out = {"layer": layer, "widths": [din, dout], "n_src": b.n_src, "n_dst": b.n_dst, "edges": int(b.edge_type.shape[0]),
               "rows": ix.n_rows, "tiles": ix.n_tiles,
               "index_build_ms": wall_ms(lambda: block_index(b, RELATIONS), steps),
               "block_ms": wall_ms(block_step, steps),
               "block_prebuilt_ms": wall_ms(lambda: block_step(ix), steps),
               "bipartite_fresh_ms": wall_ms(fresh, steps),
               "bipartite_warm_ms": wall_ms(lambda: bipartite_step(b), steps)}
        out["fresh_over_block"] = round(out["bipartite_fresh_ms"] / out["block_ms"], 2)
        out["warm_over_prebuilt"] = round(out["bipartite_warm_ms"] / out["block_prebuilt_ms"], 2)
        rec["layers"].append(out)
        clear_plan_cache()
    return rec


def step_case(steps):
    from scaling_rgcn_training_amd.layers import Emb_Layers
    from scaling_rgcn_training_amd.plan import clear_plan_cache
    dev, sampler = _setup()
    gen = torch.Generator(device=dev).manual_seed(0)
    seeds_all = torch.randperm(NODES, device=dev, generator=gen)
    target = torch.rand(1024, 16, device=dev)
    rec = {"case": STEP_CASE}
    for block_kernels in (False, True):
        torch.manual_seed(0)
        model = Emb_Layers(RELATIONS, 64, 16, NODES, 64, None).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=0.01)
        parts = {"sample": [], "plans": [], "rest": []}
        for step in range(steps + 2):
            seeds = seeds_all[step * 1024:(step + 1) * 1024]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            blocks = sampler.sample(seeds, (10, 10), step)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if not block_kernels:      # (the forward below then finds them in the cache; the block kernels' index build is part of "rest")
                for conv, b in ((model.rgcn1, blocks[0]), (model.rgcn2, blocks[1])):
                    conv._bipartite_plans(b.edge_index, b.edge_type, b.n_src, b.n_dst)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            opt.zero_grad()
            loss = torch.nn.functional.binary_cross_entropy(model.forward_blocks(blocks, torch.sigmoid, block_kernels), target)
            loss.backward()
            opt.step()
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            if step >= 2:
                for name, dt in (("sample", t1 - t0), ("plans", t2 - t1), ("rest", t3 - t2)):
                    parts[name].append(dt * 1e3)
        med = {k: sorted(v)[len(v) // 2] for k, v in parts.items()}
        rec["block_kernels" if block_kernels else "graph_plans"] = {
            "sample_ms": round(med["sample"], 4), "plans_ms": round(med["plans"], 4), "rest_ms": round(med["rest"], 4),
            "step_ms": round(sum(med.values()), 4)}
        clear_plan_cache()
    rec["plans_over_block_kernels"] = round(rec["graph_plans"]["step_ms"] / rec["block_kernels"]["step_ms"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minibatch_timing.txt"))
    ap.add_argument("--case", default=None, help="run one case in this process and print its JSON line (what the driver starts)")
    args = ap.parse_args()
    names = [f"sample_{n}_{f[0]}_{f[1]}" for n, f in CASES] + [STEP_CASE]
    if args.case is not None:
        rec = step_case(args.steps) if args.case == STEP_CASE else sample_case(*CASES[names.index(args.case)], args.steps)
        print("RESULT " + json.dumps(rec), flush=True)
        return 0
    lines = [json.dumps({"graph": {"nodes": NODES, "edges": EDGES, "relations": RELATIONS}, "steps": args.steps,
                         "method": "host clock around calls that end in a synchronise, median after two warm-ups"})]
    for name in names:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--case", name],
                               capture_output=True, text=True, timeout=CASE_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {CASE_LIMIT_S} s; stopping", flush=True)
            return 1
        got = [l[7:] for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not got:
            print(f"{name}: exit {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
            return 1
        lines.append(got[-1])
        print(got[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
