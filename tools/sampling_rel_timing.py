#!/usr/bin/env python3
"""Neighbour sampling with one fan-out per relation (scaling_rgcn_training_amd/sampling.py) on one MI355X, on the
1M-node / 10M-edge / 32-relation graph of tools/sampling_timing.py: wall-clock medians (a hop synchronises once, so the host's
share is part of its cost; median of ``--steps`` after two warm-ups) of
  * the relation-index build, beside the in-edge index build of the scalar path;
  * every hop and the whole ``sample()`` for 1,024 and 10,000 seeds at ``[2] * 32`` and ``[10] * 32`` on both layers;
  * the scalar (10, 10) ``sample()`` and its hops, in the same run;
  * the same blocks made by the torch form of tests/sampling_rel_reference.py (``vectorised=True``: a stable sort by
    ``dst * R + type`` + a per-run choice) on the same GPU, checked equal;
  * the per-kernel split of one hop (10,000 seeds' layer-0 hop at ``[10] * 32``), device time by torch.profiler.
    python tools/sampling_rel_timing.py [--steps 10] [--out profiles/sampling_rel_timing.txt]
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
REL_FANOUTS = (2, 10)
SCALAR = (10, 10)


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


def kernel_split(fn, calls=5):
    """device microseconds per kernel name, averaged over ``calls`` calls of ``fn``"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    rows = {}
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None)
        if t is None:
            t = getattr(ev, "cuda_time_total", 0.0)
        if t:
            rows[ev.key.split("(")[0][-60:]] = [round(t / calls, 2), ev.count // calls]
    return dict(sorted(rows.items(), key=lambda kv: -kv[1][0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling_rel_timing.txt"))
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from oracle import rgcn_oracle as O
    from scaling_rgcn_training_amd import _lib
    from scaling_rgcn_training_amd.sampling import NeighborSampler
    from tests import sampling_reference as R
    from tests import sampling_rel_reference as RR
    dev = torch.device("cuda:0")
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def equal(blocks, ref):
        return all(torch.equal(getattr(a, f), getattr(b, f)) for a, b in zip(blocks, ref) for f in ("edge_index", "edge_type", "src_nodes"))

    ei, et = O.synthetic_graph(NODES, EDGES, RELATIONS, seed=0)
    ei, et = ei.to(dev), et.to(dev)
    emit({"graph": {"nodes": NODES, "edges": EDGES, "relations": RELATIONS}, "device": torch.cuda.get_device_name(0), "steps": args.steps})
    few = max(args.steps // 2, 3)
    ms, sampler = wall_ms(lambda: NeighborSampler(ei, et, NODES, RELATIONS), few, warmup=1)
    ms_t, ix = wall_ms(lambda: R.build_index(ei, et, NODES), few, warmup=1)
    graph, keep = _lib.graph_struct(ei, et, NODES, RELATIONS)
    ms_r, _ = wall_ms(lambda: _lib.sample_rel_index_build(graph, dev), few, warmup=1)
    ms_rt, rx = wall_ms(lambda: RR.build_rel_index(ei, et, NODES, RELATIONS), few, warmup=1)
    rindex = sampler._relation_index()
    run_len = rx.run_beg[1:] - rx.run_beg[:-1]
    emit({"case": "index_build", "hip_ms": ms, "torch_ms": ms_t, "rel_hip_ms": ms_r, "rel_torch_ms": ms_rt,
          "num_runs": int(rindex.num_runs), "num_runs_equal": int(rindex.num_runs) == rx.num_runs,
          "longest_run": int(run_len.max()), "runs_longer_than_2": int((run_len > 2).sum()), "runs_longer_than_10": int((run_len > 10).sum())})

    def sampled_units(dst, k):
        first, last = rx.run_ptr[dst], rx.run_ptr[dst + 1]
        n_run = last - first
        q = torch.repeat_interleave(first - (torch.cumsum(n_run, 0) - n_run), n_run) + torch.arange(int(n_run.sum()), device=dev)
        return int(n_run.sum()), int((run_len[q] > k).sum())

    gen = torch.Generator(device=dev).manual_seed(0)
    split_case = None
    for n_seeds in SEEDS:
        seeds = torch.randperm(NODES, device=dev, generator=gen)[:n_seeds]
        hip_ms, blocks = wall_ms(lambda: sampler.sample(seeds, SCALAR, 7), args.steps)
        rec = {"case": f"scalar_{n_seeds}_{SCALAR[0]}_{SCALAR[1]}", "hip_sample_ms": hip_ms,
               "blocks": [{"n_src": b.n_src, "n_dst": b.n_dst, "edges": int(b.edge_type.shape[0])} for b in blocks]}
        for layer, dst in ((1, seeds), (0, blocks[1].src_nodes)):
            rec[f"hip_hop{layer}_ms"], _ = wall_ms(lambda: _lib.sample_hop(sampler._index, dst, SCALAR[layer], 7, layer, sampler._map),
                                                   args.steps)
        emit(rec)
        for k in REL_FANOUTS:
            vec = [k] * RELATIONS
            fanouts = (vec, vec)
            hip_ms, blocks = wall_ms(lambda: sampler.sample(seeds, fanouts, 7), args.steps)
            torch_ms, ref = wall_ms(lambda: RR.sample_rel(ix, rx, seeds, fanouts, 7, vectorised=True), args.steps)
            rec = {"case": f"rel_{n_seeds}_{k}x{RELATIONS}", "hip_sample_ms": hip_ms, "torch_sample_ms": torch_ms,
                   "torch_over_hip": round(torch_ms / hip_ms, 2), "blocks_equal": equal(blocks, ref),
                   "blocks": [{"n_src": b.n_src, "n_dst": b.n_dst, "edges": int(b.edge_type.shape[0])} for b in blocks]}
            for layer, dst in ((1, seeds), (0, blocks[1].src_nodes)):
                rec[f"hip_hop{layer}_ms"], _ = wall_ms(lambda: _lib.sample_hop_rel(rindex, dst, vec, 7, layer, sampler._map), args.steps)
                rec[f"torch_hop{layer}_ms"], _ = wall_ms(lambda: RR.sample_block_rel(rx, dst, vec, 7, layer, vectorised=True), args.steps)
                rec[f"hop{layer}_units"], rec[f"hop{layer}_sampled_units"] = sampled_units(dst, k)
            emit(rec)
            if n_seeds == SEEDS[-1] and k == REL_FANOUTS[-1]:
                split_case = (blocks[1].src_nodes, vec)
    dst, vec = split_case
    for k in REL_FANOUTS:
        v = [k] * RELATIONS
        emit({"case": f"kernel_split_us_hop0_{SEEDS[-1]}_{k}x{RELATIONS}", "n_dst": int(dst.shape[0]),
              "kernels": kernel_split(lambda: _lib.sample_hop_rel(rindex, dst, v, 7, 0, sampler._map))})
    emit({"case": f"kernel_split_us_scalar_hop0_{SEEDS[-1]}_{SCALAR[0]}", "n_dst": int(dst.shape[0]),
          "kernels": kernel_split(lambda: _lib.sample_hop(sampler._index, dst, SCALAR[0], 7, 0, sampler._map))})
    del keep
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
