#!/usr/bin/env python3
"""Sparse embedding rows (sparse_optim.RowAdam, csrc/rgcn_emb_rows.hip) against the dense table path, on one MI355X.
Wall-clock medians of 10 after two warm-ups, host clock around calls that end in a synchronise (tools/minibatch_timing.py's method).
  * ``row_adam_86k``: ``RowAdam.step`` alone on 86,470 distinct rows x 64 of a 1M x 64 table (``assume_unique`` and through the
    sort), against ``torch.optim.Adam.step`` on the full table (its gradient already in place);
  * ``step_1M`` / ``step_10M``: the whole 1,024-seed (10, 10) ``Emb_Layers`` 64 -> 64 -> 16 step with ``block_kernels=True`` --
    sampling, zero_grad, forward, loss, backward, optimizer -- dense (``torch.optim.Adam`` over every parameter) against sparse
    (``embedding_rows`` + ``RowAdam``), in the same process, on the 1M-node / 10M-edge / 32-relation graph and the 10M / 100M one.
Every case runs in a child process of its own under a time limit; the first one that fails ends the run.
    python tools/sparse_embedding_timing.py [--steps 10] [--out profiles/sparse_embedding_timing.txt]
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

RELATIONS, EMB, HID, LABELS, SEEDS, FANOUTS = 32, 64, 64, 16, 1024, (10, 10)
GRAPHS = {"step_1M": (1_000_000, 10_000_000), "step_10M": (10_000_000, 100_000_000)}
ROWS_CASE, ROWS, ROWS_NODES = "row_adam_86k", 86_470, 1_000_000
CASE_LIMIT_S = {"row_adam_86k": 120, "step_1M": 240, "step_10M": 400}


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


def rows_case(steps):
    import __graft_entry__ as g
    g.build()
    from scaling_rgcn_training_amd.sparse_optim import RowAdam
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    table = torch.randn(ROWS_NODES, EMB, device=dev, generator=gen)
    nodes = torch.randperm(ROWS_NODES, device=dev, generator=gen)[:ROWS]
    grad = torch.randn(ROWS, EMB, device=dev, generator=gen)
    rows = RowAdam(table.clone(), 0.01)
    dense = torch.nn.Parameter(table.clone())
    dense.grad = torch.zeros_like(dense)
    dense.grad[nodes] = grad
    opt = torch.optim.Adam([dense], lr=0.01)
    rec = {"case": ROWS_CASE, "rows": ROWS, "width": EMB, "table_rows": ROWS_NODES,
           "row_adam_unique_ms": wall_ms(lambda: rows.step(nodes, grad, assume_unique=True), steps),
           "row_adam_sorted_ms": wall_ms(lambda: rows.step(nodes, grad), steps),
           "torch_adam_full_table_ms": wall_ms(opt.step, steps)}
    rows.check()
    rec["torch_over_row_adam_unique"] = round(rec["torch_adam_full_table_ms"] / rec["row_adam_unique_ms"], 2)
    return rec


def step_case(name, steps):
    import __graft_entry__ as g
    g.build()
    from oracle import rgcn_oracle as O
    from scaling_rgcn_training_amd.layers import Emb_Layers
    from scaling_rgcn_training_amd.sampling import NeighborSampler
    from scaling_rgcn_training_amd.sparse_optim import RowAdam
    nodes, edges = GRAPHS[name]
    dev = torch.device("cuda:0")
    ei, et = O.synthetic_graph(nodes, edges, RELATIONS, seed=0)
    ei, et = ei.to(dev), et.to(dev)
    sampler = NeighborSampler(ei, et, nodes, RELATIONS)
    gen = torch.Generator(device=dev).manual_seed(0)
    seeds_all = torch.randperm(nodes, device=dev, generator=gen)
    target = torch.rand(SEEDS, LABELS, device=dev)
    rec = {"case": name, "graph": {"nodes": nodes, "edges": edges, "relations": RELATIONS}, "seeds": SEEDS, "fanouts": list(FANOUTS)}
    for sparse in (False, True):
        torch.manual_seed(0)
        model = Emb_Layers(RELATIONS, HID, LABELS, nodes, EMB, None).to(dev)
        table = model.embedding_table()
        if sparse:
            opt = torch.optim.Adam([p for p in model.parameters() if p is not table], lr=0.01)
            rows = RowAdam(table, 0.01)
        else:
            opt = torch.optim.Adam(model.parameters(), lr=0.01)
        parts = {"sample": [], "rest": []}
        n_src = []
        for step in range(steps + 2):
            seeds = seeds_all[step * SEEDS:(step + 1) * SEEDS]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            blocks = sampler.sample(seeds, FANOUTS, step)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            opt.zero_grad()
            if sparse:
                emb_rows = model.embedding_rows(blocks[0].src_nodes)
                out = model.forward_blocks_from_rows(blocks, torch.sigmoid, emb_rows, True)
            else:
                out = model.forward_blocks(blocks, torch.sigmoid, True)
            torch.nn.functional.binary_cross_entropy(out, target).backward()
            opt.step()
            if sparse:
                rows.step(blocks[0].src_nodes, emb_rows.grad, assume_unique=True)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if step >= 2:
                parts["sample"].append((t1 - t0) * 1e3)
                parts["rest"].append((t2 - t1) * 1e3)
                n_src.append(blocks[0].n_src)
        if sparse:
            rows.check()
        med = {k: sorted(v)[len(v) // 2] for k, v in parts.items()}
        rec["sparse" if sparse else "dense"] = {"sample_ms": round(med["sample"], 4), "rest_ms": round(med["rest"], 4),
                                                "step_ms": round(sum(med.values()), 4), "n_src_median": sorted(n_src)[len(n_src) // 2]}
        del model, opt, table
        torch.cuda.empty_cache()
    rec["dense_over_sparse"] = round(rec["dense"]["step_ms"] / rec["sparse"]["step_ms"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_embedding_timing.txt"))
    ap.add_argument("--case", default=None, help="run one case in this process and print its JSON line (what the driver starts)")
    args = ap.parse_args()
    names = [ROWS_CASE] + list(GRAPHS)
    if args.case is not None:
        rec = rows_case(args.steps) if args.case == ROWS_CASE else step_case(args.case, args.steps)
        print("RESULT " + json.dumps(rec), flush=True)
        return 0
    lines = [json.dumps({"steps": args.steps, "method": "host clock around calls that end in a synchronise, median after two warm-ups"})]
    for name in names:
        limit = CASE_LIMIT_S[name]
        print(f"{name}: started (limit {limit} s)", flush=True)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--case", name],
                               capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {limit} s; stopping", flush=True)
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
