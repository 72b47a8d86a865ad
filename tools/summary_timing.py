#!/usr/bin/env python3
"""Graph summaries on the GPU (csrc/rgcn_summary.hip: summaries.node_partition / quotient_graph): wall time of
  * one refinement round, for rounds 1, 2 and 3 from the trivial partition, in every direction (a round ends in its one
    read-back, so a round's time is a host clock around the call; device events around the same call are reported beside it);
  * the whole ``node_partition(k=3)`` call (argument checks, workspace and all);
  * the deduplicated quotient graph of the k = 3 "out" partition;
  * ``build_graph_plans`` on the same graph in the same process -- the project's existing sort-bound yardstick;
  * the same three rounds written with ``torch.unique(dim=0)`` on the device: what a user would write without this library
    (it lives here only; the package ships no torch form)
on the headline synthetic graph (10M nodes / 100M edges / 32 relations) and the AM-like one (1.5M / 6M / 267).
    python tools/summary_timing.py [--cases am,headline] [--repeats 5] [--torch-repeats 2]
Prints one JSON line per case: medians in ms with (min, max) over the repeats after one warm-up of every shape."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {"am": (1_500_000, 6_000_000, 267), "headline": (10_000_000, 100_000_000, 32), "100k": (100_000, 1_000_000, 32)}
DIRECTIONS = ("out", "in", "in_out")


def spread(ts):
    ts = sorted(ts)
    return [round(ts[len(ts) // 2], 3), round(ts[0], 3), round(ts[-1], 3)]      # median, min, max


def timed(fn, repeats, warmup=1):
    """(host ms [median, min, max], device-event ms [median, min, max]) of fn(), which may synchronise inside"""
    host, devt = [], []
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if i >= warmup:
            host.append((t1 - t0) * 1e3)
            devt.append(a.elapsed_time(b))
    return spread(host), spread(devt)


def torch_round(ei, et, block, n, direction, gen_words):
    """one refinement round in torch ops: distinct (owner, element) rows by torch.unique(dim=0), a two-word random signature per
    owner by index_add, classes by torch.unique(dim=0) over (block, signature), canonical ids by the smallest member"""
    src, dst = ei[0], ei[1]
    if direction == "out":
        rows = torch.stack([src, et, block[dst]], 1)
    elif direction == "in":
        rows = torch.stack([dst, et, block[src]], 1)
    else:
        z = torch.zeros_like(et)
        rows = torch.cat([torch.stack([src, z, et, block[dst]], 1), torch.stack([dst, z + 1, et, block[src]], 1)])
    rows = torch.unique(rows, dim=0)
    elem = torch.unique(rows[:, 1:], dim=0, return_inverse=True)[1]
    words = gen_words(int(elem.max()) + 1 if elem.numel() else 1)
    sig = torch.zeros(n, 2, dtype=torch.int64, device=ei.device).index_add_(0, rows[:, 0], words[elem])
    cls = torch.unique(torch.cat([block[:, None], sig], 1), dim=0, return_inverse=True)[1]
    nb = int(cls.max()) + 1
    first = torch.full((nb,), n, dtype=torch.int64, device=ei.device).scatter_reduce_(
        0, cls, torch.arange(n, device=ei.device), "amin")
    rank = torch.empty_like(first)
    rank[torch.argsort(first)] = torch.arange(nb, device=ei.device)
    return rank[cls], nb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="am,headline")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch-repeats", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch.unique baseline")
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from oracle import rgcn_oracle as O
    from scaling_rgcn_training_amd import _lib, summaries as S
    from scaling_rgcn_training_amd.plan import build_graph_plans
    dev = torch.device("cuda:0")
    for case in args.cases.split(","):
        n, e, r = CASES[case]
        ei, et = O.synthetic_graph(n, e, r, seed=0)
        ei, et = ei.to(dev), et.to(dev)
        rec = {"case": case, "nodes": n, "edges": e, "relations": r, "repeats": args.repeats, "format": "[median, min, max] ms"}
        graph, keep = _lib.graph_struct(ei, et, n, r)
        blocks = {}
        note = lambda what: print(f"[{case}] {what}", file=sys.stderr, flush=True)
        for d in DIRECTIONS:
            note(f"rounds, {d}")
            dd = _lib.SUMMARY_DIRECTIONS[d]
            ws = _lib.summary_workspace(e, n, dd, dev)
            rec[f"workspace_gb_{d}"] = round(ws.numel() / 1e9, 2)
            cur, nxt, nb = torch.zeros(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev), 1
            for rnd in (1, 2, 3):
                out = {}
                host, devt = timed(lambda: out.__setitem__("nb", _lib.summary_round(graph, dd, cur, nb, nxt, ws)), args.repeats)
                rec[f"round{rnd}_{d}_ms"], rec[f"round{rnd}_{d}_event_ms"] = host, devt
                rec[f"round{rnd}_{d}_blocks"] = out["nb"]
                cur, nxt, nb = nxt, cur, out["nb"]
            blocks[d] = (cur.long(), nb)
            del ws, cur, nxt
            torch.cuda.empty_cache()
        note("node_partition(k=3), quotient, build_graph_plans")
        for d in DIRECTIONS:
            rec[f"partition_k3_{d}_ms"] = timed(lambda: S.node_partition(ei, et, n, r, k=3, direction=d), args.repeats)[0]
        b, nb = blocks["out"]
        q = {}
        rec["quotient_dedup_ms"] = timed(lambda: q.__setitem__("q", S.quotient_graph(ei, et, b, nb)), args.repeats)[0]
        rec["quotient_edges"] = int(q["q"][1].shape[0])
        del q
        rec["build_graph_plans_ms"] = timed(lambda: build_graph_plans(ei, et, n, r, 256), args.repeats)[0]
        torch.cuda.empty_cache()
        if not args.no_torch:
            gen = torch.Generator(device=dev).manual_seed(0)
            words = lambda m: torch.randint(-2 ** 62, 2 ** 62, (m, 2), dtype=torch.int64, device=dev, generator=gen)
            for d in DIRECTIONS:
                def three():
                    blk, nbt = torch.zeros(n, dtype=torch.int64, device=dev), 1
                    for _ in range(3):
                        blk, nbt = torch_round(ei, et, blk, n, d, words)
                    three.out = (blk, nbt)
                note(f"torch.unique baseline, {d}")
                try:
                    rec[f"torch_unique_k3_{d}_ms"] = timed(three, args.torch_repeats)[0]
                    rec[f"torch_unique_k3_{d}_same_partition"] = bool(three.out[1] == blocks[d][1] and torch.equal(three.out[0], blocks[d][0]))
                    rec[f"speedup_k3_{d}"] = round(rec[f"torch_unique_k3_{d}_ms"][0] / rec[f"partition_k3_{d}_ms"][0], 2)
                except torch.cuda.OutOfMemoryError as err:
                    rec[f"torch_unique_k3_{d}_ms"] = f"out of memory: {str(err)[:80]}"
                torch.cuda.empty_cache()
        print(json.dumps(rec), flush=True)
        del ei, et, keep, blocks
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
