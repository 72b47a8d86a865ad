#!/usr/bin/env python3
"""The summary -> original pipeline on tensors (scaling_rgcn_training_amd/transfer.py, tensor_data.py, csrc/rgcn_transfer.hip,
DESIGN.md 19) against its torch formulation, on one MI355X, in one process, at 1M nodes / 10M edges and 10M nodes / 100M edges
with 3 summaries of 50,000 blocks, 64 columns, 100,000 labelled nodes (60 % of them training nodes) of 8 classes, 30 % of the
nodes unmapped.  Wall-clock medians after two warm-ups, host clock around calls that end in a synchronise
(tools/minibatch_timing.py's method).
  * ``summary_labels``: against ``bincount`` + ``index_add_`` + the double quotient + ``nonzero``, on a random partition of 50,000
    blocks and on the one-block partition (every node one id: what the wave-level combining is for); results compared exactly;
  * ``materialize`` per mode: against ``rand`` + ``index_select`` + masked assignment per summary, then ``stack`` / ``cat`` / sum;
  * ``rows``: 100,000 nodes, against indexing the materialised tensor (which has to exist first);
  * ``add_summary``: ``TensorDataset.add_summary`` end to end (k = 1 partition, quotient graph, labels), and with a given partition;
  * ``string_path`` (1M only, once): ``graphs.summary_graph`` + ``Dataset.make_training_data`` + ``graphs.stack_embeddings`` of one
    summary on the same graph given node names -- the per-node Python the tensor path replaces (CPU time of this host).
    python tools/transfer_timing.py [--steps 10] [--sizes 1000000,10000000] [--cases labels,gather,add_summary,string_path]
                                    [--append --note TEXT] [--out profiles/transfer_timing.txt]
Writes one JSON line per measurement.  ``--append`` adds a run to the file instead of replacing it, ``--note`` labels the run's
header line: with ``RGCN_LIB`` pointing at an experiment build of the library (its path is recorded) that is an A/B in one file."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SUMMARIES, DIM, BLOCKS, LABELLED, CLASSES, RELATIONS, ROWS = 3, 64, 50_000, 100_000, 8, 16, 100_000


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


def torch_labels(block, num_blocks, train_idx, y):
    size = torch.bincount(block, minlength=num_blocks)
    cnt = torch.zeros(num_blocks, y.shape[1], dtype=torch.int64, device=block.device).index_add_(0, block[train_idx], y)
    y_sum = (cnt.double() / size.clamp(min=1).double()[:, None]).float()
    x = torch.nonzero(cnt.sum(1) != 0).flatten()
    return x, y_sum[x], size


def torch_gather(tables, maps, n, mode):
    pieces = []
    for t, m in zip(tables, maps):
        p = torch.rand(n, t.shape[1], device=t.device)
        keep = m >= 0
        p[keep] = t.index_select(0, m[keep])
        pieces.append(p)
    if mode == "stack":
        return torch.stack(pieces)
    if mode == "concat":
        return torch.cat(pieces, dim=-1)
    return sum(pieces)


def string_path(ei, et, n, labelled, labels, block, num_blocks, emb):
    """seconds of the string-keyed path for one summary: names, summary_graph, make_training_data, stack_embeddings"""
    from scaling_rgcn_training_amd import graphs as G
    from scaling_rgcn_training_amd.data import Data
    from scaling_rgcn_training_amd.summaries import Partition
    out = {}
    t0 = time.perf_counter()
    names = [f"<n{i:08d}>" for i in range(n)]
    graph = G.Graph("named", {names[i]: {f"<c{c}>" for c in torch.nonzero(row).flatten().tolist()}
                              for i, row in zip(labelled.tolist(), labels)})
    graph.nodes, graph.node_to_enum, graph.num_nodes, graph.num_edges = names, {nm: i for i, nm in enumerate(names)}, n, int(et.shape[0])
    graph.relations = {f"<p{p}>": p for p in range(RELATIONS // 2)}
    graph.training_data = Data(edge_index=ei)
    graph.training_data.edge_type = et
    ds = G.Dataset(None)
    ds.orgGraph, ds.enum_classes, ds.num_classes = graph, {f"<c{c}>": c for c in range(CLASSES)}, CLASSES
    out["names_and_dicts_s"] = round(time.perf_counter() - t0, 2)
    t0 = time.perf_counter()
    sg = G.summary_graph(graph, Partition(block, num_blocks, 1, (num_blocks,), False), "summary")
    out["summary_graph_s"] = round(time.perf_counter() - t0, 2)
    ds.sumGraphs = [sg]
    t0 = time.perf_counter()
    ds.make_training_data()
    out["make_training_data_s"] = round(time.perf_counter() - t0, 2)
    sg.embedding = emb
    t0 = time.perf_counter()
    G.stack_embeddings(graph, ds.sumGraphs, DIM)
    out["stack_embeddings_s"] = round(time.perf_counter() - t0, 2)
    out["per_summary_s"] = round(out["summary_graph_s"] + out["make_training_data_s"] + out["stack_embeddings_s"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--cases", default="labels,gather,add_summary,string_path")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--note", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transfer_timing.txt"))
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from scaling_rgcn_training_amd import transfer as T
    from scaling_rgcn_training_amd.summaries import Partition
    from scaling_rgcn_training_amd.tensor_data import TensorDataset
    assert torch.cuda.is_available(), "the timing needs the MI355X"
    dev = torch.device("cuda:0")
    steps = args.steps
    lines = [json.dumps({"steps": steps, "method": "host clock around calls that end in a synchronise, median after two warm-ups",
                         "device": torch.cuda.get_device_name(0), "summaries": SUMMARIES, "dim": DIM, "blocks": BLOCKS,
                         "labelled": LABELLED, "classes": CLASSES, "unmapped": 0.3,
                         **({"note": args.note} if args.note else {}),
                         **({"library": os.path.basename(os.environ["RGCN_LIB"])} if os.environ.get("RGCN_LIB") else {})})]
    cases = set(args.cases.split(","))

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for n in (int(v) for v in args.sizes.split(",")):
        gen = torch.Generator(device=dev).manual_seed(0)
        edges = 10 * n
        shape = {"nodes": n, "edges": edges}
        ei = torch.randint(0, n, (2, edges), device=dev, generator=gen)
        et = torch.randint(0, RELATIONS, (edges,), device=dev, generator=gen)
        labelled = torch.randperm(n, device=dev, generator=gen)[:LABELLED]
        labels = torch.nn.functional.one_hot(torch.randint(0, CLASSES, (LABELLED,), device=dev, generator=gen), CLASSES)
        data = TensorDataset(ei, et, n, RELATIONS, labelled, labels)
        td = data.orgGraph.training_data
        block = torch.randint(0, BLOCKS, (n,), device=dev, generator=gen)
        one = torch.zeros(n, dtype=torch.int64, device=dev)

        # ---- (i) labels
        for name, b, nb in (("random_blocks", block, BLOCKS), ("one_block", one, 1)) if "labels" in cases else ():
            rec = {"case": "summary_labels", "partition": name, **shape, "training_rows": int(td.x_train.shape[0]),
                   "hip_ms": wall_ms(lambda: T.summary_labels(b, nb, td.x_train, td.y_train), steps),
                   "torch_ms": wall_ms(lambda: torch_labels(b, nb, td.x_train, td.y_train), steps)}
            rec["torch_over_hip"] = round(rec["torch_ms"] / rec["hip_ms"], 2)
            ours, theirs = T.summary_labels(b, nb, td.x_train, td.y_train), torch_labels(b, nb, td.x_train, td.y_train)
            rec["equal_to_torch"] = bool(torch.equal(ours[0], theirs[0]) and torch.equal(ours[1], theirs[1])
                                         and torch.equal(ours[2].long(), theirs[2]))
            emit(rec)

        # ---- (ii) the transferred embedding
        tables = [torch.randn(BLOCKS, DIM, device=dev, generator=gen) for _ in range(SUMMARIES)]
        maps = []
        for _ in range(SUMMARIES):
            m = torch.randint(0, BLOCKS, (n,), device=dev, generator=gen)
            m[torch.rand(n, device=dev, generator=gen) < 0.3] = -1
            maps.append(m)
        nodes = torch.randint(0, n, (ROWS,), device=dev, generator=gen)
        for mode in T.MODES if "gather" in cases else ():
            te = T.TransferredEmbedding(tables, maps, n, mode, seed=1)
            out_bytes = n * DIM * 4 * (1 if mode == "sum" else SUMMARIES)
            rec = {"case": "materialize", "mode": mode, **shape, "output_gb": round(out_bytes / 1e9, 3),
                   "hip_ms": wall_ms(te.materialize, steps), "torch_ms": wall_ms(lambda: torch_gather(tables, maps, n, mode), steps)}
            rec["hip_output_gb_per_s"] = round(out_bytes / 1e9 / (rec["hip_ms"] * 1e-3), 1)
            rec["torch_over_hip"] = round(rec["torch_ms"] / rec["hip_ms"], 2)
            full = te.materialize()
            mapped = torch.stack(maps) >= 0
            if mode == "stack":
                want = torch.stack([t[m.clamp(min=0)] for t, m in zip(tables, maps)])
                rec["mapped_rows_equal_index_select"] = bool(torch.equal(full[mapped], want[mapped]))
                del want
            index = (lambda: full[:, nodes]) if mode == "stack" else (lambda: full[nodes])
            rec2 = {"case": "rows", "mode": mode, **shape, "rows": ROWS, "hip_ms": wall_ms(lambda: te.rows(nodes), steps),
                    "torch_index_of_materialized_ms": wall_ms(index, steps)}
            rec2["equal_to_index_of_materialized"] = bool(torch.equal(te.rows(nodes), index()))
            te.check()
            emit(rec)
            emit(rec2)
            del full, mapped
            torch.cuda.empty_cache()

        # ---- (iii) add_summary end to end
        def add(**kw):
            data.add_summary(**kw)
            data.sumGraphs.pop()

        if "add_summary" in cases:
            part = Partition(block, BLOCKS, 1, (BLOCKS,), False)
            few = max(3, steps // 3)
            rec = {"case": "add_summary", **shape, "k1_out_ms": wall_ms(lambda: add(k=1, direction="out"), few),
                   "given_partition_ms": wall_ms(lambda: add(partition=part), few),
                   "given_partition_dedup_ms": wall_ms(lambda: add(partition=part, dedup=True), few)}
            sg = data.add_summary(k=1, direction="out")
            rec["k1_out_blocks"] = sg.num_nodes
            data.sumGraphs.pop()
            emit(rec)

        # ---- (iv) the string-keyed path, once, at the first size only
        if n <= 1_000_000 and "string_path" in cases:
            rec = {"case": "string_path", **shape, "blocks": BLOCKS, "steps": 1}
            rec.update(string_path(ei.cpu(), et.cpu(), n, labelled.cpu(), labels.cpu(), block.cpu(), BLOCKS, tables[0].cpu()))
            emit(rec)
        del ei, et, data, td, tables, maps, block, one
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
