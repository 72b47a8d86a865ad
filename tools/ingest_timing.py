#!/usr/bin/env python3
"""N-Triples ingest on the GPU (scaling_rgcn_training_amd/ingest.py, csrc/rgcn_ingest.hip) against the host loader
``graphs.Graph.init_graph`` on the same file, on one MI355X, in one process, on a synthetic file of 1M triples (200,000 nodes, 40
predicates, AIFB-length IRIs behind a common 45-byte prefix, 10 % literals, 2 % type triples) and on one of 100,000 triples.
Wall-clock medians after two warm-ups, host clock around calls that end in a synchronise (tools/minibatch_timing.py's method).
  * ``load_nt``: end to end from the path (file read, one host -> device copy, four ABI calls, the tables' read-back);
  * per phase, on bytes already on the device: ``read_file`` (numpy.fromfile, page cache warm), ``upload`` (the bare host -> device
    copy: the floor), ``tokenize`` (rgcn_nt_lines + rgcn_nt_tokenize), ``build`` (rgcn_nt_build: hash, sort, verify, rank rounds,
    roles), ``emit`` (rgcn_nt_emit + the read-back of the three tables);
  * ``host_loader``: ``graphs.parse_graph_nt`` + ``Graph.init_graph`` on the same file (CPU time of this host; ``--host-steps`` runs);
    its edge tensors are compared with ``load_nt``'s, exactly.
    python tools/ingest_timing.py [--steps 5] [--host-steps 1] [--sizes 1000000,100000] [--out profiles/ingest_timing.txt]
Writes one JSON line per measurement."""
import argparse
import json
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PREFIX = "<http://www.aifb.uni-karlsruhe.de/Publikationen/"        # 45 bytes + the '<'
RDF_TYPE = "<http://www.w3.org/1999/02/22-rdf-syntax-ns#type>"


def synthetic(path: str, triples: int, seed: int = 0) -> None:
    rng = random.Random(seed)
    nodes = max(2, triples // 5)
    ids = [f"{PREFIX}viewPublikationOWL/id{i}instance>" for i in range(nodes)]
    preds = [f"<http://swrc.ontoware.org/ontology#predicate{k}>" for k in range(40)]
    classes = [f"<http://swrc.ontoware.org/ontology#Class{k}>" for k in range(8)]
    with open(path, "w") as f:
        for _ in range(triples):
            r = rng.random()
            s = ids[rng.randrange(nodes)]
            if r < 0.02:
                f.write(f"{s} {RDF_TYPE} {classes[rng.randrange(8)]} .\n")
            elif r < 0.12:
                f.write(f'{s} {preds[rng.randrange(40)]} "literal value number {rng.randrange(triples)} of the file" .\n')
            else:
                f.write(f"{s} {preds[rng.randrange(40)]} {ids[rng.randrange(nodes)]} .\n")


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
    return round(ts[len(ts) // 2], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=1)
    ap.add_argument("--sizes", default="1000000,100000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_timing.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ingest_timing needs the GPU: nothing here is measured on a CPU")
    import __graft_entry__ as entry
    entry.build()
    from scaling_rgcn_training_amd import graphs as G
    from scaling_rgcn_training_amd import ingest

    rows = [{"what": "header", "device": torch.cuda.get_device_name(0), "steps": args.steps, "host_steps": args.host_steps,
             "method": "wall-clock median after 2 warm-ups, synchronise inside the window"}]
    with tempfile.TemporaryDirectory() as tmp:
        for triples in (int(v) for v in args.sizes.split(",")):
            path = os.path.join(tmp, f"synthetic_{triples}.nt")
            synthetic(path, triples)
            size = os.path.getsize(path)
            host = np.fromfile(path, dtype=np.uint8)
            text = torch.from_numpy(host).cuda()
            occ_off, occ_len, t, max_len = ingest.tokenize(text)
            bits = ingest._hash_bits(3 * t)
            st, counts, ws = ingest.build(text, occ_off, occ_len, t, max_len, bits, 0)
            assert st == 0, st
            g = ingest.load_nt(path)
            shape = {"triples": t, "bytes": size, "distinct_terms": int(counts[0]), "nodes": g.num_nodes, "relations": g.num_relations // 2,
                     "classes": len(g.classes), "edges": int(g.edge_type.shape[0]), "labelled": int(g.labelled_idx.shape[0]),
                     "max_term_len": max_len, "hash_bits": bits, "rank_rounds": int(counts[7])}
            rows.append({"what": "shape", **shape})
            ms = {
                "load_nt": wall_ms(lambda: ingest.load_nt(path), args.steps),
                "read_file": wall_ms(lambda: np.fromfile(path, dtype=np.uint8), args.steps),
                "upload": wall_ms(lambda: torch.from_numpy(host).cuda(), args.steps),
                "tokenize": wall_ms(lambda: ingest.tokenize(text), args.steps),
                "build": wall_ms(lambda: ingest.build(text, occ_off, occ_len, t, max_len, bits, 0), args.steps),
                "build_64_bits": wall_ms(lambda: ingest.build(text, occ_off, occ_len, t, max_len, 64, 0), args.steps),
                "emit": wall_ms(lambda: ingest.emit(text, t, counts, ws), args.steps),
            }
            for k, v in ms.items():
                rows.append({"what": k, "triples": t, "ms": v})

            def host_loader():
                hg = G.Graph("host")
                hg.init_graph(G.parse_graph_nt(path))
                return hg

            ts = []
            for _ in range(args.host_steps):
                t0 = time.perf_counter()
                hg = host_loader()
                ts.append((time.perf_counter() - t0) * 1e3)
            ts.sort()
            same = bool(torch.equal(hg.training_data.edge_index, g.edge_index.cpu()) and torch.equal(hg.training_data.edge_type, g.edge_type.cpu())
                        and hg.num_nodes == g.num_nodes)
            rows.append({"what": "host_loader", "triples": t, "ms": round(ts[len(ts) // 2], 1), "same_edges_as_load_nt": same})
            rows.append({"what": "ratio", "triples": t, "host_loader_over_load_nt": round(ts[len(ts) // 2] / ms["load_nt"], 1),
                         "load_nt_over_upload": round(ms["load_nt"] / ms["upload"], 1)})
            del g, hg, text, ws
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
