#!/usr/bin/env python3
"""Link prediction (scaling_rgcn_training_amd/linkpred.py, csrc/rgcn_linkpred.hip) against its torch formulation, on one
MI355X, in one process, on 1M nodes / 10M edges / 32 relations at dim 64.  Wall-clock medians after two warm-ups, host clock around
calls that end in a synchronise (tools/minibatch_timing.py's method).
  * ``score_backward``: DistMult forward + backward under autograd at T = 2M triples (score, index build, backward; the three parts
    also alone), against ``(z[s] * rel[r] * z[o]).sum(-1)`` and its autograd backward (``index_add_`` with float atomics);
  * ``corrupt``: 2M negatives, against ``torch.randint`` + ``torch.where``;
  * ``ranks``: filtered ranks of 10,000 queries over all 1M entities (``FilterIndex.lists`` included on both sides), against chunks of
    256 queries x 1M scores by ``matmul``, the filter scattered as -inf, compared and summed; the counts are compared too;
  * ``train_step``: one step of ``Trainer.train_link_prediction``'s loop (full-graph encode, 1M positives + 1M negatives, loss,
    backward, Adam) with the HIP decoder and negatives, against the same step with the torch decoder and negatives.
    python tools/linkpred_timing.py [--steps 10] [--out profiles/linkpred_timing.txt]
Writes one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NODES, EDGES, RELATIONS, DIM, TRIPLES, QUERIES, CHUNK = 1_000_000, 10_000_000, 32, 64, 2_000_000, 10_000, 256


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


def torch_score(z, rel, s, r, o):
    return (z[s] * rel[r] * z[o]).sum(-1)


def torch_corrupt(s, r, o, num_nodes, gen):
    ids = torch.randint(0, num_nodes, s.shape, device=s.device, generator=gen)
    side = torch.randint(0, 2, s.shape, device=s.device, generator=gen).bool()
    return torch.where(side, s, ids), r, torch.where(side, ids, o)


def torch_ranks(z, rel, s, r, o, filt):
    """object-side filtered (greater, equal), CHUNK queries x N scores at a time"""
    ptr, idx = filt.lists(s, r, o, "object")
    greater, equal = [], []
    for c0 in range(0, s.shape[0], CHUNK):
        c1 = min(c0 + CHUNK, s.shape[0])
        scores = (z[s[c0:c1]] * rel[r[c0:c1]]) @ z.t()
        rows = torch.arange(c1 - c0, device=z.device)
        t = scores[rows, o[c0:c1]].unsqueeze(1)
        lens = ptr[c0 + 1:c1 + 1] - ptr[c0:c1]
        scores[torch.repeat_interleave(rows, lens), idx[int(ptr[c0]):int(ptr[c1])]] = float("-inf")
        scores[rows, o[c0:c1]] = float("-inf")
        greater.append((scores > t).sum(1))
        equal.append((scores == t).sum(1))
    return torch.cat(greater), torch.cat(equal)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linkpred_timing.txt"))
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from oracle import rgcn_oracle as O
    from scaling_rgcn_training_amd import _lib
    from scaling_rgcn_training_amd.data import Data
    from scaling_rgcn_training_amd.layers import Emb_Layers
    from scaling_rgcn_training_amd.linkpred import DistMult, FilterIndex, corrupt, ranks
    from scaling_rgcn_training_amd.trainer import do_nothing
    assert torch.cuda.is_available(), "the timing needs the MI355X"
    dev = torch.device("cuda:0")
    steps = args.steps
    gen = torch.Generator(device=dev).manual_seed(0)
    shape = {"nodes": NODES, "edges": EDGES, "relations": RELATIONS, "dim": DIM}
    lines = [json.dumps({"steps": steps, "method": "host clock around calls that end in a synchronise, median after two warm-ups",
                         "device": torch.cuda.get_device_name(0), **shape})]

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    z = torch.randn(NODES, DIM, device=dev, generator=gen)
    dec = DistMult(RELATIONS, DIM).to(dev)
    s, o = (torch.randint(0, NODES, (TRIPLES,), device=dev, generator=gen) for _ in range(2))
    r = torch.randint(0, RELATIONS, (TRIPLES,), device=dev, generator=gen)
    gout = torch.randn(TRIPLES, device=dev, generator=gen)

    # ---- (i) score + backward
    zg = z.clone().requires_grad_(True)

    def ours_fb():
        zg.grad = dec.rel.grad = None
        dec(zg, s, r, o).backward(gout)

    def torch_fb():
        zg.grad = dec.rel.grad = None
        torch_score(zg, dec.rel, s, r, o).backward(gout)

    rec = {"case": "score_backward", "triples": TRIPLES, "hip_ms": wall_ms(ours_fb, steps)}
    ours_grads = (zg.grad.clone(), dec.rel.grad.clone())
    rec["torch_ms"] = wall_ms(torch_fb, steps)
    rec["torch_over_hip"] = round(rec["torch_ms"] / rec["hip_ms"], 2)
    rec["max_abs_diff_dz"] = float((zg.grad - ours_grads[0]).abs().max())
    rec["max_abs_diff_drel_over_max"] = float((dec.rel.grad - ours_grads[1]).abs().max() / dec.rel.grad.abs().max())
    rel = dec.rel.detach()
    rec["hip_score_ms"] = wall_ms(lambda: _lib.lp_score(z, rel, s, r, o), steps)
    rec["hip_index_build_ms"] = wall_ms(lambda: _lib.lp_index_build(s, r, o, NODES, RELATIONS), steps)
    ix = _lib.lp_index_build(s, r, o, NODES, RELATIONS)
    rec["hip_backward_ms"] = wall_ms(lambda: _lib.lp_backward(z, rel, s, r, o, gout, ix), steps)
    rec["torch_score_ms"] = wall_ms(lambda: torch_score(z, rel, s, r, o), steps)
    emit(rec)
    del zg, ours_grads, ix

    # ---- (ii) negatives
    rec = {"case": "corrupt", "triples": TRIPLES, "negatives_per_triple": 1,
           "hip_ms": wall_ms(lambda: corrupt(s, r, o, NODES, 1, 7), steps),
           "torch_ms": wall_ms(lambda: torch_corrupt(s, r, o, NODES, gen), steps)}
    rec["torch_over_hip"] = round(rec["torch_ms"] / rec["hip_ms"], 2)
    emit(rec)

    # ---- (iii) filtered ranks
    known = torch.stack([s, r, o], 1)
    t0 = time.perf_counter()
    filt = FilterIndex(known, NODES, RELATIONS)
    torch.cuda.synchronize()
    build_ms = round((time.perf_counter() - t0) * 1e3, 1)
    qs, qr, qo = s[:QUERIES].contiguous(), r[:QUERIES].contiguous(), o[:QUERIES].contiguous()
    rank_steps = max(3, steps // 2)
    rec = {"case": "ranks", "queries": QUERIES, "entities": NODES, "side": "object", "known_triples": TRIPLES,
           "filter_index_build_ms_once": build_ms, "torch_chunk_queries": CHUNK,
           "hip_ms": wall_ms(lambda: ranks(z, dec, qs, qr, qo, "object", filt), rank_steps),
           "hip_raw_ms": wall_ms(lambda: ranks(z, dec, qs, qr, qo, "object", None), rank_steps),
           "torch_ms": wall_ms(lambda: torch_ranks(z, rel, qs, qr, qo, filt), rank_steps)}
    rec["torch_over_hip"] = round(rec["torch_ms"] / rec["hip_ms"], 2)
    g_h, e_h = ranks(z, dec, qs, qr, qo, "object", filt)
    g_t, e_t = torch_ranks(z, rel, qs, qr, qo, filt)
    rec["queries_with_another_greater_count_than_torch"] = int((g_h != g_t).sum())
    rec["max_abs_diff_greater"] = int((g_h - g_t).abs().max())
    rec["pair_gflop"] = round(2 * QUERIES * NODES * DIM / 1e9, 1)
    rec["hip_raw_tflops_fp32"] = round(2 * QUERIES * NODES * DIM / (rec["hip_raw_ms"] * 1e-3) / 1e12, 2)
    emit(rec)
    del filt, known, g_h, g_t, e_h, e_t

    # ---- (iv) one training step
    ei, et = O.synthetic_graph(NODES, EDGES, RELATIONS, seed=0)
    data = Data(edge_index=ei.to(dev), edge_type=et.to(dev))
    pos = torch.stack([data.edge_index[0, :TRIPLES // 2], data.edge_type[:TRIPLES // 2], data.edge_index[1, :TRIPLES // 2]], 1)
    ps, pr, po = (pos[:, c].contiguous() for c in range(3))
    labels = torch.cat([torch.ones(ps.shape[0], device=dev), torch.zeros(ps.shape[0], device=dev)])
    rec = {"case": "train_step", "positives": int(ps.shape[0]), "negatives": int(ps.shape[0]), "encoder": f"Emb_Layers {DIM}->{DIM}->{DIM}"}
    for name in ("hip", "torch"):
        torch.manual_seed(0)
        model = Emb_Layers(RELATIONS, DIM, DIM, NODES, DIM).to(dev)
        decoder = DistMult(RELATIONS, DIM).to(dev)
        opt = torch.optim.Adam(list(model.parameters()) + list(decoder.parameters()), lr=0.01)
        count = [0]

        def step():
            opt.zero_grad()
            zz = model(data, do_nothing)
            count[0] += 1
            if name == "hip":
                sn, rn, on = corrupt(ps, pr, po, NODES, 1, count[0])
                scores = decoder(zz, torch.cat([ps, sn]), torch.cat([pr, rn]), torch.cat([po, on]))
            else:
                sn, rn, on = torch_corrupt(ps, pr, po, NODES, gen)
                scores = torch_score(zz, decoder.rel, torch.cat([ps, sn]), torch.cat([pr, rn]), torch.cat([po, on]))
            loss = torch.nn.functional.binary_cross_entropy_with_logits(scores, labels)
            loss = loss + 0.01 * (zz.pow(2).mean() + decoder.rel.pow(2).mean())
            loss.backward()
            opt.step()

        def encode_only():
            opt.zero_grad()
            model(data, do_nothing).pow(2).mean().backward()

        rec[f"{name}_ms"] = wall_ms(step, steps)
        if name == "hip":
            rec["encoder_forward_backward_alone_ms"] = wall_ms(encode_only, steps)
            decoder.check()
        del model, decoder, opt
        torch.cuda.empty_cache()
    rec["torch_over_hip"] = round(rec["torch_ms"] / rec["hip_ms"], 2)
    emit(rec)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
