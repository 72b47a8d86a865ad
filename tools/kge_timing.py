#!/usr/bin/env python3
"""The ComplEx and TransE decoders (scaling_rgcn_training_amd/linkpred.py, csrc/rgcn_kge.hip) against their torch
formulations, on one MI355X, in one process, at 1M nodes / 32 relations / dim 64, in the manner of tools/linkpred_timing.py: wall-clock
medians after two warm-ups, host clock around calls that end in a synchronise.  Per decoder:
  * ``score_backward``: forward + backward under autograd at T = 2M triples (score, index build, backward; the three parts also
    alone), against the torch score (``view_as_complex`` products / ``-(s + r - o).abs().sum(-1)``) and its autograd backward;
  * ``ranks``: object-side filtered ranks of 10,000 queries over all 1M entities, against chunks of 256 queries x 1M scores (a
    ``matmul`` on the complex query image / ``(q[:, None] - z[None]).abs().sum(-1)`` on 16 queries at a time, 4 GB of differences;
    ``torch.cdist(p=1)`` gave wrong distances at [256, 1M] on the timing machine and is not used), the filter scattered as -inf; the
    counts are compared too.
    python tools/kge_timing.py [--steps 10] [--out profiles/kge_timing.txt]
Writes one JSON line per measurement."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from linkpred_timing import CHUNK, DIM, NODES, QUERIES, RELATIONS, TRIPLES, wall_ms  # noqa: E402


def _cx(t):
    return torch.view_as_complex(t.reshape(t.shape[0], -1, 2))


def torch_score(name, z, rel, s, r, o):
    if name == "transe":
        return -(z[s] + rel[r] - z[o]).abs().sum(-1)
    return (_cx(z)[s] * _cx(rel)[r] * _cx(z)[o].conj()).real.sum(-1)


def torch_chunk_scores(name, z, rel, s, r):
    """[chunk, N] object-side scores"""
    if name == "transe":
        q = z[s] + rel[r]
        return torch.cat([-(q[i:i + 16, None, :] - z[None]).abs().sum(-1) for i in range(0, q.shape[0], 16)])
    return torch.view_as_real(_cx(z)[s] * _cx(rel)[r]).reshape(s.shape[0], -1) @ z.t()


def torch_ranks(name, z, rel, s, r, o, filt):
    ptr, idx = filt.lists(s, r, o, "object")
    greater, equal = [], []
    for c0 in range(0, s.shape[0], CHUNK):
        c1 = min(c0 + CHUNK, s.shape[0])
        scores = torch_chunk_scores(name, z, rel, s[c0:c1], r[c0:c1])
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kge_timing.txt"))
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from scaling_rgcn_training_amd import _lib
    from scaling_rgcn_training_amd.linkpred import ComplEx, FilterIndex, TransE, ranks
    assert torch.cuda.is_available(), "the timing needs the MI355X"
    dev, steps = torch.device("cuda:0"), args.steps
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [json.dumps({"steps": steps, "method": "host clock around calls that end in a synchronise, median after two warm-ups",
                         "device": torch.cuda.get_device_name(0), "nodes": NODES, "relations": RELATIONS, "dim": DIM})]

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    z = torch.randn(NODES, DIM, device=dev, generator=gen)
    s, o = (torch.randint(0, NODES, (TRIPLES,), device=dev, generator=gen) for _ in range(2))
    r = torch.randint(0, RELATIONS, (TRIPLES,), device=dev, generator=gen)
    gout = torch.randn(TRIPLES, device=dev, generator=gen)
    filt = FilterIndex(torch.stack([s, r, o], 1), NODES, RELATIONS)
    qs, qr, qo = s[:QUERIES].contiguous(), r[:QUERIES].contiguous(), o[:QUERIES].contiguous()
    rank_steps = max(3, steps // 2)
    for name, cls in (("complex", ComplEx), ("transe", TransE)):
        dec = cls(RELATIONS, DIM).to(dev)
        rel, zg = dec.rel.detach(), z.clone().requires_grad_(True)

        def ours_fb():
            zg.grad = dec.rel.grad = None
            dec(zg, s, r, o).backward(gout)

        def torch_fb():
            zg.grad = dec.rel.grad = None
            torch_score(name, zg, dec.rel, s, r, o).backward(gout)

        rec = {"case": "score_backward", "decoder": name, "triples": TRIPLES, "hip_ms": wall_ms(ours_fb, steps)}
        ours = (zg.grad.clone(), dec.rel.grad.clone())
        rec["torch_ms"] = wall_ms(torch_fb, steps)
        rec["torch_over_hip"] = round(rec["torch_ms"] / rec["hip_ms"], 2)
        rec["max_abs_diff_dz"] = float((zg.grad - ours[0]).abs().max())
        rec["max_abs_diff_drel_over_max"] = float((dec.rel.grad - ours[1]).abs().max() / dec.rel.grad.abs().max())
        rec["hip_score_ms"] = wall_ms(lambda: _lib.kge_score(dec.code, z, rel, s, r, o), steps)
        ix = _lib.lp_index_build(s, r, o, NODES, RELATIONS)
        rec["hip_index_build_ms"] = wall_ms(lambda: _lib.lp_index_build(s, r, o, NODES, RELATIONS), steps)
        rec["hip_backward_ms"] = wall_ms(lambda: _lib.kge_backward(dec.code, z, rel, s, r, o, gout, ix), steps)
        rec["torch_score_ms"] = wall_ms(lambda: torch_score(name, z, rel, s, r, o), steps)
        emit(rec)
        del zg, ours, ix

        rec = {"case": "ranks", "decoder": name, "queries": QUERIES, "entities": NODES, "side": "object", "known_triples": TRIPLES,
               "torch_chunk_queries": CHUNK,
               "hip_ms": wall_ms(lambda: ranks(z, dec, qs, qr, qo, "object", filt), rank_steps),
               "hip_raw_ms": wall_ms(lambda: ranks(z, dec, qs, qr, qo, "object", None), rank_steps),
               "hip_raw_subject_ms": wall_ms(lambda: ranks(z, dec, qs, qr, qo, "subject", None), rank_steps),
               "torch_ms": wall_ms(lambda: torch_ranks(name, z, rel, qs, qr, qo, filt), rank_steps)}
        rec["torch_over_hip"] = round(rec["torch_ms"] / rec["hip_ms"], 2)
        g_h, _ = ranks(z, dec, qs, qr, qo, "object", filt)
        g_t, _ = torch_ranks(name, z, rel, qs, qr, qo, filt)
        rec["queries_with_another_greater_count_than_torch"] = int((g_h != g_t).sum())
        rec["max_abs_diff_greater"] = int((g_h - g_t).abs().max())
        pair_columns = QUERIES * NODES * DIM
        if name == "transe":       # two VALU lane-ops per pair-column: the bound DESIGN.md 22 sets the sweep against
            rec["valu_lane_ops_e12"] = round(2 * pair_columns / 1e12, 3)
            rec["hip_raw_lane_tops"] = round(2 * pair_columns / (rec["hip_raw_ms"] * 1e-3) / 1e12, 2)
        else:
            rec["hip_raw_tflops_fp32"] = round(2 * pair_columns / (rec["hip_raw_ms"] * 1e-3) / 1e12, 2)
        emit(rec)
        dec.check()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
