"""fp64 reference of the bipartite RGCNConv (``x = (x_src, x_dst)``), composed from the frozen oracle (oracle/rgcn_oracle.py), for
tests/test_bipartite_host.py and tests/test_gpu_bipartite.py.  No tests here.

On the square graph of N = max(N_src, N_dst) nodes, with x_src and the output gradient g zero padded to N rows and no root:
``rgcn_conv_dense(...)[:N_dst] + x_dst @ root`` is the output, ``rgcn_conv_grads_dense(...)["x"][:N_src]`` is dX_src, ``["weight"]``
is d_W; ``x_dst^T g``, ``g root^T`` and the column sums of g are the rest.  The condition sums are the same expressions on absolute
values; the fp32 CPU comparison is ``cpu32_reference`` plus torch fp32 matmuls for the root terms.  ``pyg_bipartite_loop`` restates
PyG 2.3.1's loop directly (autograd does its backward): tests/test_bipartite_host.py checks the composition against it."""
import numpy as np
import torch

from oracle import rgcn_oracle as O
from oracle.tolerance import abs_condition, cpu32_reference


def bipartite_graph(n_src, n_dst, r, seed, e=2500, hub=600, dup=50):
    """``e`` random edges into the destinations before the last 5 (those stay isolated), relation r - 1 without edges, ``hub`` more
    edges into destination 0 (relation 0), the first ``dup`` triples repeated.  One-row sides: every edge touches row 0."""
    g = torch.Generator().manual_seed(seed)
    m = max(n_dst - 5, 1)
    src = torch.cat([torch.randint(0, n_src, (e,), generator=g), torch.randint(0, n_src, (hub,), generator=g)])
    dst = torch.cat([torch.randint(0, m, (e,), generator=g), torch.zeros(hub, dtype=torch.int64)])
    typ = torch.cat([torch.randint(0, max(r - 1, 1), (e,), generator=g), torch.zeros(hub, dtype=torch.int64)])
    src, dst, typ = torch.cat([src, src[:dup]]), torch.cat([dst, dst[:dup]]), torch.cat([typ, typ[:dup]])
    return torch.stack([src, dst]), typ


def _pad(a, n):
    a = np.asarray(a, dtype=np.float64)
    return a if a.shape[0] == n else np.concatenate([a, np.zeros((n - a.shape[0], a.shape[1]))], 0)


def reference(x_src, x_dst, ei, et, w_full, root, bias, g, aggr="mean"):
    """(ref, cond, cpu32): dicts with "out", "x_src", "x_dst", "weight", "root", "bias" (root / x_dst / bias only where the layer has
    them).  ``w_full``: dense [R, in_src, out]; everything numpy / torch on the CPU."""
    f64 = lambda t: None if t is None else np.asarray(t, dtype=np.float64)
    x_src, x_dst, w_full, root, bias, g = (f64(t) for t in (x_src, x_dst, w_full, root, bias, g))
    ei, et = np.asarray(ei), np.asarray(et)
    n_src, n_dst = x_src.shape[0], x_dst.shape[0]
    n = max(n_src, n_dst)

    def compose(xs, xd, w, rt, bs, gg, out, grads, mm):
        res = {"out": out[:n_dst], "x_src": grads["x"][:n_src], "weight": grads["weight"]}
        if bs is not None:
            res["bias"] = grads["bias"]
        if rt is not None:
            res["out"] = res["out"] + mm(xd, rt)
            res["root"] = mm(xd.T, gg)
            res["x_dst"] = mm(gg, rt.T)
        return res

    xs, gp = _pad(x_src, n), _pad(g, n)
    ref = compose(xs, x_dst, w_full, root, bias, g, O.rgcn_conv_dense(xs, ei, et, w_full, None, bias, aggr=aggr),
                  O.rgcn_conv_grads_dense(xs, ei, et, w_full, None, gp, aggr=aggr), np.matmul)
    a = lambda t: None if t is None else np.abs(t)
    c_out, c_g = abs_condition(xs, ei, et, w_full, None, bias, gp, aggr=aggr)
    cond = compose(a(xs), a(x_dst), a(w_full), a(root), a(bias), a(g), c_out, c_g, np.matmul)
    o32, g32 = cpu32_reference(xs, ei, et, w_full, None, bias, gp, aggr=aggr)
    t32 = lambda t: torch.as_tensor(np.ascontiguousarray(t), dtype=torch.float32)
    mm32 = lambda p, q: (t32(p) @ t32(q)).numpy()
    cpu32 = compose(xs, x_dst, w_full, root, bias, g, o32, g32, mm32)
    cpu32["out"] = np.asarray(cpu32["out"], dtype=np.float32)      # (fp32 sum of the two fp32 parts)
    return ref, cond, cpu32


def pyg_bipartite_loop(x_src, x_dst, edge_index, edge_type, weight, root, bias, aggr="mean"):
    """PyG 2.3.1 ``RGCNConv.forward`` with ``x = (x_l, x_r)``, no pyg_lib: per relation, aggregate x_l over the edges into each
    destination (mean: divided by max(1, count), duplicates counted), times W_r; ``+ x_r @ root + bias``.  Differentiable torch."""
    n_dst = x_dst.shape[0]
    out = torch.zeros(n_dst, weight.shape[2], dtype=x_src.dtype)
    for r in range(weight.shape[0]):
        sel = edge_type == r
        if not bool(sel.any()):
            continue
        src, dst = edge_index[0][sel], edge_index[1][sel]
        h = torch.zeros(n_dst, x_src.shape[1], dtype=x_src.dtype).index_add_(0, dst, x_src[src])
        if aggr == "mean":
            cnt = torch.zeros(n_dst, dtype=x_src.dtype).index_add_(0, dst, torch.ones(dst.shape[0], dtype=x_src.dtype))
            h = h / cnt.clamp(min=1)[:, None]
        out = out + h @ weight[r]
    if root is not None:
        out = out + x_dst @ root
    if bias is not None:
        out = out + bias
    return out
