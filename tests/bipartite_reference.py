"""fp64 reference of the bipartite RGCNConv (``x = (x_src, x_dst)``), composed from the frozen oracle (oracle/rgcn_oracle.py), for
tests/test_bipartite_host.py, tests/test_gpu_bipartite.py and tests/test_gpu_bipartite_options.py; ``check``: a layer's tensors
against it under oracle/tolerance.py; ``device_reference``: the same layer by plain torch ops on whatever device its inputs live,
for sizes the numpy oracle cannot hold (tests/test_gpu_bipartite_past_4gib.py).  No tests here.

On the square graph of N = max(N_src, N_dst) nodes, with x_src and the output gradient g zero padded to N rows and no root:
``rgcn_conv_dense(...)[:N_dst] + x_dst @ root`` is the output, ``rgcn_conv_grads_dense(...)["x"][:N_src]`` is dX_src, ``["weight"]``
is d_W; ``x_dst^T g``, ``g root^T`` and the column sums of g are the rest.  The condition sums are the same expressions on absolute
values; the fp32 CPU comparison is ``cpu32_reference`` plus torch fp32 matmuls for the root terms.  ``pyg_bipartite_loop`` restates
PyG 2.3.1's loop directly (autograd does its backward): tests/test_bipartite_host.py checks the composition against it."""
import numpy as np
import torch

from oracle import rgcn_oracle as O
from oracle.tolerance import abs_condition, assert_close, cpu32_reference


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


def check(conv, xs, xd, ei, et, g, got, aggr, tag):
    """every tensor of ``got`` against the fp64 reference of the equivalent dense layer; a decomposition's gradients pushed from the
    dense d_W through ``effective_weight`` by fp64 autograd (their condition: the same on absolute values)"""
    din, dout, r = conv.in_channels, conv.out_channels, conv.num_relations
    w = conv.weight.detach().cpu().double()
    comp = None if conv.comp is None else conv.comp.detach().cpu().double()
    cpu = lambda p: None if p is None else p.detach().cpu()
    wf = O.effective_weight(w, comp, r, conv.num_blocks, din, dout)
    ref, cond, cpu32 = reference(xs.cpu(), xd.cpu(), ei.cpu(), et.cpu(), wf, cpu(conv.root), cpu(conv.bias), g.cpu(), aggr)
    for k in ("out", "x_src", "x_dst", "root", "bias"):
        if got.get(k) is not None:
            assert tuple(got[k].shape) == ref[k].shape, (k, tag)
            assert_close(got[k].numpy(), ref[k], cond[k], f"bipartite {k} {tag}", cpu32=cpu32[k])
    if "weight" not in got and "comp" not in got:
        return ref
    if conv.comp is None and conv.num_blocks is None:
        assert_close(got["weight"].numpy(), ref["weight"], cond["weight"], f"bipartite d_weight {tag}", cpu32=cpu32["weight"])
        return ref

    def push(wv, cv, dw):
        wv = wv.clone().requires_grad_(True)
        cv = None if cv is None else cv.clone().requires_grad_(True)
        full = O.effective_weight(wv, cv, r, conv.num_blocks, din, dout)
        return torch.autograd.grad(full, [t for t in (wv, cv) if t is not None], torch.from_numpy(dw))

    want = push(w, comp, ref["weight"])
    cnd = push(w.abs(), None if comp is None else comp.abs(), np.abs(cond["weight"]))
    if "weight" in got:
        assert_close(got["weight"].numpy(), want[0].numpy(), cnd[0].numpy(), f"bipartite d_weight {tag}")
    if "comp" in got:
        assert_close(got["comp"].numpy(), want[1].numpy(), cnd[1].numpy(), f"bipartite d_comp {tag}")
    return ref


BATCH_ROWS = 4096


def tall_t_matmul(a, b):
    """a^T b of tall matrices a [rows, p], b [rows, q].  float64: one batched product over slices of BATCH_ROWS rows and the sum
    of its results (a single skinny float64 GEMM over 10^7 rows takes the BLAS seconds); any other dtype: the stock product"""
    k = BATCH_ROWS
    if a.dtype != torch.float64 or a.shape[0] < 2 * k:
        return a.t() @ b
    m = a.shape[0] // k
    a, b = a.contiguous(), b.contiguous()
    main = torch.bmm(a[:m * k].view(m, k, -1).transpose(1, 2), b[:m * k].view(m, k, -1)).sum(0)
    return main + a[m * k:].t() @ b[m * k:]


def device_reference(x_src, x_dst, ei, et, weight, root, bias, g, aggr="mean", dtype=torch.float64, absval=False, block=1 << 22):
    """The layer and every gradient by plain torch ops in ``dtype`` on the device of the inputs, nothing shared with the plans:
    per relation H_r = index_add_ of w_e x_src[src_e] into the destinations (mean: w_e = 1 / c[dst, rel], duplicates counted,
    float64), out += H_r @ W_r, d_weight[r] = H_r^T g, d_x_src += index_add_ of w_e (g @ W_r^T)[dst_e] into the sources; the root
    products x_dst @ root, x_dst^T g, g @ root^T in row blocks; d_bias the column sums of g.  ``absval``: the same sums over
    absolute values (the condition of oracle/tolerance.py bound (1)).  ``weight`` dense [R, in_src, out]; root / bias may be None.
    Returns a dict with "out", "x_src", "weight" and, where the layer has them, "x_dst", "root", "bias"."""
    f = (lambda t: t.abs()) if absval else (lambda t: t)
    dev = x_src.device
    n_src, n_dst, r = x_src.shape[0], x_dst.shape[0], weight.shape[0]
    src, dst, et = ei[0].long(), ei[1].long(), et.long()
    if aggr == "mean":
        _, inv, cnt = torch.unique(dst * r + et, return_inverse=True, return_counts=True)
        we = (1.0 / cnt[inv].double()).to(dtype)
    else:
        we = torch.ones(et.shape[0], dtype=dtype, device=dev)
    out = torch.zeros(n_dst, weight.shape[2], dtype=dtype, device=dev)
    dxs = torch.zeros(n_src, weight.shape[1], dtype=dtype, device=dev)
    dw = torch.zeros(weight.shape, dtype=dtype, device=dev)
    for rel in range(r):
        sel = torch.nonzero(et == rel)[:, 0]
        if sel.numel() == 0:
            continue
        s, d, wr = src[sel], dst[sel], f(weight[rel].to(dtype))
        h = torch.zeros(n_dst, weight.shape[1], dtype=dtype, device=dev).index_add_(0, d, f(x_src[s].to(dtype)) * we[sel, None])
        out += h @ wr
        dw[rel] = tall_t_matmul(h, f(g.to(dtype)))
        del h
        dxs.index_add_(0, s, (f(g[d].to(dtype)) @ wr.t()) * we[sel, None])
    res = {"out": out, "x_src": dxs, "weight": dw}
    if root is not None:
        rt = f(root.to(dtype))
        res["root"] = torch.zeros(root.shape, dtype=dtype, device=dev)
        res["x_dst"] = torch.empty(n_dst, root.shape[0], dtype=dtype, device=dev)
        for lo in range(0, n_dst, block):
            xb, gb = f(x_dst[lo:lo + block].to(dtype)), f(g[lo:lo + block].to(dtype))
            out[lo:lo + block] += xb @ rt
            res["root"] += tall_t_matmul(xb, gb)
            res["x_dst"][lo:lo + block] = gb @ rt.t()
    if bias is not None:
        out += f(bias.to(dtype))
        res["bias"] = torch.zeros(g.shape[1], dtype=dtype, device=dev)
        for lo in range(0, n_dst, block):
            res["bias"] += f(g[lo:lo + block].to(dtype)).sum(0)
    return res
