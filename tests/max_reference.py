"""Float64 reference of RGCNConv(aggr="max") as PyG 2.3.1 computes it without torch_scatter: per relation
``x.new_zeros(...).scatter_reduce(0, dst, x[src], "amax", include_self=False)``, then ``h @ W_r`` (basis: W_r = comp_r . bases;
blocks: the block-diagonal W_r), ``+ x @ root + bias``; backward by torch autograd.  TEST INFRASTRUCTURE ONLY (CPU, any device
for the inputs: everything is moved to the CPU in float64)."""
import math
from typing import Optional

import torch


def graph_case(name: str, n: int = 300, e: int = 3000, r: int = 5, seed: int = 0):
    """(edge_index [2, E] int64, edge_type [E] int64) of the graph cases the max tests share:
    * "plain": random edges, duplicate triples, relation r - 1 unused, the last 20 nodes without in-edges (isolated as
      destinations; the last 5 without any edge at all);
    * "hubs": "plain" plus a destination hub (node 0: 700 in-edges of relation 0, one segment of three PIECE pieces) and a
      source hub (node 1: 700 out-edges) -- both walked in two levels;
    * "empty": no edge at all."""
    g = torch.Generator().manual_seed(seed)
    if name == "empty":
        return torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)
    src = torch.randint(0, n - 5, (e,), generator=g)
    dst = torch.randint(0, n - 20, (e,), generator=g)
    typ = torch.randint(0, r - 1, (e,), generator=g)
    ei = torch.cat([torch.stack([src, dst]), torch.stack([src[:150], dst[:150]])], 1)     # duplicate triples
    et = torch.cat([typ, typ[:150]])
    if name == "hubs":
        k = 700
        hub_src = torch.randint(2, n - 5, (k,), generator=g)
        hub_dst = torch.randint(2, n - 20, (k,), generator=g)
        ei = torch.cat([ei, torch.stack([hub_src, torch.zeros(k, dtype=torch.int64)]),
                        torch.stack([torch.ones(k, dtype=torch.int64), hub_dst])], 1)
        et = torch.cat([et, torch.zeros(k, dtype=torch.int64), torch.randint(0, r - 1, (k,), generator=g)])
    elif name != "plain":
        raise ValueError(name)
    return ei, et


def features(kind: str, n: int, din: int, seed: int = 1) -> torch.Tensor:
    """float32 [n, din]: "normal"; "ties" (integers in -2..2: most maxima are attained by several edges); "negative" (every
    value below zero: the max must not start at 0)"""
    g = torch.Generator().manual_seed(seed)
    if kind == "ties":
        return torch.randint(-2, 3, (n, din), generator=g).float()
    x = torch.randn(n, din, generator=g)
    if kind == "negative":
        return -(x.abs() + 0.25)
    assert kind == "normal", kind
    return x


def dense_weight(weight: torch.Tensor, comp: Optional[torch.Tensor], num_relations: int, din: int, dout: int) -> torch.Tensor:
    """[R, din, dout] from the layer's own parametrisation (differentiable)"""
    if comp is not None:
        return (comp @ weight.reshape(weight.shape[0], -1)).view(num_relations, din, dout)
    if weight.dim() == 4:
        nb = weight.shape[1]
        eye = torch.eye(nb, dtype=weight.dtype)
        return torch.einsum("rbio,bc->rbico", weight, eye).reshape(num_relations, din, dout)
    return weight


def max_aggregate(x: torch.Tensor, ei: torch.Tensor, et: torch.Tensor, num_relations: int):
    """[H_r for r in range(R)]: torch scatter_reduce amax, include_self=False, zero fill (PyG 2.3.1 without torch_scatter)"""
    n, din = x.shape
    hs = []
    for r in range(num_relations):
        m = et == r
        src, dst = ei[0][m], ei[1][m]
        hs.append(x.new_zeros(n, din).scatter_reduce(0, dst[:, None].expand(-1, din), x[src], "amax", include_self=False))
    return hs


def max_layer(x, ei, et, weight, comp, root, bias, num_relations: int, act: Optional[str] = None):
    """out of the layer (differentiable in every tensor argument)"""
    din = x.shape[1]
    dout = root.shape[1] if root is not None else (weight.shape[2] if weight.dim() == 3 else weight.shape[1] * weight.shape[3])
    w = dense_weight(weight, comp, num_relations, din, dout)
    out = x.new_zeros(x.shape[0], dout)
    for r, h in enumerate(max_aggregate(x, ei, et, num_relations)):
        out = out + h @ w[r]
    if root is not None:
        out = out + x @ root
    if bias is not None:
        out = out + bias
    if act == "relu":
        out = torch.relu(out)
    elif act == "sigmoid":
        out = torch.sigmoid(out)
    return out


def reference(conv, x: torch.Tensor, ei: torch.Tensor, et: torch.Tensor, g: torch.Tensor):
    """float64 (out, {name: grad}) of the module ``conv``'s parameters on (x, graph), upstream gradient g; grads of x and of
    every parameter (frozen or not: the tests pick what they compare)"""
    c = lambda t: None if t is None else t.detach().cpu().double().clone().requires_grad_(True)
    xd, ei, et = c(x), ei.cpu(), et.cpu()
    ps = {k: c(getattr(conv, k)) for k in ("weight", "comp", "root", "bias")}
    out = max_layer(xd, ei, et, ps["weight"], ps["comp"], ps["root"], ps["bias"], conv.num_relations)
    out.backward(g.detach().cpu().double())
    grads = {"x": xd.grad.numpy()}
    grads.update({k: v.grad.numpy() for k, v in ps.items() if v is not None})
    return out.detach().numpy(), grads


def conditions(conv, x: torch.Tensor, ei: torch.Tensor, et: torch.Tensor, g: torch.Tensor):
    """(out_cond, {name: cond}): every output and gradient element as the sum of the absolute values of its terms (the
    bound 4 u cond of oracle/tolerance.py).  The selection of the maxima is exact, so only sums and products round: H and the
    tie masks come from x itself, every other factor enters by its absolute value (a decomposition: |comp| . |bases|)."""
    f = lambda t: None if t is None else t.detach().cpu().double()
    xd, ei, et, gd = f(x), ei.cpu(), et.cpu(), f(g).abs()
    r, din = conv.num_relations, conv.in_channels
    weight, comp, root, bias = (f(getattr(conv, k)) for k in ("weight", "comp", "root", "bias"))
    wabs = dense_weight(weight.abs(), None if comp is None else comp.abs(), r, din, conv.out_channels)
    hs = [h.abs() for h in max_aggregate(xd, ei, et, r)]
    out = sum(h @ wabs[q] for q, h in enumerate(hs)) + (0 if root is None else xd.abs() @ root.abs()) + (0 if bias is None else bias.abs())
    # dX: the reference's own backward with every factor non-negative and the same tie masks
    xg = xd.clone().requires_grad_(True)
    o = max_layer(xg, ei, et, wabs, None, None if root is None else root.abs(), None, r)
    o.backward(gd)
    dw = torch.stack([h.t() @ gd for h in hs])
    conds = {"x": xg.grad.numpy(), "bias": gd.sum(0).numpy()}
    if root is not None:
        conds["root"] = (xd.abs().t() @ gd).numpy()
    if comp is not None:
        conds["weight"] = torch.einsum("rb,rio->bio", comp.abs(), dw).numpy()
        conds["comp"] = torch.einsum("rio,bio->rb", dw, weight.abs()).numpy()
    elif weight.dim() == 4:
        nb = weight.shape[1]
        bi, bo = din // nb, conv.out_channels // nb
        conds["weight"] = dw.view(r, nb, bi, nb, bo).diagonal(dim1=1, dim2=3).permute(0, 3, 1, 2).numpy()
    else:
        conds["weight"] = dw.numpy()
    return out.numpy(), conds


def num_blocks_for(din: int, dout: int) -> int:
    """the largest of 4, 2, 1 that divides both widths"""
    return max(b for b in (4, 2, 1) if din % b == 0 and dout % b == 0 and math.gcd(din, dout) % b == 0)


# ---- at scale: a graph with an exact segment count, and the layer relation by relation in row blocks (any device) ------------
def exact_segment_graph(n: int, r: int, n_seg: int, extra: int, device, seed: int, hub: int = 70_000, dup: int = 50_000):
    """A graph of exactly ``n_seg`` distinct (destination, relation) pairs over relations 0 .. r - 2 (relation r - 1 stays dead):
    pair k is ``(m - 1 + k a) mod m`` of the m = n (r - 1) pairs ``dst * (r - 1) + rel``, a coprime to m, so the pairs are
    distinct and pair 0 is (n - 1, r - 2): the last node is a destination and the last segment is not empty.  Then, into
    existing pairs only (the count does not move): ``extra`` more rows, ``hub`` rows into pair 1 (one long segment), ``hub``
    out-edges of node 7 (one long source), the last node as a source, and the first ``dup`` edges once more (duplicate
    triples).  Returns the dict of tests/test_gpu_past_4gib.py make_graph (without its mean weights): n, r, ei, et and the
    edges sorted by relation (src_s, dst_s, bounds)."""
    live = r - 1
    m = n * live
    assert 2 <= n_seg <= m and live >= 1
    a = 2654435761 % m
    while math.gcd(a, m) != 1:
        a += 1
    g = torch.Generator(device=device).manual_seed(seed)
    p = (m - 1 + torch.arange(n_seg, device=device) * a) % m
    more = lambda k: p[torch.randint(0, n_seg, (k,), generator=g, device=device)]
    p = torch.cat([p, more(extra), p[1].expand(hub), more(hub)])
    src = torch.randint(0, n, (p.numel(),), generator=g, device=device)
    src[0] = n - 1
    src[-hub:] = 7
    p, src = torch.cat([p, p[:dup]]), torch.cat([src, src[:dup]])
    dst, et = p // live, p % live
    ei = torch.stack([src, dst]).contiguous()
    perm = torch.argsort(et, stable=True)
    counts = torch.bincount(et, minlength=r).tolist()
    bounds, lo = [], 0
    for c in counts:
        bounds.append((lo, lo + c))
        lo += c
    assert counts[r - 1] == 0
    return dict(n=n, r=r, ei=ei, et=et.contiguous(), src_s=src[perm], dst_s=dst[perm], bounds=bounds)


def blocked_layer(G, x, g, w, root, bias, dtype, absval: bool = False, blk: int = 1 << 22):
    """(out, d_x, d_weight, d_root, d_bias) of the max layer on the device of x in ``dtype``, sharing nothing with the plans:
    per relation ``h = zeros.scatter_reduce(0, dst, x[src], "amax", include_self=False)``, ``o_r = h @ W_r`` added to the output
    and ``torch.autograd.grad(o_r, [x, W_r], g)`` to the gradients -- torch's own tie rule; root and bias in row blocks.  With
    ``absval`` the condition sums of oracle/tolerance.py bound (1): the same passes with |W|, |root|, |g|, |bias| and |h|, |x| as
    factors, the maxima and the tie masks still from x itself (the rule of ``conditions``).  G: exact_segment_graph / make_graph."""
    f = (lambda t: t.abs()) if absval else (lambda t: t)
    n, din = x.shape
    dout = w.shape[2]
    xd = x.detach().to(dtype).requires_grad_(True)      # (detach: never the caller's own tensor)
    gd = f(g.to(dtype))
    out = torch.zeros(n, dout, dtype=dtype, device=x.device)
    dx = torch.zeros(n, din, dtype=dtype, device=x.device)
    dw = torch.zeros(G["r"], din, dout, dtype=dtype, device=x.device)
    for rel, (lo, hi) in enumerate(G["bounds"]):
        if hi == lo:
            continue
        src, dst = G["src_s"][lo:hi], G["dst_s"][lo:hi]
        wr = f(w[rel].to(dtype)).requires_grad_(True)
        h = xd.new_zeros(n, din).scatter_reduce(0, dst[:, None].expand(-1, din), xd[src], "amax", include_self=False)
        o = h @ wr
        gx, gw = torch.autograd.grad(o, [xd, wr], gd)
        dx += gx
        with torch.no_grad():
            if absval:                      # |h| is a factor of out and d_weight; d_x has no factor h (the masks alone)
                ha = h.abs()
                out += ha @ wr
                dw[rel] = ha.t() @ gd
                del ha
            else:
                out += o
                dw[rel] = gw
        del h, o, gx, gw
    xd = xd.detach()
    rm = f(root.to(dtype))
    dr = torch.zeros(din, dout, dtype=dtype, device=x.device)
    db = torch.zeros(dout, dtype=dtype, device=x.device)
    for lo in range(0, n, blk):
        xb, gb = f(xd[lo:lo + blk]), gd[lo:lo + blk]
        out[lo:lo + blk] += xb @ rm
        dx[lo:lo + blk] += gb @ rm.t()
        dr += xb.t() @ gb
        db += gb.sum(0)
    if bias is not None:
        out += f(bias.to(dtype))
    return out, dx, dw, dr, db
