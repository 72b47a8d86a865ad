"""The softmax link-prediction loss in plain float64 torch on the CPU: the decoder's query row by its formula,
``logits = q @ z.T``, ``logsumexp - gather`` and gradients by autograd; beside them the same sums on absolute values, with every
weight's own error included, which the GPU tests pass to ``oracle.tolerance.assert_close`` as ``cond``."""
import torch


def _complex(t):
    return torch.view_as_complex(t.reshape(t.shape[0], -1, 2))


def query(dec, z, rel, anchor, r, side):
    """q [Q, E]: DistMult z[a] o rel[r]; ComplEx s o r (object side) or conj(r) o o (subject side), interleaved columns"""
    if dec == "distmult":
        return z[anchor] * rel[r]
    zc, rc = _complex(z)[anchor], _complex(rel)[r]
    return torch.view_as_real(zc * rc if side == "object" else rc.conj() * zc).flatten(1)


def _absmul(dec, c, y):
    """|d (x o y) / dx| applied to the bound c: the products of a component on absolute values (a conjugate only moves signs)"""
    y = y.abs()
    if dec == "distmult":
        return c * y
    c, y = c.reshape(c.shape[0], -1, 2), y.reshape(y.shape[0], -1, 2)
    return torch.stack([c[..., 0] * y[..., 0] + c[..., 1] * y[..., 1], c[..., 0] * y[..., 1] + c[..., 1] * y[..., 0]], -1).flatten(1)


def softmax_loss(dec, z, rel, s, r, o, g, side):
    """dict of float64 numpy arrays: loss [Q], dz, drel for the upstream gradient g, their conds, the logits and the `bad` word"""
    z, rel, g = z.double().requires_grad_(True), rel.double().requires_grad_(True), g.double()
    n, nrel = z.shape[0], rel.shape[0]
    ok = (s >= 0) & (s < n) & (o >= 0) & (o < n) & (r >= 0) & (r < nrel)
    bad = (1 if bool(((s < 0) | (s >= n) | (o < 0) | (o >= n)).any()) else 0) | (2 if bool(((r < 0) | (r >= nrel)).any()) else 0)
    anchor, target = ((s, o) if side == "object" else (o, s))
    anchor, target, rr = anchor[ok], target[ok], r[ok]
    q = query(dec, z, rel, anchor, rr, side)
    logits = q @ z.T
    live = torch.logsumexp(logits, 1) - logits.gather(1, target[:, None])[:, 0]
    (live * g[ok]).sum().backward()
    loss = torch.zeros(len(s), dtype=torch.float64)
    loss[ok] = live.detach()
    with torch.no_grad():
        big = 1 + (q.abs() @ z.abs().T).max(1).values                      # 1 + L_i
        w = torch.softmax(logits, 1)
        w[torch.arange(len(target)), target] += 1                          # |w_in| / |g_i| on absolute values
        w = w * (g[ok].abs() * big)[:, None]                               # ... with the weight's own error: x (1 + L_i)
        c_dq = w @ z.abs()
        c_dz = (w.T @ q.abs()).index_add_(0, anchor, _absmul(dec, c_dq, rel[rr]))
        c_drel = torch.zeros_like(rel).index_add_(0, rr, _absmul(dec, c_dq, z[anchor]))
        c_loss = torch.ones(len(s), dtype=torch.float64)
        c_loss[ok] = big
    num = lambda t: t.detach().numpy()
    return dict(loss=num(loss), dz=num(z.grad), drel=num(rel.grad), c_loss=num(c_loss), c_dz=num(c_dz), c_drel=num(c_drel),
                logits=num(logits), bad=bad, q=num(q))
