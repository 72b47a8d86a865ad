"""The row-wise Adam step of csrc/rgcn_emb_rows.hip restated in float64 numpy, for tests/test_row_adam_reference.py
(against torch.optim.Adam on the CPU) and the GPU tests of the kernel.  ``table, m, v``: float64 ``[N, E]`` or ``[S, N, E]``,
``step``: integer ``[N]``; all four are updated IN PLACE.  ``nodes``: ``[n]`` ids, ``grads``: ``[n, E]`` or ``[S, n, E]``, one
gradient row per position.  ``hyper``: dict with lr, beta1, beta2, eps, weight_decay.  Ids outside ``[0, N)`` update nothing;
their number is returned."""
import numpy as np


def tolerance(k, max_abs_p, lr):
    """per element after k steps, k (2^-22 max|p| + 2^-18 lr): the half-ulp rounding of p per step, and about 32 ulp on the step
    itself (whose size is about lr) -- ten roundings and their carry through m, v over a handful of steps"""
    return k * (2.0 ** -22 * max_abs_p + 2.0 ** -18 * lr)


def row_adam_step(table, m, v, step, nodes, grads, hyper):
    lr, b1, b2, eps, wd = (float(hyper[k]) for k in ("lr", "beta1", "beta2", "eps", "weight_decay"))
    n_nodes = table.shape[-2]
    nodes = np.asarray(nodes, dtype=np.int64)
    grads = np.asarray(grads, dtype=np.float64)
    bad = 0
    done = set()
    for pos, n in enumerate(nodes.tolist()):
        if n < 0 or n >= n_nodes:
            bad += 1
            continue
        if n in done:
            continue
        done.add(n)
        g = np.zeros_like(grads[..., 0, :])
        for q in np.nonzero(nodes == n)[0]:          # ascending position order
            g = g + grads[..., q, :]
        p = table[..., n, :]
        g = g + wd * p
        step[n] += 1
        t = int(step[n])
        m[..., n, :] = b1 * m[..., n, :] + (1.0 - b1) * g
        v[..., n, :] = b2 * v[..., n, :] + (1.0 - b2) * g * g
        table[..., n, :] = p - lr * (m[..., n, :] / (1.0 - b1 ** t)) / (np.sqrt(v[..., n, :] / (1.0 - b2 ** t)) + eps)
    return bad
