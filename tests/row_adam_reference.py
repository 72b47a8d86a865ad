"""The row-wise Adam step of csrc/rgcn_emb_rows.hip restated in float64 numpy, for tests/test_row_adam_reference.py
(against torch.optim.Adam on the CPU) and the GPU tests of the kernel.  ``table, m, v``: float64 ``[N, E]`` or ``[S, N, E]``,
``step``: integer ``[N]``; all four are updated IN PLACE.  ``nodes``: ``[n]`` ids, ``grads``: ``[n, E]`` or ``[S, n, E]``, one
gradient row per position.  ``hyper``: dict with lr, beta1, beta2, eps, weight_decay.  Ids outside ``[0, N)`` update nothing;
their number is returned.  ``row_adam_step`` is the plain loop; ``row_adam_step_vectorised`` is its twin for lists of thousands of
positions; ``run_sums`` / ``order_changes_bits`` are the sequential per-id sums on which the bit-for-bit test of the position
order rests."""
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


def run_sums(nodes, grads, n_nodes, dtype=np.float64, descending=False):
    """(ids, sums, counts): the distinct ids of ``nodes`` inside ``[0, n_nodes)`` in ascending order, for each the sum of its rows
    of ``grads`` (``[n, E]`` or ``[S, n, E]``) taken SEQUENTIALLY in ascending position order (descending: from its last position
    back) with every partial sum rounded to ``dtype``, and the number of its positions.  One pass per occurrence rank: pass r adds
    the r-th row of every id that has one, so the order of the additions within an id is the loop's."""
    nodes = np.asarray(nodes, dtype=np.int64).reshape(-1)
    grads = np.asarray(grads).astype(dtype, copy=False)
    pos = np.nonzero((nodes >= 0) & (nodes < n_nodes))[0]
    order = np.lexsort((-pos if descending else pos, nodes[pos]))
    pos, sid = pos[order], nodes[pos][order]
    ids, start, counts = np.unique(sid, return_index=True, return_counts=True)
    sums = np.zeros(grads.shape[:-2] + (len(ids), grads.shape[-1]), dtype=dtype)
    if len(ids) == 0:
        return ids, sums, counts
    group = np.repeat(np.arange(len(ids)), counts)
    rank = np.arange(len(sid)) - np.repeat(start, counts)
    by_rank = np.argsort(rank, kind="stable")
    ends = np.cumsum(np.bincount(rank))
    lo = 0
    for r, hi in enumerate(ends.tolist()):
        sel = by_rank[lo:hi]                          # every id at most once
        if r == 0:
            sums[..., group[sel], :] = grads[..., pos[sel], :]
        else:
            sums[..., group[sel], :] = sums[..., group[sel], :] + grads[..., pos[sel], :]
        lo = hi
    return ids, sums, counts


def row_adam_step_vectorised(table, m, v, step, nodes, grads, hyper):
    """``row_adam_step`` without the Python loop over the ids (float64 throughout, the same in-place updates, the same return
    value): tests/test_row_adam_reference.py holds the two together to 1e-12"""
    lr, b1, b2, eps, wd = (float(hyper[k]) for k in ("lr", "beta1", "beta2", "eps", "weight_decay"))
    n_nodes = table.shape[-2]
    nodes = np.asarray(nodes, dtype=np.int64).reshape(-1)
    bad = int(np.count_nonzero((nodes < 0) | (nodes >= n_nodes)))
    ids, g, _ = run_sums(nodes, np.asarray(grads, dtype=np.float64), n_nodes)
    if len(ids) == 0:
        return bad
    p = table[..., ids, :]
    g = g + wd * p
    step[ids] += 1
    t = step[ids].astype(np.float64)[:, None]
    m_new = b1 * m[..., ids, :] + (1.0 - b1) * g
    v_new = b2 * v[..., ids, :] + (1.0 - b2) * g * g
    m[..., ids, :] = m_new
    v[..., ids, :] = v_new
    table[..., ids, :] = p - lr * (m_new / (1.0 - np.power(b1, t))) / (np.sqrt(v_new / (1.0 - np.power(b2, t))) + eps)
    return bad


def order_changes_bits(nodes, grads32, n_nodes):
    """(ids listed more than once, those whose fp32 sum changes its bits when the rows are added in descending position order,
    fraction of their elements that change): what makes a bit-for-bit test of the position order able to fail"""
    grads32 = np.asarray(grads32, dtype=np.float32)
    ids, up, counts = run_sums(nodes, grads32, n_nodes, np.float32)
    _, down, _ = run_sums(nodes, grads32, n_nodes, np.float32, descending=True)
    many = counts > 1
    differ = up.view(np.uint32)[..., many, :] != down.view(np.uint32)[..., many, :]
    per_id = differ.any(axis=-1)
    if per_id.ndim > 1:
        per_id = per_id.any(axis=0)
    return int(many.sum()), int(per_id.sum()), float(differ.mean()) if differ.size else 0.0
