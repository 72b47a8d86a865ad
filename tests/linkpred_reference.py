"""Float64 / integer restatements of the link-prediction kernels (csrc/rgcn_linkpred.hip).  TEST INFRASTRUCTURE ONLY:
plain numpy and Python integers, no torch op that the kernels replace, no GPU."""
import numpy as np

MASK = (1 << 64) - 1
C1, C2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
GOLDEN, NEG_MUL, SIDE_MUL = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, 0x2545F4914F6CDD1D
BAD_NODE, BAD_REL = 1, 2
U32 = 2.0 ** -24


def mix(z: int) -> int:
    """splitmix64's finaliser on Python integers (mod 2^64)"""
    z &= MASK
    z ^= z >> 30
    z = (z * C1) & MASK
    z ^= z >> 27
    z = (z * C2) & MASK
    z ^= z >> 31
    return z


def draw(seed: int, i: int, j: int, num_nodes: int):
    """(node id, replace the object?) of negative j of triple i"""
    d = mix(mix(seed + GOLDEN * (i + 1)) + NEG_MUL * (j + 1))
    return (d * num_nodes) >> 64, (mix(d + SIDE_MUL) >> 63) != 0


def corrupt(s, r, o, num_nodes: int, num_negatives: int, seed: int):
    """(s', r', o') as rgcn_lp_corrupt lays them out: position i * k + j"""
    s, r, o = (np.asarray(a, dtype=np.int64) for a in (s, r, o))
    n = len(s) * num_negatives
    so, ro, oo = np.empty(n, np.int64), np.empty(n, np.int64), np.empty(n, np.int64)
    for i in range(len(s)):
        for j in range(num_negatives):
            node, obj = draw(seed, i, j, num_nodes)
            p = i * num_negatives + j
            so[p], ro[p], oo[p] = (s[i], r[i], node) if obj else (node, r[i], o[i])
    return so, ro, oo


def corrupt_at(s, r, o, num_nodes: int, num_negatives: int, seed: int, positions):
    """(s', r', o') of ``corrupt`` at the given output positions only: a batch too long for the Python-integer loop is checked at
    chosen places"""
    s, r, o = (np.asarray(a, dtype=np.int64) for a in (s, r, o))
    positions = np.asarray(positions, dtype=np.int64)
    so, ro, oo = (np.empty(len(positions), np.int64) for _ in range(3))
    for n, p in enumerate(positions.tolist()):
        i, j = divmod(p, num_negatives)
        node, obj = draw(seed, i, j, num_nodes)
        so[n], ro[n], oo[n] = (s[i], r[i], node) if obj else (node, r[i], o[i])
    return so, ro, oo


def triple_index(s, r, o, num_nodes: int, num_relations: int):
    """What rgcn_lp_index_build must give, by stable argsorts: a dict of ``node_ptr [N + 1]``, ``node_slot`` (the slots 2 t + side of
    the valid triples in (node, slot) order), ``bad_slots`` (the sorted slots of the other triples: the tail of the device's
    node_slot, in any order), ``rel_ptr [R + 1]``, ``rel_triple``, ``bad_triples`` and the ``bad`` word"""
    s, r, o = (np.asarray(a, dtype=np.int64) for a in (s, r, o))
    ok, bad = valid_triples(s, r, o, num_nodes, num_relations)
    slot_node = np.stack([s, o], 1).reshape(-1)                     # slot 2 t + side
    slot_ok = np.repeat(ok, 2)
    slots = np.flatnonzero(slot_ok)
    order = np.argsort(slot_node[slots], kind="stable")
    triples = np.flatnonzero(ok)
    t_order = np.argsort(r[triples], kind="stable")
    return {"node_ptr": np.searchsorted(slot_node[slots][order], np.arange(num_nodes + 1)).astype(np.int64),
            "node_slot": slots[order].astype(np.int64), "bad_slots": np.flatnonzero(~slot_ok).astype(np.int64),
            "rel_ptr": np.searchsorted(r[triples][t_order], np.arange(num_relations + 1)).astype(np.int64),
            "rel_triple": triples[t_order].astype(np.int64), "bad_triples": np.flatnonzero(~ok).astype(np.int64), "bad": bad}


def valid_triples(s, r, o, num_nodes: int, num_relations: int):
    """(mask of the triples whose ids are all in range, the `bad` word the others set)"""
    s, r, o = (np.asarray(a, dtype=np.int64) for a in (s, r, o))
    bad_n = (s < 0) | (s >= num_nodes) | (o < 0) | (o >= num_nodes)
    bad_r = (r < 0) | (r >= num_relations)
    return ~(bad_n | bad_r), (BAD_NODE if bad_n.any() else 0) | (BAD_REL if bad_r.any() else 0)


def score(z, rel, s, r, o):
    """(scores, cond, bad): float64 scores of the triples (0 where an id is out of range) and the same sums on absolute values"""
    z, rel = np.asarray(z, dtype=np.float64), np.asarray(rel, dtype=np.float64)
    s, r, o = (np.asarray(a, dtype=np.int64) for a in (s, r, o))
    ok, bad = valid_triples(s, r, o, z.shape[0], rel.shape[0])
    out, cond = np.zeros(len(s)), np.zeros(len(s))
    out[ok] = (z[s[ok]] * rel[r[ok]] * z[o[ok]]).sum(-1)
    cond[ok] = (np.abs(z[s[ok]]) * np.abs(rel[r[ok]]) * np.abs(z[o[ok]])).sum(-1)
    return out, cond, bad


def backward(z, rel, s, r, o, g):
    """(dz, drel) in float64: dz[v] = sum over v's (triple, side) of g_t rel[r_t] o z[other end] (s == o: twice),
    drel[r] = sum_t g_t z[s_t] o z[o_t]; triples with an id out of range give nothing"""
    z, rel, g = np.asarray(z, dtype=np.float64), np.asarray(rel, dtype=np.float64), np.asarray(g, dtype=np.float64)
    s, r, o = (np.asarray(a, dtype=np.int64) for a in (s, r, o))
    ok, _ = valid_triples(s, r, o, z.shape[0], rel.shape[0])
    s, r, o, g = s[ok], r[ok], o[ok], g[ok]
    dz, drel = np.zeros_like(z), np.zeros_like(rel)
    np.add.at(dz, s, g[:, None] * rel[r] * z[o])
    np.add.at(dz, o, g[:, None] * rel[r] * z[s])
    np.add.at(drel, r, g[:, None] * z[s] * z[o])
    return dz, drel


def backward_cond(z, rel, s, r, o, g):
    a = lambda t: np.abs(np.asarray(t, dtype=np.float64))
    return backward(a(z), a(rel), s, r, o, a(g))


def filter_sets(known, side: str):
    """{(anchor, r): set of completing entities} of int triples [M, 3] by brute force"""
    out = {}
    for s, r, o in np.asarray(known).tolist():
        key, val = ((s, r), o) if side == "object" else ((o, r), s)
        out.setdefault(key, set()).add(val)
    return out


def rank_scores(z, rel, anchor, r):
    """float64 [Q, N] scores (z[a] o rel[r]) . z[e] and their sums on absolute values"""
    z, rel = np.asarray(z, dtype=np.float64), np.asarray(rel, dtype=np.float64)
    q = z[np.asarray(anchor)] * rel[np.asarray(r)]
    return q @ z.T, np.abs(q) @ np.abs(z).T


def rank_counts(scores, target, lists=None, above=None, equal_to=None):
    """(greater, equal) over the candidates that are neither the target nor in the query's list.  Without ``above`` / ``equal_to``
    the comparison is exact (integer inputs); else they are [Q, N] boolean matrices to count."""
    q, n = scores.shape
    target = np.asarray(target)
    t = scores[np.arange(q), target][:, None]
    above = scores > t if above is None else above
    equal_to = scores == t if equal_to is None else equal_to
    keep = np.ones((q, n), dtype=bool)
    keep[np.arange(q), target] = False
    if lists is not None:
        for i, ids in enumerate(lists):
            ids = [e for e in ids if 0 <= e < n]
            keep[i, ids] = False
    return (above & keep).sum(1).astype(np.int64), (equal_to & keep).sum(1).astype(np.int64)


def rank_band(z, rel, anchor, r, target, lists=None):
    """(lo, hi): bounds of ``greater`` for a fp32 ranking pass -- candidates with s64 > t64 + tau and with s64 > t64 - tau,
    tau = 4 * 2^-24 * (cond(q, e) + cond(q, target))"""
    sc, cond = rank_scores(z, rel, anchor, r)
    q = sc.shape[0]
    target = np.asarray(target)
    t = sc[np.arange(q), target][:, None]
    tau = 4 * U32 * (cond + cond[np.arange(q), target][:, None])
    lo, _ = rank_counts(sc, target, lists, above=sc > t + tau)
    hi, _ = rank_counts(sc, target, lists, above=sc > t - tau)
    return lo, hi


def metrics(greater, equal, ks=(1, 3, 10), ties="mean"):
    greater, equal = np.asarray(greater, dtype=np.float64), np.asarray(equal, dtype=np.float64)
    rank = 1 + greater + (equal / 2 if ties == "mean" else 0)
    out = {"mrr": float(np.mean(1 / rank))}
    for k in ks:
        out[f"hits@{k}"] = float(np.mean(rank <= k))
    return out
