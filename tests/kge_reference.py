"""Float64 restatements of the ComplEx and TransE kernels (csrc/rgcn_kge.hip).  TEST INFRASTRUCTURE ONLY: plain numpy, no
torch op that the kernels replace, no GPU.  ``dec`` is "complex" (columns 2k, 2k + 1: real and imaginary part of component k) or
"transe" (L1).  ``absolute=True`` evaluates the same sums on absolute values: the ``cond`` of ``oracle.tolerance.assert_close``."""
import numpy as np

from tests.linkpred_reference import U32, rank_counts, valid_triples


def _cmul(x, y, conj_x, absolute):
    """x o y (conj_x: conj(x) o y) on interleaved rows; absolute: every product of parts taken on absolute values and added"""
    a, b, c, d = x[..., 0::2], x[..., 1::2], y[..., 0::2], y[..., 1::2]
    if absolute:
        re, im = np.abs(a * c) + np.abs(b * d), np.abs(a * d) + np.abs(b * c)
    elif conj_x:
        re, im = a * c + b * d, a * d - b * c
    else:
        re, im = a * c - b * d, a * d + b * c
    return np.stack([re, im], -1).reshape(x.shape)


def parts(dec, zs, rr, zo, absolute=False):
    """per triple, from the three gathered rows: (score, d score / d s, d / d r, d / d o)"""
    if dec == "transe":
        d = (zs + rr) - zo
        if absolute:
            return (np.abs(zs) + np.abs(rr) + np.abs(zo)).sum(-1), np.abs(np.sign(d)), np.abs(np.sign(d)), np.abs(np.sign(d))
        return -np.abs(d).sum(-1), -np.sign(d), -np.sign(d), np.sign(d)
    q = _cmul(zs, rr, False, absolute)
    score = (np.abs(q * zo) if absolute else q * zo).sum(-1)
    return score, _cmul(rr, zo, True, absolute), _cmul(zs, zo, True, absolute), q


def score(dec, z, rel, s, r, o, absolute=False):
    """(scores, bad): float64 scores of the triples, 0 where an id is out of range"""
    z, rel = np.asarray(z, dtype=np.float64), np.asarray(rel, dtype=np.float64)
    s, r, o = (np.asarray(a, dtype=np.int64) for a in (s, r, o))
    ok, bad = valid_triples(s, r, o, z.shape[0], rel.shape[0])
    out = np.zeros(len(s))
    out[ok] = parts(dec, z[s[ok]], rel[r[ok]], z[o[ok]], absolute)[0]
    return out, bad


def backward(dec, z, rel, s, r, o, g, absolute=False):
    """(dz, drel) in float64; a triple with s == o gives its node both ends; triples with an id out of range give nothing"""
    z, rel, g = (np.asarray(a, dtype=np.float64) for a in (z, rel, g))
    s, r, o = (np.asarray(a, dtype=np.int64) for a in (s, r, o))
    ok, _ = valid_triples(s, r, o, z.shape[0], rel.shape[0])
    s, r, o, g = s[ok], r[ok], o[ok], (np.abs(g[ok]) if absolute else g[ok])[:, None]
    _, ds, dr, do = parts(dec, z[s], rel[r], z[o], absolute)
    dz, drel = np.zeros_like(z), np.zeros_like(rel)
    np.add.at(dz, s, g * ds)
    np.add.at(dz, o, g * do)
    np.add.at(drel, r, g * dr)
    return dz, drel


def rank_scores(dec, z, rel, anchor, r, side):
    """float64 [Q, N] scores of every entity as the object of (anchor, r, ?) (``side="object"``) or the subject of (?, r, anchor),
    and the same sums on absolute values"""
    z, rel = np.asarray(z, dtype=np.float64), np.asarray(rel, dtype=np.float64)
    out = [np.empty((len(anchor), z.shape[0])) for _ in range(2)]
    for i, (a, t) in enumerate(zip(np.asarray(anchor).tolist(), np.asarray(r).tolist())):
        za, rt = np.broadcast_to(z[a], z.shape), np.broadcast_to(rel[t], z.shape)
        for k, absolute in enumerate((False, True)):
            out[k][i] = parts(dec, za, rt, z, absolute)[0] if side == "object" else parts(dec, z, rt, za, absolute)[0]
    return out


def rank_band(sc, cond, target, lists=None):
    """(lo, hi): bounds of ``greater`` for a fp32 ranking pass, tau = 4 * 2^-24 * (cond(q, e) + cond(q, target))"""
    rows, target = np.arange(sc.shape[0]), np.asarray(target)
    t = sc[rows, target][:, None]
    tau = 4 * U32 * (cond + cond[rows, target][:, None])
    return rank_counts(sc, target, lists, above=sc > t + tau)[0], rank_counts(sc, target, lists, above=sc > t - tau)[0]
