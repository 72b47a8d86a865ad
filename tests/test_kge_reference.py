"""tests/kge_reference.py against torch autograd in float64: ComplEx through ``view_as_complex``, TransE as
``-(s + r - o).abs().sum(-1)``.  No GPU."""
import numpy as np
import pytest
import torch

from tests import kge_reference as K


def torch_score(dec, z, rel, s, r, o):
    if dec == "transe":
        return -(z[s] + rel[r] - z[o]).abs().sum(-1)
    cx = lambda t: torch.view_as_complex(t.reshape(t.shape[0], -1, 2))
    return (cx(z)[s] * cx(rel)[r] * cx(z)[o].conj()).real.sum(-1)


def _case(dec, seed, n=30, nrel=4, dim=6, t=200):
    g = torch.Generator().manual_seed(seed)
    z, rel = (torch.randint(-64, 65, (rows, dim), generator=g).double() / 16 for rows in (n, nrel))     # exact d, planted zeros of d
    s, o = (torch.randint(0, n, (t,), generator=g) for _ in range(2))
    r = torch.randint(0, nrel, (t,), generator=g)
    s[:5] = o[:5]
    s[7], r[8], o[9] = n, -1, 2 ** 40
    return z, rel, s, r, o, torch.randn(t, generator=g).double()


@pytest.mark.parametrize("dec", ["complex", "transe"])
def test_restatement_matches_autograd(dec):
    z, rel, s, r, o, g = _case(dec, seed=3)
    ok, bad = K.valid_triples(s.numpy(), r.numpy(), o.numpy(), 30, 4)
    assert bad == 3 and (~ok).sum() == 3
    zt, rt = z.clone().requires_grad_(True), rel.clone().requires_grad_(True)
    keep = torch.as_tensor(ok)
    out = torch_score(dec, zt, rt, s[keep], r[keep], o[keep])
    out.backward(g[keep])
    got, got_bad = K.score(dec, z.numpy(), rel.numpy(), s.numpy(), r.numpy(), o.numpy())
    assert got_bad == 3 and not got[~ok].any()
    np.testing.assert_allclose(got[ok], out.detach().numpy(), rtol=1e-13, atol=1e-13)
    dz, drel = K.backward(dec, z.numpy(), rel.numpy(), s.numpy(), r.numpy(), o.numpy(), g.numpy())
    np.testing.assert_allclose(dz, zt.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(drel, rt.grad.numpy(), rtol=1e-12, atol=1e-12)
    if dec == "transe":
        assert ((z[s[keep]] + rel[r[keep]] - z[o[keep]]) == 0).any()           # sign(0) = 0 is exercised
    # the sums on absolute values bound the sums
    assert (np.abs(got) <= K.score(dec, z.numpy(), rel.numpy(), s.numpy(), r.numpy(), o.numpy(), absolute=True)[0] + 1e-12).all()
    assert (np.abs(dz) <= K.backward(dec, z.numpy(), rel.numpy(), s.numpy(), r.numpy(), o.numpy(), g.numpy(), absolute=True)[0] + 1e-12).all()


@pytest.mark.parametrize("dec", ["complex", "transe"])
def test_rank_scores_are_the_scores_of_the_completed_triples(dec):
    z, rel, s, r, o, _ = _case(dec, seed=5)
    s, r, o = s[10:60], r[10:60], o[10:60]
    ref, _ = K.score(dec, z.numpy(), rel.numpy(), s.numpy(), r.numpy(), o.numpy())
    obj, c_obj = K.rank_scores(dec, z.numpy(), rel.numpy(), s.numpy(), r.numpy(), "object")
    sub, c_sub = K.rank_scores(dec, z.numpy(), rel.numpy(), o.numpy(), r.numpy(), "subject")
    rows = np.arange(50)
    np.testing.assert_allclose(obj[rows, o.numpy()], ref, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(sub[rows, s.numpy()], ref, rtol=1e-13, atol=1e-13)
    assert not np.allclose(obj, K.rank_scores(dec, z.numpy(), rel.numpy(), s.numpy(), r.numpy(), "subject")[0])      # not symmetric
    assert (np.abs(obj) <= c_obj + 1e-12).all() and (np.abs(sub) <= c_sub + 1e-12).all()
