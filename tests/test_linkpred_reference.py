"""tests/linkpred_reference.py against torch autograd in float64 and against its own definitions: the restatement the
GPU tests compare the kernels with must itself be right.  CPU only."""
import numpy as np
import torch

from tests import linkpred_reference as R


def _case(seed=0, n_nodes=30, n_rel=4, width=12, n=400):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n_nodes, width, generator=g, dtype=torch.float64)
    rel = torch.randn(n_rel, width, generator=g, dtype=torch.float64)
    s, o = (torch.randint(0, n_nodes, (n,), generator=g) for _ in range(2))
    r = torch.randint(0, n_rel, (n,), generator=g)
    s[:5] = o[:5]                                   # s == o contributes twice
    return z, rel, s, r, o, torch.randn(n, generator=g, dtype=torch.float64)


def test_score_and_gradients_match_autograd():
    z, rel, s, r, o, g = _case()
    zt, rt = z.clone().requires_grad_(True), rel.clone().requires_grad_(True)
    out = (zt[s] * rt[r] * zt[o]).sum(-1)
    out.backward(g)
    got, cond, bad = R.score(z.numpy(), rel.numpy(), s.numpy(), r.numpy(), o.numpy())
    assert bad == 0 and np.allclose(got, out.detach().numpy(), rtol=1e-13, atol=1e-13) and (cond >= np.abs(got) - 1e-12).all()
    dz, drel = R.backward(z.numpy(), rel.numpy(), s.numpy(), r.numpy(), o.numpy(), g.numpy())
    assert np.allclose(dz, zt.grad.numpy(), rtol=1e-12, atol=1e-12) and np.allclose(drel, rt.grad.numpy(), rtol=1e-12, atol=1e-12)
    c_dz, c_drel = R.backward_cond(z.numpy(), rel.numpy(), s.numpy(), r.numpy(), o.numpy(), g.numpy())
    assert (c_dz >= np.abs(dz) - 1e-12).all() and (c_drel >= np.abs(drel) - 1e-12).all()


def test_ids_out_of_range_give_nothing():
    z, rel, s, r, o, g = _case(1)
    s2, r2, o2 = s.clone(), r.clone(), o.clone()
    s2[7], o2[8], r2[9], r2[10] = 30, -1, 4, -2
    got, _, bad = R.score(z.numpy(), rel.numpy(), s2.numpy(), r2.numpy(), o2.numpy())
    assert bad == R.BAD_NODE | R.BAD_REL and not got[7:11].any()
    keep = np.ones(len(s), dtype=bool)
    keep[7:11] = False
    dz, drel = R.backward(z.numpy(), rel.numpy(), s2.numpy(), r2.numpy(), o2.numpy(), g.numpy())
    dz_k, drel_k = R.backward(z.numpy(), rel.numpy(), s.numpy()[keep], r.numpy()[keep], o.numpy()[keep], g.numpy()[keep])
    assert np.array_equal(dz, dz_k) and np.array_equal(drel, drel_k)


def test_mix_is_the_samplers():
    from tests import sampling_reference as S
    for v in (0, 1, 2 ** 63, 2 ** 64 - 1, 0x9E3779B97F4A7C15):
        assert R.mix(v) == S.mix(v)


def test_corrupt_properties():
    g = torch.Generator().manual_seed(2)
    n, k, n_nodes = 500, 5, 1000
    s, o = (torch.randint(0, n_nodes, (n,), generator=g).numpy() for _ in range(2))
    r = torch.randint(0, 7, (n,), generator=g).numpy()
    so, ro, oo = R.corrupt(s, r, o, n_nodes, k, seed=99)
    rep = lambda a: np.repeat(a, k)
    assert np.array_equal(ro, rep(r))
    assert (((so != rep(s)).astype(int) + (oo != rep(o)).astype(int)) <= 1).all()           # at most one end differs
    assert (so >= 0).all() and (so < n_nodes).all() and (oo >= 0).all() and (oo < n_nodes).all()
    changed_s, changed_o = (so != rep(s)).mean(), (oo != rep(o)).mean()
    assert 0.4 < changed_s < 0.6 and 0.4 < changed_o < 0.6                                  # one bit chooses the end
    assert len(np.unique(np.concatenate([so[so != rep(s)], oo[oo != rep(o)]]))) > 800      # the ids spread over the nodes
    # a function of (seed, i, j): a prefix of the batch gives a prefix of the result; another seed gives other draws
    for a, b in zip(R.corrupt(s[:100], r[:100], o[:100], n_nodes, k, seed=99), (so, ro, oo)):
        assert np.array_equal(a, b[:100 * k])
    assert not np.array_equal(R.corrupt(s, r, o, n_nodes, k, seed=100)[0], so)
    # num_nodes enters only through the multiply-high reduction
    for nn in (1, 2, 2 ** 31 - 1):
        ids = [R.draw(5, i, j, nn)[0] for i in range(50) for j in range(3)]
        assert min(ids) >= 0 and max(ids) < nn
    assert all(R.draw(5, i, 0, 2)[0] == (R.draw(5, i, 0, 2 ** 31 - 1)[0] >> 30) for i in range(50))


def test_corrupt_at_is_corrupt_at_those_positions():
    g = torch.Generator().manual_seed(4)
    n, k, n_nodes = 60, 7, 1000
    s, o = (torch.randint(0, n_nodes, (n,), generator=g).numpy() for _ in range(2))
    r = torch.randint(0, 5, (n,), generator=g).numpy()
    full = R.corrupt(s, r, o, n_nodes, k, seed=2 ** 63 - 1)
    pos = np.array([0, 1, 6, 7, 8, 13, 14, 200, n * k - 1, 200])       # both ends, around multiples of k, one position twice
    for a, b in zip(R.corrupt_at(s, r, o, n_nodes, k, 2 ** 63 - 1, pos), full):
        assert np.array_equal(a, b[pos])
    every = R.corrupt_at(s, r, o, n_nodes, k, 2 ** 63 - 1, np.arange(n * k))
    assert all(np.array_equal(a, b) for a, b in zip(every, full))


def test_triple_index_against_buckets():
    """the argsort formulation against plain buckets filled in position order"""
    g = torch.Generator().manual_seed(6)
    n_nodes, n_rel, n = 300, 270, 500
    s, o = (torch.randint(0, n_nodes, (n,), generator=g).numpy() for _ in range(2))
    r = torch.randint(0, n_rel, (n,), generator=g).numpy()
    s[3], o[4], r[5], s[6], r[7] = n_nodes, 2 ** 40, n_rel, -1, -7
    s[8], r[8] = n_nodes + 1, n_rel + 1
    s[9], o[9] = 0, n_nodes - 1
    ix = R.triple_index(s, r, o, n_nodes, n_rel)
    node, rel, bad_slots, bad_triples = [[] for _ in range(n_nodes)], [[] for _ in range(n_rel)], [], []
    for t in range(n):
        if 0 <= s[t] < n_nodes and 0 <= o[t] < n_nodes and 0 <= r[t] < n_rel:
            node[s[t]].append(2 * t)
            node[o[t]].append(2 * t + 1)
            rel[r[t]].append(t)
        else:
            bad_slots += [2 * t, 2 * t + 1]
            bad_triples.append(t)
    assert bad_triples == [3, 4, 5, 6, 7, 8] and ix["bad"] == R.BAD_NODE | R.BAD_REL
    assert ix["node_slot"].tolist() == [x for b in node for x in b] and ix["rel_triple"].tolist() == [x for b in rel for x in b]
    assert ix["node_ptr"].tolist() == np.concatenate([[0], np.cumsum([len(b) for b in node])]).tolist()
    assert ix["rel_ptr"].tolist() == np.concatenate([[0], np.cumsum([len(b) for b in rel])]).tolist()
    assert ix["bad_slots"].tolist() == bad_slots and ix["bad_triples"].tolist() == bad_triples
    assert ix["node_ptr"][-1] == 2 * (n - 6) and ix["rel_ptr"][-1] == n - 6


def test_rank_counts_and_band():
    z = np.array([[1., 0.], [2., 0.], [2., 0.], [3., 0.], [0., 5.]])
    rel = np.array([[1., 1.]])
    sc, cond = R.rank_scores(z, rel, [0, 0], [0, 0])                # scores of query 0: 1 2 2 3 0
    assert np.array_equal(sc[0], [1, 2, 2, 3, 0]) and np.array_equal(cond, np.abs(sc))
    g, e = R.rank_counts(sc, [1, 4])
    assert g.tolist() == [1, 4] and e.tolist() == [1, 0]
    g, e = R.rank_counts(sc, [1, 4], [[2, 3, 99], [0, 1, 2, 3, 4]])
    assert g.tolist() == [0, 0] and e.tolist() == [0, 0]
    lo, hi = R.rank_band(z, rel, [0, 0], [0, 0], [1, 4])
    assert lo.tolist() == [1, 4] and hi.tolist() == [2, 4]          # the exact tie sits inside the band
    m = R.metrics([0, 1, 3], [0, 2, 0])
    assert abs(m["mrr"] - (1 + 1 / 3 + 1 / 4) / 3) < 1e-15 and m["hits@1"] == 1 / 3 and m["hits@3"] == 2 / 3 and m["hits@10"] == 1
