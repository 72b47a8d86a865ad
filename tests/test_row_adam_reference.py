"""tests/row_adam_reference.py against ``torch.optim.Adam`` in float64 on the CPU: with every row listed once per step the
row-wise step IS the dense optimizer; a duplicated id is the step on the pre-summed rows; rows that are not listed do not change."""
import numpy as np
import pytest
import torch

from tests.row_adam_reference import row_adam_step

N, E = 9, 5


def _hyper(wd):
    return {"lr": 0.01, "beta1": 0.9, "beta2": 0.999, "eps": 1e-8, "weight_decay": wd}


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("shape", [(N, E), (3, N, E)], ids=["table", "planes"])
def test_every_row_listed_is_dense_adam(wd, shape):
    rng = np.random.default_rng(0)
    p0 = rng.standard_normal(shape)
    table, m, v, step = p0.copy(), np.zeros(shape), np.zeros(shape), np.zeros(N, dtype=np.int64)
    param = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([param], lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    for k in range(4):
        g = rng.standard_normal(shape)
        order = rng.permutation(N)                  # any order of the positions: every row is listed once
        assert row_adam_step(table, m, v, step, order, g[..., order, :], _hyper(wd)) == 0
        param.grad = torch.from_numpy(g.copy())
        opt.step()
        assert np.abs(table - param.detach().numpy()).max() <= 1e-12, k
    assert step.tolist() == [4] * N


def test_duplicate_is_the_presummed_row():
    rng = np.random.default_rng(1)
    p0 = rng.standard_normal((N, E))
    g = rng.standard_normal((4, E))
    a = [p0.copy(), np.zeros((N, E)), np.zeros((N, E)), np.zeros(N, dtype=np.int64)]
    b = [p0.copy(), np.zeros((N, E)), np.zeros((N, E)), np.zeros(N, dtype=np.int64)]
    row_adam_step(*a, [2, 7, 2, 4], g, _hyper(0.01))
    row_adam_step(*b, [2, 7, 4], np.stack([g[0] + g[2], g[1], g[3]]), _hyper(0.01))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert a[3].tolist() == [0, 0, 1, 0, 1, 0, 0, 1, 0]


def test_unlisted_rows_and_bad_ids():
    rng = np.random.default_rng(2)
    p0 = rng.standard_normal((N, E))
    m0, v0 = rng.standard_normal((N, E)), rng.random((N, E))
    table, m, v, step = p0.copy(), m0.copy(), v0.copy(), np.arange(N, dtype=np.int64)
    bad = row_adam_step(table, m, v, step, [3, -1, N, 5], rng.standard_normal((4, E)), _hyper(0.01))
    assert bad == 2
    rest = [i for i in range(N) if i not in (3, 5)]
    for now, before in ((table, p0), (m, m0), (v, v0)):
        assert np.array_equal(now[rest], before[rest])          # bit-identical
        assert not np.array_equal(now[[3, 5]], before[[3, 5]])
    assert step.tolist() == [0, 1, 2, 4, 4, 6, 6, 7, 8]
