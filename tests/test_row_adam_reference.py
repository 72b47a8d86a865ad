"""tests/row_adam_reference.py against ``torch.optim.Adam`` in float64 on the CPU: with every row listed once per step the
row-wise step IS the dense optimizer; a duplicated id is the step on the pre-summed rows; rows that are not listed do not change."""
import numpy as np
import pytest
import torch

from tests.row_adam_cases import hub_ids, longest_run, uniform_ids, with_bad_ids
from tests.row_adam_reference import order_changes_bits, row_adam_step, row_adam_step_vectorised, run_sums

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


@pytest.mark.parametrize("shape", [(40, E), (3, 40, E)], ids=["table", "planes"])
def test_vectorised_twin_is_the_loop(shape):
    """duplicates (runs of up to 30), ids out of range, planes, weight decay, preset moments and step counts, three steps: the
    same state to 1e-12, the same return value"""
    rng = np.random.default_rng(3)
    n_nodes = shape[-2]
    start = [rng.standard_normal(shape), 0.3 * rng.standard_normal(shape), rng.random(shape), rng.integers(0, 700, n_nodes)]
    a, b = [x.copy() for x in start], [x.copy() for x in start]
    for k in range(3):
        nodes = rng.integers(0, n_nodes - 5, 200)              # the last five rows are never listed
        nodes[rng.permutation(200)[:30]] = 7
        nodes[rng.permutation(200)[:12]] = np.array([-1, n_nodes, 2 ** 32 + 5, -2 ** 63] * 3)
        g = rng.standard_normal(shape[:-2] + (200, E))
        bad = row_adam_step(*a, nodes, g, _hyper(0.01))
        assert row_adam_step_vectorised(*b, nodes, g, _hyper(0.01)) == bad == 12
        for x, y, name in zip(a, b, ("table", "exp_avg", "exp_avg_sq")):
            assert np.abs(x - y).max() <= 1e-12, (name, k)
        assert np.array_equal(a[3], b[3])
    for x, y, z in zip(a, b, start):
        assert np.array_equal(x[..., -5:, :] if x.ndim > 1 else x[-5:], z[..., -5:, :] if z.ndim > 1 else z[-5:])
        assert np.array_equal(y[..., -5:, :] if y.ndim > 1 else y[-5:], z[..., -5:, :] if z.ndim > 1 else z[-5:])
    assert row_adam_step_vectorised(*b, [-1, n_nodes], np.zeros(shape[:-2] + (2, E)), _hyper(0.01)) == 2       # no valid id at all


def test_run_sums_follow_the_position_order():
    """fp32, one id at positions 0, 2, 3: ascending is ((a + b) + c), descending ((c + b) + a)"""
    a, b, c = np.float32(1.0), np.float32(2.0 ** -24), np.float32(2.0 ** -24)
    g = np.array([[a], [5.0], [b], [c]], dtype=np.float32)
    ids, up, counts = run_sums([4, 1, 4, 4], g, 9, np.float32)
    _, down, _ = run_sums([4, 1, 4, 4], g, 9, np.float32, descending=True)
    assert ids.tolist() == [1, 4] and counts.tolist() == [1, 3]
    assert up[1, 0] == np.float32(1.0) and down[1, 0] == np.float32(1.0 + 2.0 ** -23) and up[0, 0] == down[0, 0] == 5.0
    assert order_changes_bits([4, 1, 4, 4], g, 9) == (1, 1, 1.0)


@pytest.mark.parametrize("width", [4, 68])
@pytest.mark.parametrize("kind", ["uniform", "hub"])
def test_position_order_is_visible_in_fp32(kind, width):
    """the precondition of tests/test_gpu_row_adam_edges.py::test_position_order_bit_for_bit on its id lists: adding an id's rows
    in descending position order changes the bits of at least half of the ids listed more than once"""
    num_nodes = 300 if kind == "uniform" else 1000
    ids = uniform_ids(num_nodes, 16385, seed=16385) if kind == "uniform" else hub_ids(num_nodes, 16385)
    g = torch.randn(16385, width, generator=torch.Generator().manual_seed(width)).numpy()
    many, changed, elements = order_changes_bits(ids, g, num_nodes)
    print(f"{kind} width={width}: {changed} of {many} repeated ids change, {100 * elements:.0f}% of their elements")
    assert many > num_nodes // 2 and 2 * changed >= many


def test_id_lists_are_what_the_gpu_tests_say():
    hub = hub_ids(1000, 16385)
    at = np.nonzero(hub == 421)[0]
    assert longest_run(hub, 1000) == len(at) == 5000 and at[0] < 2048 and at[-1] >= 14336
    assert 1 < longest_run(uniform_ids(70000, 16385, seed=16385), 70000) <= 4
    for n in (256, 65536):
        ids = with_bad_ids(n, 2049)
        assert np.count_nonzero(ids == -1) == 20 and np.count_nonzero(ids == n) == 20 and 0 in ids and n - 1 in ids
        assert longest_run(ids, n) >= 1
