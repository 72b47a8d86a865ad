"""``rgcn_emb_adam_rows`` and ``sparse_optim.RowAdam`` where tests/test_gpu_row_adam.py stops, against the float64
restatement of tests/row_adam_reference.py:
  A  the sort behind ``emb_keys_kernel`` past one 2,048-key wave segment, one workgroup, one scan block and two radix passes;
  B  "added in ascending position order" bit for bit: at beta1 = beta2 = 0 the moments ARE the fp32 sum and its square;
  C  lane groups of 1..64 lanes, whole 16-byte pieces beside a partial one on the vector path, two and three passes, strides and
     bases that differ between the buffers, plane strides that are odd or smaller than a row stride;
  D  preset step counts up to 2^31 - 1, neighbouring units with very different counts, beta = 0, lr = 0;
  E  ids far out of range, more of them than a segment holds, a NULL ``bad_ids``;
  F  ``RowAdam`` on views, int32 and strided ids, expanded gradients, a growing workspace, a side stream.
The tolerance is the project's k (2^-22 max|p| + 2^-18 lr); in D, where preset moments or beta2 = 0 make a step larger than lr, the
second term takes max(lr, max|dp| of the reference) for lr.  Every case prints error / tolerance."""
import numpy as np
import pytest
import torch

from tests.row_adam_cases import B1, B2, EPS, LR, T_LIST, EdgeCase, bits, hub_ids, hyper32, longest_run, uniform_ids, with_bad_ids
from tests.row_adam_reference import order_changes_bits, row_adam_step_vectorised, run_sums, tolerance

pytestmark = pytest.mark.gpu


def _ids(kind, num_nodes, n_rows):
    if kind == "uniform":
        return uniform_ids(num_nodes, n_rows, seed=n_rows)
    if kind == "hub":
        return hub_ids(num_nodes, n_rows)
    return with_bad_ids(num_nodes, n_rows)


# ---- A: the sort past one segment ----------------------------------------------------------------------------------------------
SORT_CASES = [("uniform", 300, 2049, 4), ("uniform", 300, 8193, 4), ("uniform", 300, 16385, 4), ("uniform", 70000, 16385, 4),
              ("hub", 1000, 16385, 4), ("bad", 256, 2049, 4), ("bad", 65536, 2049, 4), ("uniform", 300, 16385, 68)]


@pytest.mark.parametrize("kind,num_nodes,n_rows,width", SORT_CASES, ids=lambda v: str(v))
def test_sort_past_one_segment(kind, num_nodes, n_rows, width):
    ids = _ids(kind, num_nodes, n_rows)
    run = longest_run(ids, num_nodes)
    if kind == "hub":
        at = np.nonzero(ids == 421)[0]
        assert run == len(at) == 5000 and at[0] < 2048 and at[-1] >= 14336      # its positions lie in the first and the last segment
    if kind == "bad":
        assert np.count_nonzero((ids < 0) | (ids >= num_nodes)) == 40 and 0 in ids and num_nodes - 1 in ids
    if num_nodes == 70000:
        assert 1 < run <= 4
    c = EdgeCase(num_nodes, width, wd=0.01, seed=n_rows + width, label=f"A {kind}")
    for _ in range(2):
        c.step(ids, c.grads(n_rows), False, longest=run)


# ---- B: position order, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 68])
@pytest.mark.parametrize("kind,num_nodes", [("uniform", 300), ("hub", 1000)])
def test_position_order_bit_for_bit(kind, num_nodes, width):
    n_rows = 16385
    ids = _ids(kind, num_nodes, n_rows)
    c = EdgeCase(num_nodes, width, hyper=hyper32(beta1=0.0, beta2=0.0, wd=0.0), seed=width, label=f"B {kind}")
    for s in range(2):
        g = c.grads(n_rows)
        g32 = g.numpy()
        many, changed, elements = order_changes_bits(ids, g32, num_nodes)
        print(f"position order {kind} width={width} step {s + 1}: {changed} of {many} repeated ids change their bits in descending "
              f"order ({100 * elements:.0f}% of their elements)")
        assert many > 0 and 2 * changed >= many               # the test can fail
        c.step(ids, g, False, longest=longest_run(ids, num_nodes))
        listed, sums, _ = run_sums(ids, g32, num_nodes, np.float32)
        rows = torch.from_numpy(listed).to(c.dev)
        got_m, got_v = c.m[rows].cpu().numpy(), c.v[rows].cpu().numpy()
        wrong = int((got_m.view(np.uint32) != sums.view(np.uint32)).sum())
        wrong_sq = int((got_v.view(np.uint32) != (sums * sums).view(np.uint32)).sum())
        print(f"position order {kind} width={width} step {s + 1}: exp_avg differs in {wrong} of {sums.size} elements, "
              f"exp_avg_sq in {wrong_sq}")
        assert wrong == 0 and wrong_sq == 0


# ---- C: lane groups, pieces and strides -----------------------------------------------------------------------------------------
SHAPES = [(3, 4, 4), (6, 8, 8), (66, 68, 68), (12, 12, 12), (20, 20, 20), (132, 132, 132), (252, 252, 252), (253, 256, 256),
          (256, 256, 256), (257, 260, 260), (516, 516, 516), (8, 8, 12), (8, 12, 8), (8, 8, 10), (8, 10, 8)]


def _two_steps_of_257(c, unique):
    for s in range(2):
        nodes = torch.randperm(1000, generator=c.gen)[:257].tolist()
        if s == 1:
            nodes[3], nodes[200] = 999, 0                      # the last row and the first
        nodes = list(dict.fromkeys(nodes))
        c.step(nodes, c.grads(len(nodes)), unique)


@pytest.mark.parametrize("unique", [True, False], ids=["unique", "sorted"])
@pytest.mark.parametrize("width,ld,ldg", SHAPES, ids=lambda v: str(v))
def test_groups_pieces_and_strides(width, ld, ldg, unique):
    c = EdgeCase(1000, width, ld, ldg, wd=0.01, seed=width + ld + ldg, label="C")
    assert c.vec() == (ld % 4 == 0 and ldg % 4 == 0)          # (the partial pieces of 3, 6, 66, 253, 257 lie on the vector path)
    _two_steps_of_257(c, unique)


@pytest.mark.parametrize("unique", [True, False], ids=["unique", "sorted"])
@pytest.mark.parametrize("which", ["grad", "exp_avg_sq", "table"])
def test_one_base_4_bytes_off(which, unique):
    c = EdgeCase(1000, 8, off={which: 1}, wd=0.01, seed=3, label=f"C base {which}")
    at = {"table": c.table, "exp_avg": c.m, "exp_avg_sq": c.v, "grad": c.device_grad(c.grads_like(2))}
    assert [name for name, t in at.items() if t.data_ptr() % 16] == [which] and not c.vec()
    _two_steps_of_257(c, unique)


S, NP, EP = 3, 37, 12
PLANES = {"table stride 38*12+2": dict(plane_stride=38 * EP + 2),
          "grad stride odd": dict(grad_plane_stride=21 * EP + 1),
          "table interleaved": dict(ld=S * EP, plane_stride=EP),
          "grad interleaved": dict(ldg=S * EP, grad_plane_stride=EP)}


@pytest.mark.parametrize("unique", [True, False], ids=["unique", "sorted"])
@pytest.mark.parametrize("name", list(PLANES))
def test_plane_strides(name, unique):
    c = EdgeCase(NP, EP, planes=S, wd=0.01, seed=7, label=f"C {name}", **PLANES[name])
    assert c.vec() == ("interleaved" in name)
    if name == "table interleaved":
        assert c.table.stride() == (EP, S * EP, 1) and c.plane_stride < c.ld
    for _ in range(2):
        nodes = torch.randperm(NP, generator=c.gen)[:20].tolist()
        c.step(nodes, c.grads(20), unique)


# ---- D: step counts and hyper-parameter edges -----------------------------------------------------------------------------------
@pytest.mark.parametrize("t", T_LIST)
def test_preset_step(t):
    c = EdgeCase(64, 16, preset_t=np.full(64, t), step_scaled=True, seed=t % 1000, label=f"D t={t}")
    c.step(torch.randperm(64, generator=c.gen).tolist(), c.grads(64), True)
    assert c.row_step.tolist() == [t] * 64


@pytest.mark.parametrize("width,unique", [(12, True), (64, True), (68, True), (12, False)], ids=lambda v: str(v))
def test_mixed_step_counts_in_one_call(width, unique):
    """row i is about to take step T_LIST[i mod 9]: a t handed to the wrong lane group shows as a wrong row"""
    n = 257
    t = np.array([T_LIST[i % 9] for i in range(n)])
    c = EdgeCase(n, width, preset_t=t, step_scaled=True, seed=width, label="D mixed t")
    c.step(torch.randperm(n, generator=c.gen).tolist(), c.grads(n), unique)
    assert np.array_equal(c.row_step.cpu().numpy(), t)


@pytest.mark.parametrize("t", [1, 693])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("betas", [(0.0, 0.999), (0.9, 0.0), (0.0, 0.0)], ids=lambda v: str(v))
def test_zero_betas(betas, wd, t):
    c = EdgeCase(64, 16, hyper=hyper32(beta1=betas[0], beta2=betas[1], wd=wd), preset_t=np.full(64, t), step_scaled=True, seed=t,
                 label=f"D betas={betas} wd={wd} t={t}")
    c.step(torch.randperm(64, generator=c.gen).tolist(), c.grads(64), True)


@pytest.mark.parametrize("beta2", [0.999, 0.9999])
def test_bias_correction_digits_at_small_t(beta2):
    """steps 1..4 from a zero state on a table of |p| ~ 1e-3, so that the tolerance is its second term, 32 ulp of the step
    (3.8e-8 per step), and not the ulp of a p near 4.  1 - beta2^t is about t (1 - beta2): an fp32 ``1 - powf(beta2, t)`` is
    exact at t = 1 (beta2 reaches the kernel as a float) and rounds beta2^t to 3e-8 from t = 2 on, which is 7.5e-6 (7.5e-5 at
    0.9999) of the difference and half as much of the step"""
    c = EdgeCase(64, 16, hyper=hyper32(beta2=beta2), p_scale=1e-3, seed=17, label=f"D beta2={beta2} small p")
    for _ in range(4):
        c.step(torch.randperm(64, generator=c.gen).tolist(), c.grads(64), True)


@pytest.mark.parametrize("t", [1, 693])
def test_zero_lr(t):
    """the table keeps its bits (EdgeCase.step asserts it at lr = 0); the moments and the step counts follow the reference"""
    c = EdgeCase(64, 16, hyper=hyper32(lr=0.0, wd=0.01), preset_t=np.full(64, t), step_scaled=True, seed=t, label=f"D lr=0 t={t}")
    m0 = c.m.clone()
    c.step(torch.randperm(64, generator=c.gen).tolist(), c.grads(64), True)
    assert c.row_step.tolist() == [t] * 64 and not torch.equal(c.m, m0)


# ---- E: ids out of range --------------------------------------------------------------------------------------------------------
EXTREME = [-2 ** 63, -2 ** 31 - 1, -1, 1000, 2 ** 31, 2 ** 32 + 5, 2 ** 63 - 1]


@pytest.mark.parametrize("unique", [True, False], ids=["unique", "sorted"])
def test_extreme_ids(unique):
    """an id truncated to 32 bits would update row 5 (2^32 + 5) and row 0 (-2^63); neither is listed"""
    c = EdgeCase(1000, 8, wd=0.01, seed=9, label="E extreme")
    for _ in range(2):
        valid = [i for i in torch.randperm(1000, generator=c.gen).tolist() if i not in (0, 5)][:9]
        nodes = valid[:2] + EXTREME[:3] + valid[2:6] + EXTREME[3:6] + valid[6:] + EXTREME[6:]
        assert len(nodes) == 16 and 5 not in nodes
        before = bits(c.table[5]).clone()
        c.step(nodes, c.grads(16), unique)                     # (compares the device's count with the reference's)
        assert c.last_bad == 7
        assert torch.equal(bits(c.table[5]), before) and int(c.row_step[5]) == 0 and int(c.row_step[0]) == 0


def test_more_bad_ids_than_a_segment():
    rng = np.random.default_rng(4)
    ids = rng.integers(0, 1000, 5000, dtype=np.int64)
    at = rng.permutation(5000)[:3000]
    ids[at[:1500]], ids[at[1500:]] = -1, 1000
    c = EdgeCase(1000, 8, wd=0.01, seed=10, label="E 3000 bad")
    c.step(ids, c.grads(5000), False, longest=longest_run(ids, 1000))
    assert c.ref[3].sum() == len(np.unique(ids[(ids >= 0) & (ids < 1000)]))


@pytest.mark.parametrize("unique", [True, False], ids=["unique", "sorted"])
def test_every_id_bad(unique):
    """100 positions, none valid (distinct values: ``assume_unique`` promises no duplicates): nothing changes, the count is 100"""
    ids = np.concatenate([-1 - np.arange(50, dtype=np.int64), 1000 + np.arange(50, dtype=np.int64)])
    c = EdgeCase(1000, 8, wd=0.01, seed=11, label="E all bad")
    whole = [bits(b).clone() for b in (*c.bufs.values(), c.step_buf)]
    c.step(ids, c.grads(100), unique)
    assert all(torch.equal(bits(b), w) for b, w in zip((*c.bufs.values(), c.step_buf), whole))


@pytest.mark.parametrize("unique", [True, False], ids=["unique", "sorted"])
def test_null_bad_ids(unique):
    c = EdgeCase(1000, 8, wd=0.01, seed=12, label="E NULL bad_ids")
    valid = torch.randperm(1000, generator=c.gen)[:9].tolist()
    nodes = valid[:4] + [-1, 1000] + valid[4:] + [2 ** 40]
    c.step(nodes, c.grads(len(nodes)), unique, bad_ids=None)
    assert c.ref[3].sum() == 9


# ---- F: sparse_optim.RowAdam ----------------------------------------------------------------------------------------------------
def _row_adam_pair(table, wd=0.01):
    """(RowAdam on ``table``, RowAdam on a contiguous copy, the float64 state)"""
    from scaling_rgcn_training_amd.sparse_optim import RowAdam
    twin = table.detach().clone().contiguous()
    ref = [table.detach().cpu().double().numpy().copy(), np.zeros(tuple(table.shape)), np.zeros(tuple(table.shape)),
           np.zeros(table.shape[-2], dtype=np.int64)]
    return RowAdam(table, LR, (B1, B2), EPS, wd), RowAdam(twin, LR, (B1, B2), EPS, wd), ref


def _row_adam_check(a, b, ref, k, label, longest=1):
    torch.cuda.synchronize()
    a.check()
    if b is not None:
        for name in ("table", "exp_avg", "exp_avg_sq", "row_step"):
            assert torch.equal(bits(getattr(a, name).detach()), bits(getattr(b, name).detach())), (label, name)
    err = np.abs(a.table.detach().cpu().double().numpy() - ref[0]).max()
    tol = tolerance(k, np.abs(ref[0]).max(), LR)
    print(f"RowAdam {label} step {k}: max error {err:.3e}, tolerance {tol:.3e}, ratio {err / tol:.3f}")
    assert err <= tol
    for i, scale in ((1, longest + 3), (2, 2 * longest + 5)):
        got = (a.exp_avg, a.exp_avg_sq)[i - 1].cpu().double().numpy()
        assert np.abs(got - ref[i]).max() <= k * scale * 2.0 ** -23 * max(np.abs(ref[i]).max(), 1e-30)
    assert np.array_equal(a.row_step.cpu().numpy(), ref[3])


def _dup_nodes(n_nodes, n, gen):
    """n positions over n // 2 ids: every id twice, scattered"""
    ids = torch.randperm(n_nodes, generator=gen)[:n // 2]
    return torch.cat([ids, ids])[torch.randperm(n, generator=gen)]


@pytest.mark.parametrize("view", ["columns", "interleaved"])
def test_row_adam_on_a_view_of_the_table(view):
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(21)
    n_nodes, e = 50, 12
    if view == "columns":
        big = torch.randn(n_nodes, e + 8, generator=gen).to(dev)
        table = big[:, :e]
        outside = torch.ones_like(big, dtype=torch.bool)
        outside[:, :e] = False
    else:
        big = torch.randn(n_nodes, 3, e, generator=gen).to(dev)
        table = big.permute(1, 0, 2)
        assert table.stride() == (e, 3 * e, 1)
        outside = torch.zeros_like(big, dtype=torch.bool)
    big0 = big.clone()
    a, b, ref = _row_adam_pair(table)
    assert a.exp_avg.stride() == table.stride() and a.exp_avg_sq.stride() == table.stride()
    listed = torch.zeros(n_nodes, dtype=torch.bool)
    for k in range(1, 3):
        nodes = _dup_nodes(n_nodes, 20, gen)
        g = torch.randn(*table.shape[:-2], 20, e, generator=gen)
        for opt in (a, b):
            opt.step(nodes.to(dev), g.to(dev), assume_unique=False)
        row_adam_step_vectorised(*ref, nodes.numpy(), g.double().numpy(), hyper32(wd=0.01))
        _row_adam_check(a, b, ref, k, f"view {view}", longest=2)
        listed[nodes] = True
    assert torch.equal(bits(big)[outside], bits(big0)[outside])
    rest = (~listed).to(dev)
    assert torch.equal(bits(table[..., rest, :]), bits((big0[:, :e] if view == "columns" else big0.permute(1, 0, 2))[..., rest, :]))


@pytest.mark.parametrize("kind", ["int32", "strided"])
def test_row_adam_node_lists(kind):
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(22)
    table = torch.randn(50, 12, generator=gen).to(dev)
    a, b, ref = _row_adam_pair(table)
    for k in range(1, 3):
        ids = _dup_nodes(50, 40, gen).to(dev)
        nodes = ids[:20].to(torch.int32) if kind == "int32" else ids[::2]
        assert kind == "int32" or nodes.stride(0) == 2
        g = torch.randn(20, 12, generator=gen)
        a.step(nodes, g.to(dev))
        b.step(nodes.long().contiguous(), g.to(dev))
        row_adam_step_vectorised(*ref, nodes.cpu().numpy(), g.double().numpy(), hyper32(wd=0.01))
        _row_adam_check(a, b, ref, k, f"nodes {kind}", longest=2)


def _autograd_gradient(n, e, w, how):
    """a gradient whose every row is w.  "leaf": ``.grad`` of the leaf of (rows * w[None, :]).sum(), which the accumulation
    into ``.grad`` hands over as a tensor of its own; "row sum": ``torch.autograd.grad`` of (rows.sum(0) * w).sum(), where the
    backward of the row sum expands w over the rows and nothing copies it -- strides (0, 1)"""
    rows = torch.zeros(n, e, device=w.device, requires_grad=True)
    if how == "leaf":
        (rows * w[None, :]).sum().backward()
        return rows.grad
    return torch.autograd.grad((rows.sum(0) * w).sum(), rows)[0]


@pytest.mark.parametrize("kind", ["last dimension strided", "expanded", "autograd leaf", "autograd row sum"])
@pytest.mark.parametrize("unique", [True, False], ids=["unique", "sorted"])
def test_row_adam_gradient_layouts(kind, unique):
    """a gradient whose rows overlap (row stride 0) has to be copied before the call: the C ABI refuses ``ldg < width``"""
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(23)
    n, e = 20, 12
    table = torch.randn(50, e, generator=gen).to(dev)
    a, b, ref = _row_adam_pair(table)
    w = torch.randn(e, generator=gen).to(dev)
    for k in range(1, 3):
        nodes = torch.randperm(50, generator=gen)[:n] if unique else _dup_nodes(50, n, gen)
        if kind == "last dimension strided":
            g = torch.randn(n, 2 * e, generator=gen).to(dev)[:, ::2]
            assert g.stride() == (2 * e, 2)
        elif kind == "expanded":
            g = w.expand(n, e)
            assert g.stride() == (0, 1)
        else:
            g = _autograd_gradient(n, e, w, kind[9:])
            assert torch.equal(g, w.expand(n, e))
            print(f"RowAdam: {kind} hands back strides {g.stride()}")
        a.step(nodes.to(dev), g, assume_unique=unique)
        b.step(nodes.to(dev), g.contiguous(), assume_unique=unique)
        row_adam_step_vectorised(*ref, nodes.numpy(), g.cpu().double().numpy(), hyper32(wd=0.01))
        _row_adam_check(a, b, ref, k, f"grad {kind}", longest=2)


def test_row_adam_workspace_grows_once():
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(24)
    table = torch.randn(1000, 8, generator=gen).to(dev)
    a, _, ref = _row_adam_pair(table)
    seen = []
    for k, n in enumerate((4, 5000, 4), 1):
        nodes = torch.randint(0, 1000, (n,), generator=gen)
        g = torch.randn(n, 8, generator=gen)
        a.step(nodes.to(dev), g.to(dev))
        row_adam_step_vectorised(*ref, nodes.numpy(), g.double().numpy(), hyper32(wd=0.01))
        _row_adam_check(a, None, ref, k, f"workspace n={n}", longest=longest_run(nodes.numpy(), 1000))
        seen.append(a._workspace)
    assert seen[1] is not seen[0] and seen[1].numel() > seen[0].numel() and seen[2] is seen[1]


def test_row_adam_on_a_side_stream():
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(25)
    table = torch.randn(1000, 64, generator=gen).to(dev)
    a, b, ref = _row_adam_pair(table)
    nodes = torch.randint(0, 1000, (300,), generator=gen)
    g = torch.randn(300, 64, generator=gen)
    nodes_d, g_d = nodes.to(dev), g.to(dev)
    b.step(nodes_d, g_d)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        a.step(nodes_d, g_d)
    side.synchronize()
    row_adam_step_vectorised(*ref, nodes.numpy(), g.double().numpy(), hyper32(wd=0.01))
    _row_adam_check(a, b, ref, 1, "side stream", longest=longest_run(nodes.numpy(), 1000))
