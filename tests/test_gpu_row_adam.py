"""``rgcn_emb_adam_rows`` (csrc/rgcn_emb_rows.hip) and ``sparse_optim.RowAdam`` against the float64 restatement of
tests/row_adam_reference.py, on the smallest shapes that reach each code path: the scalar path (widths 1 and 3, a stride or a base
that is not 16-byte aligned), exactly one 16-byte piece (4), 16 lanes per row (64), a number of rows per wave that is no power of
two (68: 17 lanes, 3 rows), several passes (260), a padded stride (64 in 72), planes, duplicated ids through the sort, ids out of
range.  Every case runs 3 steps with p, g ~ N(0, 1) and lr = 0.01 and is compared after EACH step k with the tolerance
k (2^-22 max|p| + 2^-18 lr) per element; rows that are not listed, the pad columns behind ``width`` and a pad row behind the last
one must keep their bits in the table, both moments and the step counts."""
import numpy as np
import pytest
import torch

from tests.row_adam_reference import row_adam_step, tolerance

pytestmark = pytest.mark.gpu

SENT = 777.0
LR, B1, B2, EPS = 0.01, 0.9, 0.999, 1e-8


def _hyper(wd, beta2=B2):
    """what the kernel is given: the C ABI takes floats, so the reference starts from the same fp32-rounded values (1 - beta2
    differs by 1.3e-5 of itself between 0.999 and its fp32 rounding: visible in exp_avg_sq, not in p)"""
    h = {"lr": LR, "beta1": B1, "beta2": beta2, "eps": EPS, "weight_decay": wd}
    return {k: float(np.float32(v)) for k, v in h.items()}


def _padded(planes, rows, width, ld, dev, off=0, dtype=torch.float32):
    """(buffer, pad mask, view): a [planes, rows, width] view (2-D when planes == 0) of row stride ld in a buffer of sentinels --
    the pad columns, one pad row behind every plane and ``off`` elements in front are what the mask marks"""
    p = max(planes, 1)
    buf = torch.full((off + p * (rows + 1) * ld,), SENT, device=dev, dtype=dtype)
    pad = torch.ones_like(buf, dtype=torch.bool)
    cut = lambda b: b[off:].view(p, rows + 1, ld)[:, :rows, :width]
    cut(pad).fill_(False)
    view = cut(buf)
    return buf, pad, (view if planes else view[0])


class Case:
    """device state in sentinel buffers + the float64 twin; ``step`` runs both and compares"""

    def __init__(self, n_nodes, width, ld=None, planes=0, wd=0.0, beta2=B2, off=0, seed=0):
        from scaling_rgcn_training_amd import _lib
        self.lib, self.dev = _lib, torch.device("cuda:0")
        self.n, self.width, self.ld, self.planes, self.off = n_nodes, width, ld or width, planes, off
        self.hyper = _hyper(wd, beta2)
        self.gen = torch.Generator().manual_seed(seed)
        shape = (planes, n_nodes, width) if planes else (n_nodes, width)
        p0 = torch.randn(shape, generator=self.gen)
        self.bufs = {}
        for name in ("table", "exp_avg", "exp_avg_sq"):
            self.bufs[name] = _padded(planes, n_nodes, width, self.ld, self.dev, off)
        self.table, self.m, self.v = (self.bufs[k][2] for k in ("table", "exp_avg", "exp_avg_sq"))
        self.table.copy_(p0)
        self.m.zero_()
        self.v.zero_()
        self.step_buf = torch.full((n_nodes + 1,), 12345, dtype=torch.int32, device=self.dev)
        self.row_step = self.step_buf[:n_nodes]
        self.row_step.zero_()
        self.bad = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.ref = [p0.double().numpy().copy(), np.zeros(shape), np.zeros(shape), np.zeros(n_nodes, dtype=np.int64)]
        self.k = 0
        self.worst = 0.0

    def grads(self, n, zero=False):
        shape = (self.planes, n, self.width) if self.planes else (n, self.width)
        return torch.zeros(shape) if zero else torch.randn(shape, generator=self.gen)

    def device_grad(self, g):
        n = g.shape[-2]
        _, _, view = _padded(self.planes, max(n, 1), self.width, self.ld, self.dev, self.off)
        view = view[..., :n, :]
        view.copy_(g)
        return view

    def snapshot(self):
        return [t.clone() for t in (self.table, self.m, self.v, self.row_step)]

    def step(self, nodes, g, unique, longest_run=1):
        nodes_t = torch.as_tensor(nodes, dtype=torch.int64)
        before = self.snapshot()
        self.lib.emb_adam_rows(self.table, self.m, self.v, self.row_step, nodes_t.to(self.dev), self.device_grad(g), LR, B1,
                               self.hyper["beta2"], EPS, self.hyper["weight_decay"], unique, self.bad)
        torch.cuda.synchronize()
        bad = row_adam_step(*self.ref, nodes_t.numpy(), g.double().numpy(), self.hyper)
        self.k += 1
        assert int(self.bad.item()) == bad
        self.bad.zero_()
        # listed rows against the reference
        got = [t.cpu().double().numpy() for t in (self.table, self.m, self.v)]
        tol = tolerance(self.k, np.abs(self.ref[0]).max(), LR)
        err = np.abs(got[0] - self.ref[0]).max()
        self.worst = max(self.worst, err / tol)
        print(f"row_adam n={self.n} width={self.width} ld={self.ld} planes={self.planes} rows={len(nodes)} unique={unique} "
              f"step {self.k}: max error {err:.3e}, tolerance {tol:.3e}, ratio {err / tol:.3f}")
        assert err <= tol, (err, tol)
        # the moments: every step rounds the gradient sum (one rounding per added row) and the two updates a few times
        for i, scale in ((1, longest_run + 3), (2, 2 * longest_run + 5)):
            bound = self.k * scale * 2.0 ** -23 * max(np.abs(self.ref[i]).max(), 1e-30)
            assert np.abs(got[i] - self.ref[i]).max() <= bound, ("exp_avg" if i == 1 else "exp_avg_sq", self.k)
        assert np.array_equal(self.row_step.cpu().numpy(), self.ref[3])
        # rows that are not listed keep their bits; so do the pads
        listed = torch.zeros(self.n, dtype=torch.bool)
        listed[nodes_t[(nodes_t >= 0) & (nodes_t < self.n)]] = True
        rest = (~listed).to(self.dev)
        for now, was in zip(self.snapshot(), before):
            assert torch.equal(now[..., rest, :] if now.dim() > 1 else now[rest], was[..., rest, :] if was.dim() > 1 else was[rest])
        for name, (buf, pad, _) in self.bufs.items():
            assert bool((buf[pad] == SENT).all()), f"{name}: a pad element was written"
        assert int(self.step_buf[self.n]) == 12345


def _distinct(n_nodes, n, gen):
    return torch.randperm(n_nodes, generator=gen)[:n].tolist()


WIDTHS = [(1, 1), (3, 3), (4, 4), (64, 64), (68, 68), (260, 260), (64, 72), (6, 6), (8, 10)]


@pytest.mark.parametrize("unique", [True, False], ids=["unique", "sorted"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("width,ld", WIDTHS, ids=lambda v: str(v))
def test_widths(width, ld, wd, unique):
    c = Case(1000, width, ld, wd=wd, seed=width)
    for s in range(3):
        nodes = _distinct(1000, 257, c.gen)
        if s == 1:
            nodes[3], nodes[200] = 999, 0            # the last row and the first
        nodes = list(dict.fromkeys(nodes))
        c.step(nodes, c.grads(len(nodes)), unique)


@pytest.mark.parametrize("unique", [True, False], ids=["unique", "sorted"])
@pytest.mark.parametrize("n_rows", [0, 1, 5, 257])
def test_row_counts(n_rows, unique):
    c = Case(1000, 64, wd=0.01, seed=n_rows)
    for _ in range(3):
        c.step(_distinct(1000, n_rows, c.gen), c.grads(n_rows), unique)


def test_base_not_16_byte_aligned():
    c = Case(50, 8, off=1, wd=0.01)
    assert c.table.data_ptr() % 16 == 4
    for _ in range(3):
        c.step(_distinct(50, 20, c.gen), c.grads(20), True)


@pytest.mark.parametrize("unique", [True, False], ids=["unique", "sorted"])
@pytest.mark.parametrize("width", [12, 5])
def test_planes(width, unique):
    c = Case(37, width, planes=3, wd=0.01, seed=width)
    for _ in range(3):
        c.step(_distinct(37, 20, c.gen), c.grads(20), unique)


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_one_id_at_every_position(wd):
    """300 positions, one run: longer than a wave's worth of units"""
    c = Case(1000, 64, wd=wd, seed=3)
    for node in (17, 999, 17):
        c.step([node] * 300, c.grads(300), False, longest_run=300)


@pytest.mark.parametrize("width,planes", [(64, 0), (7, 0), (12, 3)])
def test_runs_of_one_to_five(width, planes):
    c = Case(1000 if not planes else 37, width, planes=planes, wd=0.01, seed=5)
    for _ in range(3):
        ids = _distinct(c.n, 30, c.gen)
        nodes = [i for j, i in enumerate(ids) for _r in range(1 + j % 5)]
        order = torch.randperm(len(nodes), generator=c.gen).tolist()
        nodes = [nodes[i] for i in order]              # the runs scattered over the positions
        c.step(nodes, c.grads(len(nodes)), False, longest_run=5)


def test_two_calls_on_identical_inputs_are_bit_identical():
    outs = []
    for _ in range(2):
        c = Case(1000, 68, wd=0.01, seed=11)
        ids = _distinct(1000, 60, c.gen)
        nodes = [i for j, i in enumerate(ids) for _r in range(1 + j % 5)] + [ids[0]] * 120
        for _s in range(3):
            c.step(nodes, c.grads(len(nodes)), False, longest_run=121)
        outs.append(c.snapshot())
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("unique", [True, False], ids=["unique", "sorted"])
def test_zero_gradient_rows_do_not_move_without_weight_decay(unique):
    """m = v = 0 and g = 0 give 0 / (0 + eps): the update is exactly 0, the step count still advances"""
    c = Case(1000, 64, wd=0.0, seed=7)
    nodes = _distinct(1000, 40, c.gen)
    p0 = c.table.clone()
    for _ in range(3):
        c.step(nodes, c.grads(40, zero=True), unique)
    assert torch.equal(c.table, p0) and not bool(c.m.any()) and not bool(c.v.any())
    assert c.row_step[nodes].tolist() == [3] * 40 and int(c.row_step.sum()) == 120


@pytest.mark.parametrize("unique", [True, False], ids=["unique", "sorted"])
def test_ids_out_of_range(unique):
    """-1 and N among valid ids: the valid rows match the reference, nothing else changes (Case.step), the count is 2"""
    c = Case(1000, 64, wd=0.01, seed=9)
    for _ in range(3):
        nodes = _distinct(1000, 9, c.gen)
        nodes[2:2] = [-1]
        nodes[7:7] = [1000]
        c.step(nodes, c.grads(len(nodes)), unique)


def test_first_step_bias_correction():
    """t = 1 at beta2 = 0.999: 1 - beta2^t = 1e-3 must keep its digits (a plain fp32 1 - powf loses four)"""
    c = Case(64, 16, wd=0.0, seed=13)
    c.step(list(range(64)), c.grads(64), True)
    assert c.k == 1


# ---- sparse_optim.RowAdam ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("shape", [(50, 20), (3, 37, 12)], ids=["table", "planes"])
def test_every_row_listed_is_torch_adam(shape, wd):
    from scaling_rgcn_training_amd.sparse_optim import RowAdam
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1)
    p0 = torch.randn(shape, generator=gen)
    n = shape[-2]
    dense = torch.nn.Parameter(p0.clone().to(dev))
    opt = torch.optim.Adam([dense], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd)
    table = torch.nn.Parameter(p0.clone().to(dev))
    rows = RowAdam(table, LR, (B1, B2), EPS, wd)
    for k in range(1, 4):
        g = torch.randn(shape, generator=gen).to(dev)
        dense.grad = g.clone()
        opt.step()
        order = torch.randperm(n, generator=gen).to(dev)
        rows.step(order, g[..., order, :], assume_unique=(k != 2))
        err = float((table.detach() - dense.detach()).abs().max())
        tol = tolerance(k, float(dense.detach().abs().max()), LR)
        print(f"RowAdam vs torch.optim.Adam {shape} wd={wd} step {k}: max error {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol
    rows.check()
    assert rows.row_step.tolist() == [3] * n


def test_row_adam_check_state_dict_and_cpu():
    from scaling_rgcn_training_amd.sparse_optim import RowAdam
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(2)
    p0 = torch.randn(30, 8, generator=gen).to(dev)
    a = RowAdam(p0.clone(), LR, weight_decay=0.01)
    assert a.exp_avg.shape == (30, 8) and a.row_step.dtype == torch.int32 and a.bad_ids.shape == (1,)
    nodes = torch.tensor([4, 9, 4, 29], device=dev)
    g = torch.randn(4, 8, generator=gen).to(dev)
    a.step(nodes, g)
    a.check()
    ws = a._workspace
    a.step(nodes[:2], g[:2])
    assert a._workspace is ws                      # cached, grow-only
    state = a.state_dict()
    b = RowAdam(a.table.clone(), 0.5)
    b.load_state_dict(state)
    assert (b.lr, b.betas, b.eps, b.weight_decay) == (a.lr, a.betas, a.eps, a.weight_decay)
    a.step(nodes, g)
    b.step(nodes, g)
    for name in ("table", "exp_avg", "exp_avg_sq", "row_step"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.row_step[[4, 9, 29]].tolist() == [3, 3, 2] and int(a.row_step.sum()) == 8      # (4, 9, 4, 29), (4, 9), (4, 9, 4, 29)
    before = a.table.clone()
    a.step(torch.tensor([-1, 30], device=dev), g[:2], assume_unique=True)
    with pytest.raises(IndexError, match="2 listed node id"):
        a.check()
    a.check()                                      # the count was reset
    assert torch.equal(a.table, before)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RowAdam(torch.zeros(4, 4), LR)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        a.step(torch.tensor([1]), g[:1])
