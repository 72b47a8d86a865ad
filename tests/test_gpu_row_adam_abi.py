"""The C ABI of ``rgcn_emb_adam_rows`` (include/rgcn_mi355x.h, csrc/rgcn_emb_rows.hip): every refusal through raw ctypes with host
dummy pointers -- all of them are answered before the device is looked at, nothing is launched -- the ABI version, the workspace
query, and one update past 2^31 elements (row offsets are 64-bit)."""
import ctypes

import numpy as np
import pytest
import torch

from tests.row_adam_reference import row_adam_step, tolerance

pytestmark = pytest.mark.gpu

OK, NULL, PLAN, WORKSPACE, ARG = 0, -1, -4, -6, -11
_DUMMY = (ctypes.c_int32 * 64)()


def _call(**kw):
    from scaling_rgcn_training_amd import _lib
    d = ctypes.addressof(_DUMMY)
    a = dict(table=d, exp_avg=d, exp_avg_sq=d, row_step=d, planes=1, plane_stride=0, num_nodes=100, width=8, ld=8, nodes=d, n_rows=4,
             grad=d, grad_plane_stride=0, ldg=8, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, assume_unique=0,
             bad_ids=None, workspace=d, workspace_bytes=0, stream=None)
    assert set(kw) <= set(a), kw
    a.update(kw)
    return _lib.load().rgcn_emb_adam_rows(*a.values())


def test_abi_version_is_unchanged():
    from scaling_rgcn_training_amd import _lib
    assert _lib.load().rgcn_abi_version() == 19 and _lib.ABI_VERSION == 19


def test_refusals_before_any_launch():
    # as given the call stops at the last check before the device: a workspace of 0 bytes
    assert _call() == WORKSPACE
    for name in ("table", "exp_avg", "exp_avg_sq", "row_step", "nodes", "grad"):
        assert _call(**{name: None}) == NULL, name
    assert _call(bad_ids=None) == WORKSPACE                      # bad_ids may be NULL
    for kw in (dict(width=0), dict(width=-1), dict(width=9), dict(width=8, ld=12, ldg=7), dict(planes=0), dict(planes=-2),
               dict(n_rows=-1), dict(num_nodes=-1), dict(plane_stride=-8), dict(grad_plane_stride=-8),
               dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=1.5), dict(beta2=float("nan")),
               dict(eps=0.0), dict(eps=-1e-8), dict(lr=-0.01), dict(weight_decay=-0.01)):
        assert _call(**kw) == ARG, kw
    for kw in (dict(beta1=0.0, beta2=0.0), dict(lr=0.0), dict(width=8, ld=12, ldg=8), dict(planes=3, plane_stride=800)):
        assert _call(**kw) == WORKSPACE, kw                      # inside the domain
    assert _call(n_rows=0xFFFF0001) == PLAN
    # no row: nothing to launch, whatever the workspace, and no list to read
    assert _call(n_rows=0, workspace=None) == OK
    assert _call(n_rows=0, nodes=None, grad=None, assume_unique=1) == OK


def test_workspace_one_byte_short_is_refused():
    from scaling_rgcn_training_amd import _lib
    lib = _lib.load()
    need = lib.rgcn_emb_adam_rows_workspace_bytes(300, 1000)
    assert need > 300 * 24
    assert _call(n_rows=300, num_nodes=1000, workspace_bytes=need - 1) == WORKSPACE
    assert _call(n_rows=300, num_nodes=1000, workspace=None, workspace_bytes=need) == NULL
    # the query: 0 on arguments the call refuses (and for no rows); it grows with the rows
    assert lib.rgcn_emb_adam_rows_workspace_bytes(-1, 1000) == 0 and lib.rgcn_emb_adam_rows_workspace_bytes(300, -1) == 0
    assert lib.rgcn_emb_adam_rows_workspace_bytes(0xFFFF0001, 1000) == 0 and lib.rgcn_emb_adam_rows_workspace_bytes(0, 1000) == 0
    assert lib.rgcn_emb_adam_rows_workspace_bytes(5000, 1000) > need


@pytest.mark.parametrize("unique", [True, False], ids=["unique", "sorted"])
def test_rows_past_2_31_elements(unique):
    """width 4, N = 2^29 + 8: the last row starts at element 2^31 + 28.  Three buffers of 8 GiB from ``torch.empty``; only the
    three touched rows are initialised and only they are compared."""
    from scaling_rgcn_training_amd import _lib
    dev = torch.device("cuda:0")
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 30 * 2 ** 30:
        pytest.skip("needs 30 GiB of free device memory")
    n = 2 ** 29 + 8
    rows = [5, 2 ** 29 - 1, n - 1]
    gen = torch.Generator().manual_seed(0)
    p0, g = torch.randn(3, 4, generator=gen), torch.randn(3, 4, generator=gen)
    idx = torch.tensor(rows, device=dev)
    table, m, v = (torch.empty(n, 4, device=dev) for _ in range(3))
    step = torch.empty(n, dtype=torch.int32, device=dev)
    table[idx], m[idx], v[idx], step[idx] = p0.to(dev), 0.0, 0.0, 0
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    hyper = {k: float(np.float32(x)) for k, x in dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01).items()}
    _lib.emb_adam_rows(table, m, v, step, idx, g.to(dev), 0.01, 0.9, 0.999, 1e-8, 0.01, unique, bad)
    torch.cuda.synchronize()
    got = [t[idx].cpu().double().numpy() for t in (table, m, v)]
    got_step, got_bad = step[idx].tolist(), int(bad.item())
    del table, m, v, step
    torch.cuda.empty_cache()                       # (hand the 26 GiB back: later tests measure what is free)
    ref = [p0.double().numpy().copy(), np.zeros((3, 4)), np.zeros((3, 4))]      # the three rows as a table of their own
    assert row_adam_step(ref[0], ref[1], ref[2], np.zeros(3, dtype=np.int64), [0, 1, 2], g.double().numpy(), hyper) == 0
    assert got_bad == 0 and got_step == [1, 1, 1]
    err = np.abs(got[0] - ref[0]).max()
    tol = tolerance(1, np.abs(ref[0]).max(), 0.01)
    print(f"row_adam past 2^31 elements unique={unique}: max error {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    assert np.abs(got[1] - ref[1]).max() <= 2.0 ** -21 * np.abs(ref[1]).max()
    assert np.abs(got[2] - ref[2]).max() <= 2.0 ** -20 * np.abs(ref[2]).max()
