"""The host's rules past 2^24 rows and 4 GiB, against the C sources they restate (no GPU needed).

_lib.buffer_addressable mirrors buffer_bytes (csrc/rgcn_kernels_shared.h: which gathered matrices a buffer descriptor reaches),
eplan.EP_MAX_OWNED the layout-2 limit of the plan builder (csrc/rgcn_plan.hip: the most owned rows of an edge-parallel plan).
Past that limit the path choice must never pick the edge-parallel path, and a pinned 'ep' is refused before any plan is built.
tests/test_gpu_past_4gib.py runs the same regime on the GPU."""
import os
import re

import pytest
import torch

from scaling_rgcn_training_amd import _lib, eplan as E, plan as P
from scaling_rgcn_training_amd.conv import RGCNConv

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scaling_rgcn_training_amd", "csrc")
N_PAST = (1 << 24) + 4099


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"\s+", " ", f.read())


def _one(name, pattern):
    m = re.findall(pattern, _src(name))
    assert len(m) == 1, f"{name}: {pattern!r} matched {len(m)} times -- the source changed; update the Python mirror"
    return m[0]


def _int(expr):
    assert re.fullmatch(r"[0-9a-fA-Fx <()]+", expr), expr
    return eval(expr.replace("ull", ""))       # an integer literal or a shift of literals


def test_buffer_addressable_matches_buffer_bytes():
    body = _one("rgcn_kernels_shared.h", r"static unsigned buffer_bytes\(int rows, int ld, unsigned flags\) \{(.*?)\}")
    assert "const size_t bytes = (size_t)rows * ld * sizeof(float);" in body
    assert "const size_t with_pad_row = bytes + (size_t)ld * sizeof(float);" in body
    rows_max, bytes_max = re.fullmatch(r".*return \(rows < \(([^)]+)\) && with_pad_row < (0x[0-9A-Fa-f]+)ull\) \? \(unsigned\)bytes : 0u; ",
                                       body).groups()
    rows_max, bytes_max = _int(rows_max), _int(bytes_max)
    assert (rows_max, bytes_max) == (1 << 24, 0xFFFFFF00)

    def c_rule(rows, ld):
        return rows < rows_max and (rows + 1) * ld * 4 < bytes_max

    cases = [((1 << 24) - 3, 64), ((1 << 24) - 2, 64), ((1 << 24) - 1, 16), (1 << 24, 16), (N_PAST, 16), (N_PAST, 64),
             ((1 << 25) + 4099, 64), (8_388_606, 128), (8_388_607, 128), (8_388_607, 16), (4_194_302, 256), (1, 128)]
    for rows, ld in cases:
        assert _lib.buffer_addressable(rows, ld) == c_rule(rows, ld), (rows, ld)
    # the regimes tests/test_gpu_past_4gib.py relies on
    assert _lib.buffer_addressable((1 << 24) - 3, 64) and not _lib.buffer_addressable((1 << 24) - 2, 64)
    assert not _lib.buffer_addressable(N_PAST, 16) and (N_PAST + 1) * 16 * 4 < bytes_max      # rows alone
    assert _lib.buffer_addressable(8_388_606, 128) and not _lib.buffer_addressable(8_388_607, 128)
    assert _lib.buffer_addressable(8_388_607, 16)


def test_ep_max_owned_matches_the_plan_builder():
    lim = _one("rgcn_plan.hip", r"if \(chunk != 64 \|\| node_end - node_begin > \(([^)]+)\)\) return RGCN_ERR_PLAN;")
    assert _int(lim) == E.EP_MAX_OWNED == 1 << 24


def _graph(kind, r, e=100_000, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = N_PAST
    src = torch.randint(0, n, (e,), generator=g)
    if kind == "hub":
        u = torch.rand(e, generator=g, dtype=torch.float64)
        dst = (torch.floor(u.pow(-5.0)).clamp_(max=2.0 ** 62).to(torch.int64) - 1) % n
    else:
        dst = torch.randint(0, n, (e,), generator=g)
    return torch.stack([src, dst]), torch.randint(0, r, (e,), generator=g)


@pytest.mark.parametrize("kind,r", [("uniform", 32), ("hub", 32), ("uniform", 267)])
def test_auto_path_never_edge_parallel_past_the_limit(kind, r):
    ei, et = _graph(kind, r)
    conv = RGCNConv(64, 64, r)
    tile, chunk = conv.layout(N_PAST, int(et.numel()))
    assert E.decide_paths(ei, N_PAST, r, 64, 64, tile, chunk) == ("ring", "ring")
    assert E.choose_path(N_PAST, int(et.numel()), r, 64, 64, tile, chunk, N_PAST) == "ring"
    # the cost model alone would take the edge-parallel path here: the limit, not the model, decides
    assert "ep" in (E.choose_path(E.EP_MAX_OWNED, int(et.numel()), r, 64, 64, tile, chunk, E.EP_MAX_OWNED),
                    E.choose_path(E.EP_MAX_OWNED, 8_000_000, r, 64, 64, tile, chunk, E.EP_MAX_OWNED))


@pytest.mark.parametrize("paths", [("ep", "ring"), ("ring", "ep"), ("ep", "ep")])
def test_pinned_edge_parallel_path_refused_past_the_limit(paths):
    ei, et = _graph("uniform", 32)
    with pytest.raises(ValueError, match="EP_MAX_OWNED"):
        P.build_graph_plans(ei, et, N_PAST, 32, 272, paths=paths)
    with pytest.raises(ValueError, match="EP_MAX_OWNED"):
        P.cached_graph_plans(ei, et, N_PAST, 32, 272, "mean", paths=paths)
    P.clear_plan_cache()


def test_owned_range_check_is_exact():
    E.check_ep_ranges(("ep", "ep"), [((0, 1 << 24), (5, 5 + (1 << 24)))])
    E.check_ep_ranges(("ring", "ring"), [((0, N_PAST), (0, N_PAST))])
    with pytest.raises(ValueError, match="dX"):
        E.check_ep_ranges(("ring", "ep"), [((0, 1 << 24), (0, (1 << 24) + 1))])
    with pytest.raises(ValueError, match="forward"):
        E.check_ep_ranges(("ep", "ring"), [((0, 16), (0, 16)), ((16, 17 + (1 << 24)), (0, 16))])
