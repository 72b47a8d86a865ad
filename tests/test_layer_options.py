"""The case table of tests/test_gpu_layer_options.py (tests/layer_options.py) held to what it promises, without a GPU: a pairwise
cover of routes x options, every decomposition edge, and the route each entry claims (``RGCNConv._route`` needs no device).
Also the bf16 x 3 split of the weight packer emulated in numpy: the bound tests/test_gpu_decomposed.py asserts on the planes."""
import math

import numpy as np
import pytest

from tests import layer_options as L


def test_flag_values_match_the_library():
    from scaling_rgcn_training_amd import _lib
    assert (L.FLAG_POINTER_GATHER, L.FLAG_DW_RING, L.FLAG_DW_DIRECT) == (_lib.FLAG_POINTER_GATHER, _lib.FLAG_DW_RING, _lib.FLAG_DW_DIRECT)


def test_the_table_is_a_pairwise_cover():
    seen = {pf: set() for pf in L.PAIR_FIELDS}
    for c in L.CASES:
        f = L.case_fields(c)
        for a, b in L.PAIR_FIELDS:
            assert L.pair_admitted(a, f[a], b, f[b]), f"{L.case_id(c)}: ({a}, {b}) = ({f[a]}, {f[b]}) is listed as not admitted"
            seen[(a, b)].add((f[a], f[b]))
    missing = [(a, av, b, bv) for a, b in L.PAIR_FIELDS for av in L.DOMAINS[a] for bv in L.DOMAINS[b]
               if L.pair_admitted(a, av, b, bv) and (av, bv) not in seen[(a, b)]]
    assert not missing, f"{len(missing)} admitted pairs without a case: {missing}"
    assert 40 <= len(L.CASES) <= 70
    assert len({L.case_id(c) for c in L.CASES}) == len(L.CASES)


def test_every_case_is_constructible_and_within_its_route():
    for c in L.CASES:
        tag = L.case_id(c)
        assert c.route in L.ROUTES and c.mode in L.MODES and c.aggr in L.AGGRS and c.frozen in L.FROZEN, tag
        assert 1 <= c.din <= 128 and 1 <= c.dout <= 128 and c.r >= 2, tag
        assert (c.k is None) == (c.mode == "full"), tag
        if c.mode == "block":
            assert c.din % c.k == 0 and c.dout % c.k == 0, tag
        if c.frozen == "root+bias":
            assert c.root or c.bias, f"{tag}: nothing to freeze"
        if c.frozen == "comp":
            assert c.mode == "basis", tag
        pad = lambda w: 16 if w <= 16 else 32 if w <= 32 else 64 if w <= 64 else 128      # noqa: E731
        w64 = pad(c.din) == 64 and pad(c.dout) == 64
        if not c.route.startswith("ep"):       # (the edge-parallel routes take every width class)
            assert w64 == (c.route != "ring-exact"), tag
        if c.route.startswith("tiles"):
            assert c.r <= 32, tag
        if c.route.startswith("ep"):
            assert 45 <= c.r <= 89, tag
        assert c.swap is False or c.route == "ep-ring", tag


def test_decomposition_and_width_edges_occur():
    basis = [c for c in L.CASES if c.mode == "basis"]
    block = [c for c in L.CASES if c.mode == "block"]
    assert any(c.k == 1 for c in basis), "B = 1"
    assert any(c.k > c.r for c in basis), "B > R"
    assert any(c.k == 30 and c.r >= 45 for c in basis), "B = 30 with R >= 45"
    assert any(c.k == 1 for c in block), "num_blocks = 1"
    assert any(c.k == c.din == c.dout == 16 for c in block), "blocks of 1 x 1 at a 16-wide layer"
    assert any(c.din // c.k > c.dout // c.k for c in block) and any(c.din // c.k < c.dout // c.k for c in block), "non-square blocks"
    assert any(c.din % 4 and c.dout % 4 for c in L.CASES) and any(c.din % 4 for c in block) and any(c.din % 4 for c in basis)
    pad = lambda w: 16 if w <= 16 else 32 if w <= 32 else 64 if w <= 64 else 128      # noqa: E731
    exact = [c for c in L.CASES if c.route == "ring-exact"]
    for cls in (16, 32, 64, 128):       # every padded width class on either side of the exact-fp32 tile kernel, odd widths on both
        assert any(pad(c.din) == cls for c in exact) and any(pad(c.dout) == cls for c in exact), cls
    assert any(c.din % 2 for c in exact) and any(c.dout % 2 for c in exact)
    ep = [c for c in L.CASES if c.route == "ep"]
    assert {(63, 16), (32, 32), (64, 64)} <= {(c.din, c.dout) for c in ep} and any(max(c.din, c.dout) > 64 for c in ep)
    assert any(c.split for c in ep) and any(not c.split and (c.din, c.dout) == (64, 64) for c in ep), "both transforms at 64 x 64"
    assert {c.swap for c in L.CASES if c.route == "ep-ring"} == {False, True}, "both orders of the mixed route"
    assert any(c.chunk == 112 for c in L.CASES if c.route == "tiles-split"), "the seven-row-tile ring slots"
    assert any(c.aggr == "sum" for c in L.CASES if c.route.startswith("tiles") and c.mode == "full")


@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_route_claimed_by_the_table(case, monkeypatch):
    """``_route`` of the case's layer, on a graph of the case's size with its tensors on the device: the chunk, the plan layout,
    d_weight on its own plan, the bf16 x 3 flag and the paths the table entry claims -- a change of the layout chooser or of
    the routing shows up here"""
    conv = L.make_layer(case, monkeypatch)
    L.assert_route(case, conv._route(case.n, case.e, True))
    trains = {k for k, p in conv.named_parameters() if p.requires_grad}
    want = {k for k, p in conv.named_parameters()} - {"none": set(), "x": set(), "weight": {"weight"}, "comp": {"comp"},
                                                      "root+bias": {"root", "bias"}, "params": {"weight", "comp", "root", "bias"}}[case.frozen]
    assert trains == want


# ---- the bf16 x 3 split of rgcn_pack3_kernel, emulated ------------------------------------------------------------------------
def bf16_rne(v: np.ndarray) -> np.ndarray:
    """csrc/rgcn_abi.hip bf16_rne on float32 values, returned as float32"""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32)
    return (b << np.uint32(16)).view(np.float32)


def split3(v: np.ndarray):
    """h = bf16(v), m = bf16(v - h), l = bf16(v - h - m), the differences in fp32 as the kernel forms them"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    h = bf16_rne(v)
    v1 = v - h
    m = bf16_rne(v1)
    l = bf16_rne(v1 - m)
    return h, m, l


def test_three_bf16_pieces_rebuild_an_fp32_value_within_2_to_the_minus_27():
    """bf16 keeps 8 significant bits: a round-to-nearest cut leaves at most half a bf16 ulp (2^-8 of the value, and at most 16
    significant bits), the remainders v - h and v - h - m are exact in fp32, and the third piece takes the last 8 bits -- on
    normal values of glorot size the three pieces hold all 24 bits and the rebuilt value is v itself.  So the bound
    test_gpu_decomposed.py asserts on the planes of a pack, 2^-27 |v| (an eighth of an fp32 ulp: any lost bit breaks it), holds
    with nothing to spare on the right side and nothing used on the left."""
    rng = np.random.default_rng(0)
    bound = math.sqrt(6.0 / 128)
    v = rng.uniform(-bound, bound, 2_000_000).astype(np.float32)
    v = v[np.abs(v) >= 2.0 ** -100]
    h, m, l = split3(v)
    v64 = v.astype(np.float64)
    assert np.all(np.abs(v64 - h) <= 2.0 ** -8 * np.abs(v64)) and np.all(np.abs(v64 - h - m) <= 2.0 ** -16 * np.abs(v64))
    assert np.all((v64 - h).astype(np.float32) == v - h) and np.all((v64 - h - m).astype(np.float32) == (v - h) - m), "exact remainders"
    err = np.abs(h.astype(np.float64) + m + l - v64)
    assert np.all(err <= 2.0 ** -27 * np.abs(v64))
    assert float(err.max()) == 0.0
    # a plane emulated wrongly must not pass: without the last piece the error is far above the bound
    assert np.any(np.abs(h.astype(np.float64) + m - v64) > 2.0 ** -27 * np.abs(v64))
