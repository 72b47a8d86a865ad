"""The case table of tests/test_gpu_bipartite_options.py (tests/bipartite_options.py) held to what it promises, without a GPU: a
pairwise cover of routes x options, every decomposition and size edge, and the route each entry claims
(``RGCNConv._route(max(N_src, N_dst), E, True, plain=True)`` needs no device)."""
import pytest

from tests import bipartite_options as L


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
    # one case per admitted (route, frozen) pair is the least a cover can hold: the table holds no more
    assert len(L.CASES) == len(L.ROUTES) * len(L.FROZEN) == 49
    assert len({L.case_id(c) for c in L.CASES}) == len(L.CASES)


def test_what_is_not_admitted_is_what_the_docstring_names():
    out = {(a, av, b, bv) for a, b in L.PAIR_FIELDS for av in L.DOMAINS[a] for bv in L.DOMAINS[b] if not L.pair_admitted(a, av, b, bv)}
    assert out == {("mode", "full", "frozen", "comp"), ("mode", "block", "frozen", "comp")}
    # the two (root/bias, frozen) pairs are not among the pairs covered: they bind case by case
    assert not L.pair_admitted("root_bias", (False, True), "frozen", "x_dst") and not L.pair_admitted("root_bias", (False, False), "frozen", "x_dst")
    assert not L.pair_admitted("root_bias", (False, False), "frozen", "root+bias") and L.pair_admitted("root_bias", (False, True), "frozen", "root+bias")
    for text in ("frozen = comp outside basis mode", "frozen = x_dst on a layer without a root", "frozen = root+bias on a layer with neither"):
        assert text in L.__doc__


def test_every_case_is_constructible_and_within_its_route():
    pad = lambda w: 16 if w <= 16 else 32 if w <= 32 else 64 if w <= 64 else 128      # noqa: E731
    for c in L.CASES:
        tag = L.case_id(c)
        assert c.route in L.ROUTES and c.mode in L.MODES and c.aggr in L.AGGRS and c.frozen in L.FROZEN, tag
        assert all(1 <= w <= 128 for w in (c.in_src, c.in_dst, c.dout)) and c.r >= 3, tag
        assert (c.k is None) == (c.mode == "full"), tag
        if c.mode == "block":
            assert c.in_src % c.k == 0 and c.dout % c.k == 0, tag
        if c.frozen == "root+bias":
            assert c.root or c.bias, f"{tag}: nothing to freeze"
        if c.frozen == "x_dst":
            assert c.root, f"{tag}: x_dst is read by the root term alone"
        if c.frozen == "comp":
            assert c.mode == "basis", tag
        w64 = pad(c.in_src) == 64 and pad(c.dout) == 64
        if not c.route.startswith("ep"):       # (the edge-parallel routes take every width class)
            assert w64 == (c.route != "ring-exact"), tag
            assert c.r == 9, tag
        else:
            assert 45 <= c.r <= 89, tag
        assert c.split == (w64 and c.chunk == 128), tag
        assert c.swap is False or c.route == "ep-ring", tag
        assert (c.n_src, c.n_dst) in (L.A, L.B) and c.e in (L.E, L.ED), tag
        ei, et = L.make_graph(c)
        assert tuple(ei.shape) == (2, c.e) and int(ei[0].max()) < c.n_src and int(ei[1].max()) < c.n_dst - 5, tag
        assert int((et == c.r - 1).sum()) == 0 and int(((ei[1] == 0) & (et == 0)).sum()) >= L.HUB, tag
        assert int(((ei[0] == 0) & (et == 1)).sum()) >= L.HUB, tag


def test_decomposition_size_and_width_edges_occur():
    pad = lambda w: 16 if w <= 16 else 32 if w <= 32 else 64 if w <= 64 else 128      # noqa: E731
    basis = [c for c in L.CASES if c.mode == "basis"]
    block = [c for c in L.CASES if c.mode == "block"]
    assert any(c.k == 1 for c in basis), "B = 1"
    assert any(c.k > c.r for c in basis), "B > R"
    assert any(c.k == 1 for c in block), "num_blocks = 1"
    assert any(c.k == c.in_src == c.dout for c in block), "blocks of 1 x 1"
    assert any(1 < c.in_src // c.k < 4 for c in block), "blocks narrower than four columns"
    assert any(c.in_src // c.k != c.dout // c.k for c in block), "non-square blocks"
    assert any(c.frozen == "comp" for c in basis) and any(c.frozen in ("weight", "params") for c in basis)
    for route in L.ROUTES:       # both orders of the sizes, most widths unequal, on every route
        mine = [c for c in L.CASES if c.route == route]
        assert {(c.n_src, c.n_dst) for c in mine} == {L.A, L.B}, route
        assert sum(c.in_src != c.in_dst for c in mine) >= 5, route
    tiles = lambda n: (n // 64, n % 64)       # noqa: E731  (the smallest tile of the layout chooser)
    assert all(tiles(n)[0] > 2 and tiles(n)[1] for n in L.A), "both node ranges span several tiles and end inside one"
    exact = [c for c in L.CASES if c.route == "ring-exact"]
    for cls in (16, 32, 128):
        assert any(pad(c.in_src) == cls for c in exact) and any(pad(c.dout) == cls for c in exact), cls
    assert {c.chunk for c in exact} == {64, 128}, "64- and 128-slot chunks on the ring"
    ep = [c for c in L.CASES if c.route == "ep"]
    assert any(c.split and c.chunk == 128 for c in ep), "the bf16 x 3 transform on 128-slot routes"
    assert any(not c.split and pad(c.in_src) == pad(c.dout) == 64 for c in ep), "the exact transform at 64 x 64"
    assert any(max(c.in_src, c.dout) > 64 for c in ep) and any(c.r == 89 for c in ep) and any(c.r == 45 for c in ep)
    mixed = [c for c in L.CASES if c.route == "ep-ring"]
    assert {c.swap for c in mixed} == {False, True} and {c.swap for c in mixed if c.split} == {True}, "both orders of the mixed route"
    assert {c.aggr for c in L.CASES if c.mode == "full"} == {"mean", "sum"}


@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_route_claimed_by_the_table(case):
    """``_route`` of the case's layer on the square graph a bipartite call runs on: the chunk, layout 0, no tile-major d_weight,
    the bf16 x 3 flag and the paths the table entry claims -- a change of the layout chooser or of the routing shows up here"""
    conv = L.make_layer(case)
    L.assert_route(case, conv._route(max(case.n_src, case.n_dst), case.e, True, plain=True))
    assert conv.kernel_flags == L.ROUTES[case.route].flags and (conv.in_channels, conv.in_channels_r) == (case.in_src, case.in_dst)
    trains = {k for k, p in conv.named_parameters() if p.requires_grad}
    assert trains == {k for k, p in conv.named_parameters()} - set(L.frozen_params(case))
