"""Neighbour sampling with one fan-out per relation on the GPU (csrc/rgcn_sample.hip: rgcn_sample_rel_index_build,
rgcn_sample_hop_rel): every index and block EQUAL, field by field, to what tests/sampling_rel_reference.py makes on
the CPU, at the smallest shapes where the kernels can go wrong; then the C ABI called directly between guard words, and the blocks
through ``Emb_Layers.forward_blocks`` against float64 and ``Trainer.train_minibatch``.

The graph of the hop tests: 4,200 nodes, E = 3 x 2,048 + 1, R = 5 with the last relation empty; node 0 a hub whose single run
(relation 2) has 5,000 edges; nodes 1 .. 11 one run each, in relation 1, of lengths 1, 2, 3, 62 .. 66, 255, 256, 257 (k-1, k, k+1
of every fan-out used on relation 1: 1, 2, 63, 64, 65, 256; the length 0 is node 13); node 12 a run in every non-empty relation;
self loops, repeated triples, scattered input order.  5,000 of its 6,145 edges are one run, so it has fewer than 2,047 runs: the
cases with 2,047 / 2,048 / 2,049 units run on a second graph of the same size without a hub."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.tolerance import assert_close
from tests import sampling_reference as R
from tests import sampling_rel_reference as RR
from tests.test_gpu_sampling import _net64, _same

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, E, NREL, HUB = 4200, 3 * 2048 + 1, 5, 5000
RUNS = (1, 2, 3, 62, 63, 64, 65, 66, 255, 256, 257)      # nodes 1 .. 11, relation 1
EVERY = (2, 1, 3, 2)                                     # node 12: its runs in relations 0 .. 3
# relation 1 sees 1, 2, 63, 64, 65, 256, -1 and 0; the largest positive entry walks the register ladder (64 -> 1 register per lane,
# 65 / 128 -> 2, 192 -> 3, 256 -> 4) with the unit's own k below it; the hub (relation 2) is taken whole, dropped, or sampled
FANOUTS = ([256, 1, -1, 0, 5], [64, 2, 1, -1, 0], [0, 63, 65, 1, -1], [1, 64, 64, 0, 3], [-1, 65, 256, 64, 1], [65, 256, 0, 1, 0],
           [3, -1, 128, 1, 1], [1, 0, 192, -1, 7], [0, 0, 0, 0, 0], [-1, -1, -1, -1, -1])


def _graph():
    g = torch.Generator().manual_seed(11)
    dst = [torch.full((HUB,), 0, dtype=torch.int64)]
    typ = [torch.full((HUB,), 2, dtype=torch.int64)]
    for v, d in enumerate(RUNS, start=1):
        dst.append(torch.full((d,), v, dtype=torch.int64))
        typ.append(torch.full((d,), 1, dtype=torch.int64))
    for t, d in enumerate(EVERY):
        dst.append(torch.full((d,), 12, dtype=torch.int64))
        typ.append(torch.full((d,), t, dtype=torch.int64))
    used = sum(int(x.numel()) for x in dst)
    rest = E - used
    assert rest > 0
    dst.append(torch.randint(14, N - 3, (rest,), generator=g))
    typ.append(torch.randint(0, NREL - 1, (rest,), generator=g))     # the last relation is empty
    dst, typ = torch.cat(dst), torch.cat(typ)
    src = torch.randint(0, N, (E,), generator=g)
    src[40:80] = src[0:40]                                           # repeated triples, in the hub's run
    src[HUB:HUB + 30] = dst[HUB:HUB + 30]                            # self loops
    perm = torch.randperm(E, generator=g)                            # a run's edges are scattered over the input
    return torch.stack([src[perm], dst[perm]]), typ[perm]


def _cpu(b):
    return R.Block(*[t.cpu() if torch.is_tensor(t) else t for t in b])


@pytest.fixture(scope="module")
def case():
    from scaling_rgcn_training_amd.sampling import NeighborSampler
    ei, et = _graph()
    ix, rx = R.build_index(ei, et, N), RR.build_rel_index(ei, et, N, NREL)
    # the counts that make this graph the edge case it is meant to be
    pair, cnt = torch.unique(ei[1] * NREL + et, return_counts=True)
    runs = dict(zip(pair.tolist(), cnt.tolist()))
    assert runs[0 * NREL + 2] == HUB and [runs[v * NREL + 1] for v in range(1, 12)] == list(RUNS)
    assert [runs[12 * NREL + t] for t in range(4)] == list(EVERY) and not any(13 * NREL + t in runs for t in range(NREL))
    assert not bool((et == NREL - 1).any()) and rx.num_runs == len(runs) < 2047
    sampler = NeighborSampler(ei.to(DEV), et.to(DEV), N, NREL)      # one sampler for the module: its map must come back clean
    assert sampler._rel_index is None                               # built on the first per-relation hop
    g = torch.Generator().manual_seed(5)
    special = torch.arange(14)
    others = 14 + torch.randperm(N - 14, generator=g)
    dsts = {1: torch.tensor([0]),
            65: torch.cat([special, others[:51]])[torch.randperm(65, generator=g)],
            4097: torch.cat([special, others[:4083]])[torch.randperm(4097, generator=g)]}
    return ei, et, ix, rx, sampler, dsts


def _same_index(arrays, num_runs, rx):
    run_ptr, run_beg, run_type, src = arrays
    assert num_runs == rx.num_runs
    assert torch.equal(run_ptr.cpu().long(), rx.run_ptr)
    assert torch.equal(run_beg[:num_runs + 1].cpu().long(), rx.run_beg)
    assert torch.equal(run_type[:num_runs].cpu().long(), rx.run_type)
    assert torch.equal(src[:rx.src.numel()].cpu().long(), rx.src)


def test_relation_index_equals_the_reference(case):
    ei, et, ix, rx, sampler, dsts = case
    index = sampler._relation_index()
    assert sampler._relation_index() is index                        # built once, kept on the sampler
    _same_index(sampler._rel_arrays, int(index.num_runs), rx)
    assert (int(index.num_edges), int(index.num_nodes), int(index.num_relations)) == (E, N, NREL)


@pytest.mark.parametrize("n_dst", (1, 65, 4097))
@pytest.mark.parametrize("k", FANOUTS, ids=lambda k: "_".join(map(str, k)))
def test_one_hop_equals_the_reference(case, k, n_dst):
    ei, et, ix, rx, sampler, dsts = case
    dst = dsts[n_dst]
    if n_dst > 1:      # what the case is about: runs taken whole and runs sampled in one call, a unit's k below the largest
        d = torch.tensor([HUB] + list(RUNS) + list(EVERY))
        kk = torch.tensor([k[2]] + [k[1]] * len(RUNS) + k[:4])
        sampled, whole = int(((kk > 0) & (d > kk)).sum()), int(((kk < 0) | ((kk > 0) & (d <= kk))).sum())
        assert (sampled > 0) == (max(k) > 0) and (whole > 0) == any(k)
        assert max(k) <= 0 or int(kk[(kk > 0) & (d > kk)].min()) < max(k)      # a sampled unit's k below the largest
    for seed, hop in ((0, 0), (2 ** 63 - 1, 1)):
        want = RR.sample_block_rel(rx, dst, k, seed, hop)
        # a one-layer call samples hop 0; hop 1 is the second layer of a two-layer call whose first is a scalar take-all hop
        if hop == 0:
            got = sampler.sample(dst.to(DEV), (k,), seed)[0]
        else:
            got = sampler.sample(dst.to(DEV), (-1, tuple(k)), seed)[1]
        _same(got, want, f"k={k} n_dst={n_dst} seed={seed} hop={hop}")
    assert bool((sampler._map == -1).all()), "the node map was not reset"


@pytest.fixture(scope="module")
def flat_case():
    """no hub: nearly every edge a run of its own, so destinations can be chosen to give 2,047 / 2,048 / 2,049 units"""
    from scaling_rgcn_training_amd.sampling import NeighborSampler
    ei, et = R.hub_graph(N, E, NREL, seed=23, hub_edges=0)
    ei[1, :400] = ei[1, 0]                                            # one node with runs worth sampling
    rx = RR.build_rel_index(ei, et, N, NREL)
    assert rx.num_runs > 2049
    return ei, et, rx, NeighborSampler(ei.to(DEV), et.to(DEV), N, NREL)


@pytest.mark.parametrize("units", (2047, 2048, 2049))
def test_unit_counts_on_both_sides_of_one_scan_workgroup(flat_case, units):
    ei, et, rx, sampler = flat_case
    per_node = (rx.run_ptr[1:] - rx.run_ptr[:-1]).tolist()
    g = torch.Generator().manual_seed(units)
    chosen, total = [int(ei[1, 0])], per_node[int(ei[1, 0])]
    for v in torch.randperm(N, generator=g).tolist():
        if v != chosen[0] and total + per_node[v] <= units:
            chosen.append(v)
            total += per_node[v]
    dst = torch.tensor(chosen)
    assert int((rx.run_ptr[dst + 1] - rx.run_ptr[dst]).sum()) == units      # the count that makes the case
    for k, seed in (([3, 1, -1, 2, 0], 0), ([0, 65, 1, 1, 1], 9)):
        _same(sampler.sample(dst.to(DEV), (k,), seed)[0], RR.sample_block_rel(rx, dst, k, seed, 0), f"units={units} k={k}")
    assert bool((sampler._map == -1).all())


def test_more_than_256_relations_and_a_three_byte_node_id():
    """R = 300 with runs in relations 255, 256 and 299: the fan-out array past one byte and past one wave; N = 65,537 with
    in-edges on node N - 1: (N - 1) * R + t needs 25 bits, four sort passes, and the node field starts inside a byte"""
    from scaling_rgcn_training_amd.sampling import NeighborSampler
    n, r, e = 65537, 300, 3000
    g = torch.Generator().manual_seed(7)
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, n, (e,), generator=g)
    typ = torch.randint(0, r, (e,), generator=g)
    dst[:600] = torch.tensor([n - 1, 65535, 65534, 255, 256, 0]).repeat(100)
    typ[:600] = torch.tensor([255, 256, 299, 0, 1, 254]).repeat_interleave(100)
    perm = torch.randperm(e, generator=g)
    ei, et = torch.stack([src[perm], dst[perm]]), typ[perm]
    rx, ix = RR.build_rel_index(ei, et, n, r), R.build_index(ei, et, n)
    assert int(((ei[1] == n - 1) & (et == 255)).sum()) >= 16 and int(((ei[1] == 65534) & (et == 299)).sum()) >= 16
    assert ((n - 1) * r + r - 1).bit_length() == 25
    sampler = NeighborSampler(ei.to(DEV), et.to(DEV), n, r)
    index = sampler._relation_index()
    _same_index(sampler._rel_arrays, int(index.num_runs), rx)
    k = [1] * r
    k[254], k[255], k[256], k[299], k[0], k[1] = 0, 3, 65, 7, -1, 2
    dst = torch.cat([torch.tensor([n - 1, 65535, 65534, 255, 256, 0]), torch.randperm(65000, generator=g)[:200] + 300])
    want = RR.sample_block_rel(rx, dst, k, 4, 0)
    types = set(want.edge_type.tolist())
    assert {255, 256, 299}.issubset(types) and 254 not in types
    _same(sampler.sample(dst.to(DEV), (k,), 4)[0], want)
    for a, b in zip(sampler.sample(dst.to(DEV), (2, k), 5), RR.sample_rel(ix, rx, dst, (2, k), 5)):
        _same(a, b)
    assert bool((sampler._map == -1).all())


def test_two_calls_return_equal_tensors_and_seeds_differ(case):
    ei, et, ix, rx, sampler, dsts = case
    f = ([2, 3, 64, 1, 0], [1, 65, -1, 2, 0])
    a = sampler.sample(dsts[4097].to(DEV), f, 9)
    b = sampler.sample(dsts[4097].to(DEV), f, 9)
    c = sampler.sample(dsts[4097].to(DEV), f, 10)
    for x, y in zip(a, b):
        _same(x, _cpu(y))
    assert any(x.edge_index.shape != z.edge_index.shape or not torch.equal(x.edge_index, z.edge_index) for x, z in zip(a, c))


def test_three_layers_mixing_int_and_sequence_entries_chain(case):
    ei, et, ix, rx, sampler, dsts = case
    seeds = dsts[65]
    fanouts = ([2, 2, 1, 0, 0], 65, (1, 3, 64, -1, 2))
    got = sampler.sample(seeds.to(DEV), fanouts, 77)
    want = RR.sample_rel(ix, rx, seeds, fanouts, 77)
    assert len(got) == 3
    for i, (a, b) in enumerate(zip(got, want)):
        _same(a, b, f"layer {i}")
    assert torch.equal(got[2].src_nodes[:65].cpu(), seeds)
    for i in range(2):
        assert got[i].n_dst == got[i + 1].n_src and torch.equal(got[i].src_nodes[:got[i].n_dst], got[i + 1].src_nodes)
        assert torch.unique(got[i].src_nodes).numel() == got[i].n_src
    assert bool((sampler._map == -1).all())


def test_strided_views_of_the_reference_layout(case):
    """edge_index[0 / 1] as rows of a transposed [E, 3] (src, type, dst) tensor, edge_type its middle column"""
    from scaling_rgcn_training_amd.sampling import NeighborSampler
    ei, et, ix, rx, _, dsts = case
    trip = torch.stack([ei[0], et, ei[1]], 1).to(DEV)
    view, typ = trip.t()[0::2], trip[:, 1]
    assert view.stride() == (2, 3) and typ.stride() == (3,) and not view.is_contiguous()
    sampler = NeighborSampler(view, typ, N, NREL)
    index = sampler._relation_index()
    _same_index(sampler._rel_arrays, int(index.num_runs), rx)
    k = [2, 3, 1, 1, 0]
    _same(sampler.sample(dsts[65].to(DEV), (k,), 1)[0], RR.sample_block_rel(rx, dsts[65], k, 1, 0))


def test_graph_without_edges_and_empty_seeds(case):
    from scaling_rgcn_training_amd.sampling import NeighborSampler
    ei = torch.zeros(2, 0, dtype=torch.int64)
    et = torch.zeros(0, dtype=torch.int64)
    sampler = NeighborSampler(ei.to(DEV), et.to(DEV), 10, 2)
    index = sampler._relation_index()
    assert int(index.num_runs) == 0 and not bool(sampler._rel_arrays[0].any()) and int(sampler._rel_arrays[1][0]) == 0
    seeds = torch.tensor([3, 9, 0])
    ix, rx = R.build_index(ei, et, 10), RR.build_rel_index(ei, et, 10, 2)
    for fanouts in (([4, -1], [-1, -1]), ([0, 1],)):
        for a, b in zip(sampler.sample(seeds.to(DEV), fanouts, 0), RR.sample_rel(ix, rx, seeds, fanouts, 0)):
            _same(a, b)
            assert a.n_src == 3 and a.edge_type.numel() == 0
    _, _, _, _, full, _ = case
    blocks = full.sample(torch.zeros(0, dtype=torch.int64, device=DEV), ([3] * NREL, [2] * NREL), 0)
    assert [(b.n_src, b.n_dst, b.edge_type.numel(), tuple(b.edge_index.shape)) for b in blocks] == [(0, 0, 0, (2, 0))] * 2


# ---- the C ABI, called directly ----------------------------------------------------------------------------------------------------
OK, NULL, PLAN, WS, GRAPH, ARG = 0, -1, -4, -6, -9, -11
SENT32, SENT64, SENT8 = -1234567, -7654321012345, 0xA5
AN, AE, AR, ND, TAIL = 300, 1000, 5, 40, 64
AK = [3, 1, -1, 2, 0]


class Call:
    """one well-formed call of each new entry point; keyword overrides swap single arguments"""

    def __init__(self):
        from scaling_rgcn_training_amd import _lib as L
        self.L, self.lib = L, L.load()
        self.ei, self.et = R.hub_graph(AN, AE, AR, seed=1, hub_edges=120)
        self.dei, self.det = self.ei.to(DEV), self.et.to(DEV)
        self.graph, self.keep = L.graph_struct(self.dei, self.det, AN, AR)
        self.ref = RR.build_rel_index(self.ei, self.et, AN, AR)
        self.fan = (C.c_int32 * AR)(*AK)
        self.need_ix = self.lib.rgcn_sample_rel_index_workspace_bytes(AE, AN)
        self.need = self.lib.rgcn_sample_hop_rel_workspace_bytes(ND, self.fan, AR, AE, self.ref.num_runs, AN)
        assert self.need_ix > 0 and self.need > 0
        u8, i32, i64 = (dict(dtype=t, device=DEV) for t in (torch.uint8, torch.int32, torch.int64))
        self.ws_ix = torch.full((4096 + self.need_ix + 4096,), SENT8, **u8)
        self.ws = torch.full((4096 + self.need + 4096,), SENT8, **u8)
        self.run_ptr = torch.full((AN + 1 + TAIL,), SENT32, **i32)
        self.run_beg = torch.full((AE + 1 + TAIL,), SENT32, **i32)
        self.run_type = torch.full((AE + TAIL,), SENT32, **i32)
        self.src = torch.full((AE + TAIL,), SENT32, **i32)
        self.cap = AE                                                  # an entry is -1
        self.edges = torch.full((3, self.cap + TAIL), SENT64, **i64)
        self.nodes = torch.full((ND + min(self.cap, AN) + TAIL,), SENT64, **i64)
        self.map = torch.full((AN + TAIL,), -1, **i32)
        g = torch.Generator().manual_seed(3)
        self.dst = torch.cat([torch.tensor([0, AN - 1]), 1 + torch.randperm(AN - 2, generator=g)[:ND - 2]])
        self.ddst = self.dst.to(DEV)
        self.ne, self.ns, self.nr = C.c_int64(SENT64), C.c_int64(SENT64), C.c_int64(SENT64)
        self.ix, self.ix_arrays = L.sample_rel_index_build(self.graph, torch.device(DEV))      # a good index for the hop calls

    def build(self, **o):
        a = dict(graph=C.byref(self.graph), run_ptr=self.run_ptr.data_ptr(), run_beg=self.run_beg.data_ptr(),
                 run_type=self.run_type.data_ptr(), src=self.src.data_ptr(), ws=self.ws_ix[4096:].data_ptr(), ws_bytes=self.need_ix,
                 nr=C.byref(self.nr))
        a.update(o)
        return self.lib.rgcn_sample_rel_index_build(a["graph"], a["run_ptr"], a["run_beg"], a["run_type"], a["src"], a["ws"],
                                                    a["ws_bytes"], a["nr"], torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def hop(self, **o):
        a = dict(ix=C.byref(self.ix), dst=self.ddst.data_ptr(), nd=ND, fan=self.fan, seed=5, hop=0, map=self.map.data_ptr(),
                 es=self.edges[0].data_ptr(), ed=self.edges[1].data_ptr(), et=self.edges[2].data_ptr(), nodes=self.nodes.data_ptr(),
                 ws=self.ws[4096:].data_ptr(), ws_bytes=self.need, ne=C.byref(self.ne), ns=C.byref(self.ns))
        a.update(o)
        return self.lib.rgcn_sample_hop_rel(a["ix"], a["dst"], a["nd"], a["fan"], a["seed"], a["hop"], a["map"], a["es"], a["ed"],
                                            a["et"], a["nodes"], a["ws"], a["ws_bytes"], a["ne"], a["ns"],
                                            torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def untouched(self):
        torch.cuda.synchronize()
        assert bool((self.ws == SENT8).all()) and bool((self.ws_ix == SENT8).all()), "workspace written by a refused call"
        for t in (self.run_ptr, self.run_beg, self.run_type, self.src):
            assert bool((t == SENT32).all()), "index output written by a refused call"
        assert bool((self.edges == SENT64).all()) and bool((self.nodes == SENT64).all()), "output written by a refused call"
        assert bool((self.map == -1).all()), "node map written by a refused call"
        assert self.ne.value == SENT64 and self.ns.value == SENT64 and self.nr.value == SENT64

    def guards(self, need):
        assert bool((self.ws[:4096] == SENT8).all()) and bool((self.ws[4096 + need:] == SENT8).all()), "hop workspace guard"
        assert bool((self.ws_ix[:4096] == SENT8).all()) and bool((self.ws_ix[4096 + self.need_ix:] == SENT8).all())
        assert bool((self.edges[:, self.cap:] == SENT64).all()) and bool((self.nodes[ND + min(self.cap, AN):] == SENT64).all())
        assert bool((self.map[AN:] == -1).all())


def _struct_with(base, **fields):
    s = type(base)()
    C.memmove(C.byref(s), C.byref(base), C.sizeof(s))
    for k, v in fields.items():
        setattr(s, k, v)
    return C.byref(s)


def _fan(*k):
    return (C.c_int32 * len(k))(*k)


def test_abi_additions_keep_the_version_and_the_status_text():
    from scaling_rgcn_training_amd import _lib as L
    assert L.load().rgcn_abi_version() == 19 == L.ABI_VERSION
    assert b"fan-out" in L.load().rgcn_status_string(ARG)


def test_abi_workspace_queries():
    from scaling_rgcn_training_amd import _lib as L
    lib = L.load()
    qi, qh = lib.rgcn_sample_rel_index_workspace_bytes, lib.rgcn_sample_hop_rel_workspace_bytes
    assert qi(-1, 10) == 0 and qi(10, 0) == 0 and qi(0xFFFF0001, 10) == 0 and qi(0, 1) > 0 and qi(AE, AN) > qi(0, AN)
    good = _fan(*AK)
    assert qh(ND, good, AR, AE, 700, AN) > 0 and qh(0, good, AR, AE, 700, AN) > 0 and qh(ND, good, AR, 0, 0, AN) > 0
    assert qh(-1, good, AR, AE, 700, AN) == 0 and qh(AN + 1, good, AR, AE, 700, AN) == 0 and qh(ND, None, AR, AE, 700, AN) == 0
    assert qh(ND, good, 0, AE, 700, AN) == 0 and qh(ND, good, 65537, AE, 700, AN) == 0 and qh(ND, good, AR, AE, AE + 1, AN) == 0
    assert qh(ND, good, AR, AE, -1, AN) == 0 and qh(ND, good, AR, AE, 700, 0) == 0 and qh(ND, good, AR, 0xFFFF0001, 700, AN) == 0
    for bad in ((3, 1, -2, 2, 0), (3, 1, 257, 2, 0)):
        assert qh(ND, _fan(*bad), AR, AE, 700, AN) == 0
    big = 100_000      # sized by cap: E with a -1, else min(E, num_dst * sum of the positive entries)
    assert qh(1000, _fan(-1, 0, 0, 0, 0), AR, 10 ** 6, 10 ** 5, big) > qh(1000, _fan(3, 2, 0, 0, 0), AR, 10 ** 6, 10 ** 5, big) \
        > qh(1000, _fan(1, 0, 0, 0, 0), AR, 10 ** 6, 10 ** 5, big) > qh(1000, _fan(0, 0, 0, 0, 0), AR, 10 ** 6, 10 ** 5, big) > 0
    assert qh(1000, _fan(256, 256, 0, 0, 0), AR, 200_000, 10 ** 5, big) == qh(1000, _fan(-1, 0, 0, 0, 0), AR, 200_000, 10 ** 5, big)


def test_abi_refusals_launch_nothing():
    """a short workspace, a bad fan-out entry, bad scalars, NULL pointers: a status, and no byte written anywhere"""
    c = Call()
    s = _struct_with
    for o, want in (
            (dict(graph=None), NULL), (dict(run_ptr=None), NULL), (dict(run_beg=None), NULL), (dict(run_type=None), NULL),
            (dict(src=None), NULL), (dict(ws=None), NULL), (dict(nr=None), NULL),
            (dict(graph=s(c.graph, dst=None)), NULL), (dict(ws_bytes=c.need_ix - 1), WS), (dict(ws_bytes=0), WS),
            (dict(graph=s(c.graph, num_edges=-1)), PLAN), (dict(graph=s(c.graph, num_nodes=0)), PLAN),
            (dict(graph=s(c.graph, num_relations=0)), PLAN), (dict(graph=s(c.graph, num_relations=65537)), PLAN),
            (dict(graph=s(c.graph, num_edges=0xFFFF0001)), PLAN)):
        assert c.build(**o) == want, o
        c.untouched()
    for o, want in (
            (dict(ix=None), NULL), (dict(fan=None), NULL), (dict(dst=None), NULL), (dict(map=None), NULL), (dict(es=None), NULL),
            (dict(ed=None), NULL), (dict(et=None), NULL), (dict(nodes=None), NULL), (dict(ws=None), NULL), (dict(ne=None), NULL),
            (dict(ns=None), NULL), (dict(ix=s(c.ix, run_ptr=None)), NULL), (dict(ix=s(c.ix, run_beg=None)), NULL),
            (dict(ix=s(c.ix, run_type=None)), NULL), (dict(ix=s(c.ix, src=None)), NULL),
            (dict(ws_bytes=c.need - 1), WS), (dict(ws_bytes=0), WS),
            (dict(fan=_fan(3, 1, -2, 2, 0)), ARG), (dict(fan=_fan(3, 1, -1, 2, 257)), ARG), (dict(fan=_fan(-2 ** 31, 1, -1, 2, 0)), ARG),
            (dict(seed=-1), ARG), (dict(hop=-1), ARG), (dict(nd=-1), ARG), (dict(nd=AN + 1), ARG),
            (dict(ix=s(c.ix, num_nodes=0)), PLAN), (dict(ix=s(c.ix, num_edges=-1)), PLAN), (dict(ix=s(c.ix, num_runs=-1)), PLAN),
            (dict(ix=s(c.ix, num_runs=AE + 1)), PLAN), (dict(ix=s(c.ix, num_relations=0)), PLAN),
            (dict(ix=s(c.ix, num_edges=0xFFFF0001)), PLAN)):
        assert c.hop(**o) == want, o
        c.untouched()


def test_abi_served_calls_stay_inside_their_outputs():
    c = Call()
    assert c.build() == OK
    torch.cuda.synchronize()
    nr = c.nr.value
    _same_index((c.run_ptr[:AN + 1], c.run_beg, c.run_type, c.src[:AE]), nr, c.ref)
    assert bool((c.run_ptr[AN + 1:] == SENT32).all()) and bool((c.run_beg[nr + 1:] == SENT32).all())
    assert bool((c.run_type[nr:] == SENT32).all()) and bool((c.src[AE:] == SENT32).all())
    c.guards(c.need)
    for k, seed, hop in ((AK, 5, 0), ([1, 0, 2, 256, 1], 2 ** 63 - 1, 7), ([0] * AR, 1, 0)):
        c.edges.fill_(SENT64)
        c.nodes.fill_(SENT64)
        c.ws.fill_(SENT8)
        fan = _fan(*k)
        need = c.lib.rgcn_sample_hop_rel_workspace_bytes(ND, fan, AR, AE, nr, AN)
        assert 0 < need <= c.need
        assert c.hop(fan=fan, seed=seed, hop=hop, ws_bytes=need) == OK
        torch.cuda.synchronize()
        want = RR.sample_block_rel(c.ref, c.dst, k, seed, hop)
        ne, ns = c.ne.value, c.ns.value
        assert (ne, ns) == (want.edge_type.numel(), want.n_src)
        got = c.edges[:, :ne].cpu()
        assert torch.equal(got[:2], want.edge_index) and torch.equal(got[2], want.edge_type)
        assert torch.equal(c.nodes[:ns].cpu(), want.src_nodes)
        assert bool((c.edges[:, ne:] == SENT64).all()) and bool((c.nodes[ns:] == SENT64).all())
        c.guards(need)
        assert bool((c.map == -1).all())
    c.ne.value = c.ns.value = SENT64
    c.edges.fill_(SENT64)
    assert c.hop(nd=0, dst=None) == OK and (c.ne.value, c.ns.value) == (0, 0)      # no destinations: nothing launched
    torch.cuda.synchronize()
    assert bool((c.edges == SENT64).all())


def test_abi_bad_ids_are_answered_with_a_status():
    """an id out of range in the graph, a destination out of range: RGCN_ERR_GRAPH; a destination listed twice: RGCN_ERR_ARG;
    nothing outside the outputs is written and the node map is reset"""
    c = Call()
    for row, col, val in ((0, 17, AN), (1, 900, -1), (2, 5, AR), (2, 6, -3)):
        t = torch.stack([c.ei[0], c.ei[1], c.et]).clone()
        t[row, col] = val
        d = t.to(DEV)
        g, keep = c.L.graph_struct(d[:2], d[2], AN, AR)
        assert c.build(graph=C.byref(g)) == GRAPH
        torch.cuda.synchronize()
        assert bool((c.run_ptr[AN + 1:] == SENT32).all()) and bool((c.run_beg[AE + 1:] == SENT32).all())
        assert bool((c.run_type[AE:] == SENT32).all()) and bool((c.src[AE:] == SENT32).all())
        c.guards(c.need)
    for pos, val, want in ((3, AN, GRAPH), (0, -1, GRAPH), (ND - 1, 2 ** 40, GRAPH), (7, 0, ARG), (ND - 1, int(c.dst[5]), ARG)):
        bad = c.dst.clone()
        bad[pos] = val
        dbad = bad.to(DEV)
        assert c.hop(dst=dbad.data_ptr()) == want, (pos, val)
        torch.cuda.synchronize()
        assert bool((c.map == -1).all()), "node map not reset after an error found on the device"
        c.guards(c.need)
    assert c.hop() == OK


# ---- through the layer and the model -------------------------------------------------------------------------------------------
MN, ME, MR, EMB, HID, LAB = 300, 2400, 4, 16, 12, 5


@pytest.fixture(scope="module")
def model_case():
    from scaling_rgcn_training_amd.layers import Emb_Layers
    from scaling_rgcn_training_amd.sampling import NeighborSampler
    ei, et = R.hub_graph(MN, ME, MR, seed=21, hub_edges=150, empty_rel=False)
    torch.manual_seed(0)
    model = Emb_Layers(MR, HID, LAB, MN, EMB, None)
    with torch.no_grad():
        model.rgcn1.bias.normal_(0, 0.1)
        model.rgcn2.bias.normal_(0, 0.1)
    params = {k: v.detach().clone().double() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(6)
    seeds = torch.cat([torch.tensor([0, MN - 1]), 1 + torch.randperm(MN - 2, generator=g)[:30]])
    return ei, et, model.to(DEV), params, seeds, NeighborSampler(ei.to(DEV), et.to(DEV), MN, MR), g


@pytest.mark.parametrize("block_kernels", (False, True))
def test_full_fanout_forward_equals_the_full_graph_rows(model_case, block_kernels):
    from scaling_rgcn_training_amd.trainer import do_nothing
    ei, et, model, params, seeds, sampler, _ = model_case
    blocks = sampler.sample(seeds.to(DEV), ([-1] * MR, [-1] * MR), 0)
    out = model.forward_blocks(blocks, do_nothing, block_kernels)
    torch.cuda.synchronize()
    full = R.Block(ei, et, MN, MN, torch.arange(MN))
    ref = _net64(params, (full, full))[seeds]
    cond = _net64(params, (full, full), absolute=True)[seeds]
    # two chained fp32 layers, each within 4 u of its sum of absolute terms: 2 x the network on absolute values (as the scalar test)
    assert tuple(out.shape) == (seeds.numel(), LAB)
    assert_close(out.detach().cpu().numpy(), ref.numpy(), 2 * cond.numpy(), "forward_blocks, every run whole, vs the full graph")


def test_sampled_forward_and_gradients_match_float64(model_case):
    from scaling_rgcn_training_amd.trainer import do_nothing
    ei, et, model, params, seeds, sampler, g = model_case
    fanouts = ([3, 1, 0, 2], [2, -1, 1, 0])
    blocks = sampler.sample(seeds.to(DEV), fanouts, 4)
    cpu_blocks = [_cpu(b) for b in blocks]
    for a, b in zip(blocks, RR.sample_rel(R.build_index(ei, et, MN), RR.build_rel_index(ei, et, MN, MR), seeds, fanouts, 4)):
        _same(a, b)
    assert all(b.edge_type.numel() > 0 for b in cpu_blocks) and not bool((cpu_blocks[0].edge_type == 2).any())
    dg = torch.randn(seeds.numel(), LAB, generator=g)
    model.zero_grad()
    out = model.forward_blocks(blocks, do_nothing)
    out.backward(dg.to(DEV))
    torch.cuda.synchronize()

    def run(absolute):
        p = {k: (v.abs() if absolute else v).clone().requires_grad_(True) for k, v in params.items()}
        o = _net64(p, cpu_blocks)
        o.backward(dg.double().abs() if absolute else dg.double())
        return o.detach(), {k: v.grad for k, v in p.items()}

    ref, ref_g = run(False)
    cond, cond_g = run(True)
    assert_close(out.detach().cpu().numpy(), ref.numpy(), 2 * cond.numpy(), "forward_blocks per-relation")
    for name, q in model.named_parameters():      # up to four fp32 stages (two forward, two backward): 4 x, as the scalar test
        assert q.grad is not None, name
        assert_close(q.grad.cpu().numpy(), ref_g[name].numpy(), 4 * cond_g[name].numpy(), f"d_{name} per-relation")


def _train(sparse, epochs, fanouts):
    from scaling_rgcn_training_amd.data import Data
    from scaling_rgcn_training_amd.layers import Emb_Layers
    from scaling_rgcn_training_amd.trainer import Trainer, bce_loss
    n, c = 300, 4
    ei, et = R.hub_graph(n, 2400, MR, seed=31, hub_edges=150)
    g = torch.Generator().manual_seed(2)
    y = torch.nn.functional.one_hot(torch.randint(0, c, (n,), generator=g), c).float()
    perm = torch.randperm(n, generator=g)
    data = Data(edge_index=ei)
    data.edge_type = et
    data.x_train, data.y_train = perm[:80], y[perm[:80]]
    data.x_val, data.y_val = perm[80:120], y[perm[80:120]]

    class _Graph:
        pass

    gobj = _Graph()
    gobj.training_data = data
    torch.manual_seed(0)
    model = Emb_Layers(MR, HID, c, n, EMB, None)
    kw = dict(sparse_embedding=True) if sparse else {}
    tr = Trainer(None, HID, epochs=epochs, emb_dim=EMB, lr=0.01, weight_d=5e-5, verbose=False, **kw)
    _, losses, _, _ = tr.train_minibatch(model, gobj, bce_loss, torch.sigmoid, batch_size=32, fanouts=fanouts, seed=3)
    assert [int(b.numel()) for b in tr.last_batches] == [32, 32, 16]
    assert gobj._sampler[1]._rel_index is not None
    return losses


@pytest.mark.parametrize("sparse,epochs", ((False, 2), (True, 1)))
def test_train_minibatch_with_per_relation_fanouts(sparse, epochs):
    fanouts = ([3, 2, -1, 0], (2, 1, 4, 1))
    first = _train(sparse, epochs, fanouts)
    assert len(first) == epochs and all(np.isfinite(first))
    assert _train(sparse, epochs, fanouts) == first      # a repeated run: an equal loss list
