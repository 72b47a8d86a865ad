"""C ABI of the sampling entry points (rgcn_sample_index_workspace_bytes / rgcn_sample_hop_workspace_bytes /
rgcn_sample_index_build / rgcn_sample_hop): every refusal answers its status code and launches nothing -- outputs, workspace and
the host out-words keep their sentinel -- and a served call writes nothing outside its outputs: guard words sit around the
workspace and behind every output, the node map comes back all "none"."""
import ctypes as C

import pytest
import torch

from tests import sampling_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OK, NULL, PLAN, WS, GRAPH, ARG = 0, -1, -4, -6, -9, -11
SENT32, SENT64, SENT8 = -1234567, -7654321012345, 0xA5
N, E, NREL, ND, K, TAIL = 300, 1000, 5, 40, 3, 64


def _L():
    from scaling_rgcn_training_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


class Call:
    """one well-formed call of each entry point; keyword overrides swap single arguments"""

    def __init__(self):
        L = _L()
        self.lib = L.load()
        self.ei, self.et = R.hub_graph(N, E, NREL, seed=1, hub_edges=120)
        self.dei, self.det = self.ei.to(DEV), self.et.to(DEV)
        self.graph, self.keep = L.graph_struct(self.dei, self.det, N, NREL)
        self.ref = R.build_index(self.ei, self.et, N)
        self.need_ix = self.lib.rgcn_sample_index_workspace_bytes(E, N)
        self.need = self.lib.rgcn_sample_hop_workspace_bytes(ND, K, E, N)
        assert self.need_ix > 0 and self.need > 0
        u8, i32, i64 = (dict(dtype=t, device=DEV) for t in (torch.uint8, torch.int32, torch.int64))
        self.ws_ix = torch.full((4096 + self.need_ix + 4096,), SENT8, **u8)
        self.ws = torch.full((4096 + self.need + 4096,), SENT8, **u8)
        self.ptr = torch.full((N + 1 + TAIL,), SENT32, **i32)
        self.src = torch.full((E + TAIL,), SENT32, **i32)
        self.typ = torch.full((E + TAIL,), SENT32, **i32)
        self.cap = min(E, ND * K)
        self.edges = torch.full((3, self.cap + TAIL), SENT64, **i64)
        self.nodes = torch.full((ND + min(self.cap, N) + TAIL,), SENT64, **i64)
        self.map = torch.full((N + TAIL,), -1, **i32)
        g = torch.Generator().manual_seed(3)
        self.dst = torch.cat([torch.tensor([0, N - 1]), 1 + torch.randperm(N - 2, generator=g)[:ND - 2]])
        self.ddst = self.dst.to(DEV)
        self.ne, self.ns = C.c_int64(SENT64), C.c_int64(SENT64)
        # a good index for the hop calls, built through the binding
        self.ix, self.ix_arrays = L.sample_index_build(self.graph, torch.device(DEV))

    def build(self, **o):
        a = dict(graph=C.byref(self.graph), ptr=self.ptr.data_ptr(), src=self.src.data_ptr(), typ=self.typ.data_ptr(),
                 ws=self.ws_ix[4096:].data_ptr(), ws_bytes=self.need_ix)
        a.update(o)
        return self.lib.rgcn_sample_index_build(a["graph"], a["ptr"], a["src"], a["typ"], a["ws"], a["ws_bytes"], _stream())

    def hop(self, **o):
        a = dict(ix=C.byref(self.ix), dst=self.ddst.data_ptr(), nd=ND, k=K, seed=5, hop=0, map=self.map.data_ptr(),
                 es=self.edges[0].data_ptr(), ed=self.edges[1].data_ptr(), et=self.edges[2].data_ptr(), nodes=self.nodes.data_ptr(),
                 ws=self.ws[4096:].data_ptr(), ws_bytes=self.need, ne=C.byref(self.ne), ns=C.byref(self.ns))
        a.update(o)
        return self.lib.rgcn_sample_hop(a["ix"], a["dst"], a["nd"], a["k"], a["seed"], a["hop"], a["map"], a["es"], a["ed"], a["et"],
                                        a["nodes"], a["ws"], a["ws_bytes"], a["ne"], a["ns"], _stream())

    def untouched(self):
        torch.cuda.synchronize()
        assert bool((self.ws == SENT8).all()) and bool((self.ws_ix == SENT8).all()), "workspace written by a refused call"
        assert bool((self.ptr == SENT32).all()) and bool((self.src == SENT32).all()) and bool((self.typ == SENT32).all())
        assert bool((self.edges == SENT64).all()) and bool((self.nodes == SENT64).all()), "output written by a refused call"
        assert bool((self.map == -1).all()), "node map written by a refused call"
        assert self.ne.value == SENT64 and self.ns.value == SENT64, "host out-word written by a refused call"

    def struct_with(self, base, **fields):
        s = type(base)()
        C.memmove(C.byref(s), C.byref(base), C.sizeof(s))
        for k, v in fields.items():
            setattr(s, k, v)
        return C.byref(s)


def test_abi_version_is_still_19():
    L = _L()
    assert L.load().rgcn_abi_version() == 19 == L.ABI_VERSION
    assert b"fan-out" in L.load().rgcn_status_string(ARG)
    assert (L.ERR_GRAPH, L.ERR_ARG) == (GRAPH, ARG)


def test_workspace_queries():
    lib = _L().load()
    qi, qh = lib.rgcn_sample_index_workspace_bytes, lib.rgcn_sample_hop_workspace_bytes
    assert qi(-1, 10) == 0 and qi(10, 0) == 0 and qi(10, -3) == 0 and qi(0xFFFF0001, 10) == 0
    assert qi(0, 1) > 0 and qi(0xFFFF0000, 10) > 0 and qi(E, N) > qi(0, N)
    assert qh(-1, 3, E, N) == 0 and qh(N + 1, 3, E, N) == 0 and qh(10, 0, E, N) == 0 and qh(10, 257, E, N) == 0
    assert qh(10, -2, E, N) == 0 and qh(10, 3, -1, N) == 0 and qh(10, 3, E, 0) == 0 and qh(10, 3, 0xFFFF0001, N) == 0
    assert qh(0, 3, E, N) > 0 and qh(10, 3, 0, N) > 0 and qh(N, 256, 0xFFFF0000, N) > 0
    big = 100_000                                                          # sized by cap = min(E, num_dst * fanout), E for -1
    assert qh(1000, -1, 10 ** 6, big) > qh(1000, 3, 10 ** 6, big) > qh(1000, 1, 10 ** 6, big)
    assert qh(1000, 256, 200_000, big) == qh(1000, -1, 200_000, big)       # 256,000 > E: both hold E edges at most


def test_index_build_refusals_launch_nothing():
    c = Call()
    for o, want in (
            (dict(graph=None), NULL), (dict(ptr=None), NULL), (dict(src=None), NULL), (dict(typ=None), NULL), (dict(ws=None), NULL),
            (dict(graph=c.struct_with(c.graph, src=None)), NULL), (dict(graph=c.struct_with(c.graph, dst=None)), NULL),
            (dict(graph=c.struct_with(c.graph, type=None)), NULL),
            (dict(ws_bytes=c.need_ix - 1), WS), (dict(ws_bytes=0), WS),
            (dict(graph=c.struct_with(c.graph, num_edges=-1)), PLAN), (dict(graph=c.struct_with(c.graph, num_nodes=0)), PLAN),
            (dict(graph=c.struct_with(c.graph, num_nodes=-7)), PLAN), (dict(graph=c.struct_with(c.graph, num_relations=0)), PLAN),
            (dict(graph=c.struct_with(c.graph, num_relations=65537)), PLAN),
            (dict(graph=c.struct_with(c.graph, num_edges=0xFFFF0001)), PLAN),
    ):
        assert c.build(**o) == want, o
        c.untouched()


def test_hop_refusals_launch_nothing():
    c = Call()
    for o, want in (
            (dict(ix=None), NULL), (dict(dst=None), NULL), (dict(map=None), NULL), (dict(es=None), NULL), (dict(ed=None), NULL),
            (dict(et=None), NULL), (dict(nodes=None), NULL), (dict(ws=None), NULL), (dict(ne=None), NULL), (dict(ns=None), NULL),
            (dict(ix=c.struct_with(c.ix, ptr=None)), NULL), (dict(ix=c.struct_with(c.ix, src=None)), NULL),
            (dict(ix=c.struct_with(c.ix, type=None)), NULL),
            (dict(ws_bytes=c.need - 1), WS), (dict(ws_bytes=0), WS),
            (dict(k=0), ARG), (dict(k=-2), ARG), (dict(k=257), ARG), (dict(seed=-1), ARG), (dict(seed=-2 ** 63), ARG),
            (dict(hop=-1), ARG), (dict(nd=-1), ARG), (dict(nd=N + 1), ARG),
            (dict(ix=c.struct_with(c.ix, num_nodes=0)), PLAN), (dict(ix=c.struct_with(c.ix, num_edges=-1)), PLAN),
            (dict(ix=c.struct_with(c.ix, num_edges=0xFFFF0001)), PLAN),
    ):
        assert c.hop(**o) == want, o
        c.untouched()


def test_served_calls_stay_inside_their_outputs():
    """exact workspaces between guard pages, outputs with sentinel tails: the guards stay, the results are the reference's"""
    c = Call()
    assert c.build() == OK
    torch.cuda.synchronize()
    assert torch.equal(c.ptr[:N + 1].cpu().long(), c.ref.ptr) and bool((c.ptr[N + 1:] == SENT32).all())
    assert torch.equal(c.src[:E].cpu().long(), c.ref.src) and bool((c.src[E:] == SENT32).all())
    assert torch.equal(c.typ[:E].cpu().long(), c.ref.type) and bool((c.typ[E:] == SENT32).all())
    assert bool((c.ws_ix[:4096] == SENT8).all()) and bool((c.ws_ix[4096 + c.need_ix:] == SENT8).all())
    for k, seed, hop in ((K, 5, 0), (1, 2 ** 63 - 1, 7)):
        c.edges.fill_(SENT64)
        c.nodes.fill_(SENT64)
        c.ws.fill_(SENT8)
        need = c.lib.rgcn_sample_hop_workspace_bytes(ND, k, E, N)
        assert need <= c.need
        assert c.hop(k=k, seed=seed, hop=hop, ws_bytes=need) == OK
        torch.cuda.synchronize()
        want = R.sample_block(c.ref, c.dst, k, seed, hop)
        ne, ns = c.ne.value, c.ns.value
        assert (ne, ns) == (want.edge_type.numel(), want.n_src)
        got = c.edges[:, :ne].cpu()
        assert torch.equal(got[:2], want.edge_index) and torch.equal(got[2], want.edge_type)
        assert torch.equal(c.nodes[:ns].cpu(), want.src_nodes)
        assert bool((c.edges[:, ne:] == SENT64).all()) and bool((c.nodes[ns:] == SENT64).all())
        assert bool((c.ws[:4096] == SENT8).all()) and bool((c.ws[4096 + need:] == SENT8).all())
        assert bool((c.map == -1).all())
    # no destinations: an empty block, nothing launched
    c.ne.value = c.ns.value = SENT64
    c.edges.fill_(SENT64)
    assert c.hop(nd=0, dst=None) == OK and (c.ne.value, c.ns.value) == (0, 0)
    torch.cuda.synchronize()
    assert bool((c.edges == SENT64).all())


def test_bad_ids_are_found_on_the_device():
    """a node or relation id out of range in the graph, a destination out of range: RGCN_ERR_GRAPH; a destination listed twice:
    RGCN_ERR_ARG; nothing outside the outputs is written and the node map is reset"""
    L = _L()
    c = Call()
    for row, col, val in ((0, 17, N), (1, 900, -1), (2, 5, NREL), (2, 6, -3)):
        t = torch.stack([c.ei[0], c.ei[1], c.et]).clone()
        t[row, col] = val
        d = t.to(DEV)
        g, keep = L.graph_struct(d[:2], d[2], N, NREL)
        assert c.build(graph=C.byref(g)) == GRAPH
        torch.cuda.synchronize()
        assert bool((c.ptr[N + 1:] == SENT32).all()) and bool((c.src[E:] == SENT32).all()) and bool((c.typ[E:] == SENT32).all())
        assert bool((c.ws_ix[:4096] == SENT8).all()) and bool((c.ws_ix[4096 + c.need_ix:] == SENT8).all())
    for pos, val, want in ((3, N, GRAPH), (0, -1, GRAPH), (ND - 1, 2 ** 40, GRAPH), (7, 0, ARG), (ND - 1, int(c.dst[5]), ARG)):
        bad = c.dst.clone()
        bad[pos] = val
        dbad = bad.to(DEV)
        assert c.hop(dst=dbad.data_ptr()) == want, (pos, val)
        torch.cuda.synchronize()
        assert bool((c.map == -1).all()), "node map not reset after an error found on the device"
        assert bool((c.edges[:, c.cap:] == SENT64).all()) and bool((c.nodes[ND + min(c.cap, N):] == SENT64).all())
        assert bool((c.ws[:4096] == SENT8).all()) and bool((c.ws[4096 + c.need:] == SENT8).all())
    assert c.hop() == OK
