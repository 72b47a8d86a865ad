"""C ABI of the summary entry points (rgcn_summary_workspace_bytes / rgcn_summary_round / rgcn_summary_quotient): every refusal
answers its status code and launches nothing -- outputs, workspace and the host out-words keep their sentinel -- and a served
call writes nothing outside its outputs."""
import ctypes as C

import pytest
import torch

from tests import summary_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OK, NULL, PLAN, WS, GRAPH = 0, -1, -4, -6, -9
SENT32, SENT64, SENT8 = -1234567, -7654321012345, 0xA5
N, E, NREL = 300, 1000, 5


def _L():
    from scaling_rgcn_training_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


class Call:
    """one well-formed call of each entry point; `args(**overrides)` swaps single arguments"""

    def __init__(self, direction=2):
        L = _L()
        self.lib = L.load()
        ei, et = R.random_graph(N, E, NREL, seed=1)
        self.ei, self.et = ei, et
        self.dei, self.det = ei.to(DEV), et.to(DEV)
        self.graph, self.keep = L.graph_struct(self.dei, self.det, N, NREL)
        self.direction = direction
        self.need = self.lib.rgcn_summary_workspace_bytes(E, N, direction)
        assert self.need > 0
        self.ws = torch.full((self.need + 4096,), SENT8, dtype=torch.uint8, device=DEV)
        self.block = torch.zeros(N, dtype=torch.int32, device=DEV)
        self.out = torch.full((N + 64,), SENT32, dtype=torch.int32, device=DEV)
        self.q = torch.full((4, E + 64), SENT64, dtype=torch.int64, device=DEV)
        self.nb, self.ne = C.c_int32(SENT32), C.c_int64(SENT64)

    def round(self, **o):
        a = dict(graph=C.byref(self.graph), direction=self.direction, block_in=self.block.data_ptr(), nb_in=1, route=0,
                 block_out=self.out.data_ptr(), ws=self.ws.data_ptr(), ws_bytes=self.need, nb_out=C.byref(self.nb))
        a.update(o)
        return self.lib.rgcn_summary_round(a["graph"], a["direction"], a["block_in"], a["nb_in"], a["route"], a["block_out"], a["ws"],
                                           a["ws_bytes"], a["nb_out"], _stream())

    def quotient(self, **o):
        a = dict(graph=C.byref(self.graph), block=self.block.data_ptr(), nb=1, route=0, src=self.q[0].data_ptr(),
                 dst=self.q[1].data_ptr(), typ=self.q[2].data_ptr(), mult=self.q[3].data_ptr(), ws=self.ws.data_ptr(),
                 ws_bytes=self.need, ne_out=C.byref(self.ne))
        a.update(o)
        return self.lib.rgcn_summary_quotient(a["graph"], a["block"], a["nb"], a["route"], a["src"], a["dst"], a["typ"], a["mult"],
                                              a["ws"], a["ws_bytes"], a["ne_out"], _stream())

    def untouched(self):
        torch.cuda.synchronize()
        assert bool((self.ws == SENT8).all()), "workspace written by a refused call"
        assert bool((self.out == SENT32).all()) and bool((self.q == SENT64).all()), "output written by a refused call"
        assert self.nb.value == SENT32 and self.ne.value == SENT64, "host out-word written by a refused call"

    def graph_with(self, **fields):
        L = _L()
        g = L.RgcnGraphStruct()
        C.memmove(C.byref(g), C.byref(self.graph), C.sizeof(g))
        for k, v in fields.items():
            setattr(g, k, v)
        return C.byref(g)


def test_abi_version_is_still_19():
    L = _L()
    assert L.load().rgcn_abi_version() == 19 == L.ABI_VERSION


def test_workspace_query():
    lib = _L().load()
    q = lib.rgcn_summary_workspace_bytes
    assert q(-1, 10, 0) == 0 and q(10, 0, 0) == 0 and q(10, -3, 0) == 0 and q(10, 10, 3) == 0 and q(10, 10, -1) == 0
    assert q(0xFFFF0001, 10, 0) == 0 and q(0x7FFF8001, 10, 2) == 0
    assert q(0, 1, 0) > 0
    assert q(E, N, 2) > q(E, N, 0) == q(E, N, 1) > q(0, N, 0)
    assert q(0xFFFF0000, 10, 0) > 0 and q(0x7FFF8000, 10, 2) > 0


def test_round_refusals_launch_nothing():
    c = Call()
    for o, want in (
            (dict(graph=None), NULL), (dict(block_in=None), NULL), (dict(block_out=None), NULL), (dict(ws=None), NULL),
            (dict(nb_out=None), NULL),
            (dict(graph=c.graph_with(src=None)), NULL), (dict(graph=c.graph_with(dst=None)), NULL),
            (dict(graph=c.graph_with(type=None)), NULL),
            (dict(ws_bytes=c.need - 1), WS), (dict(ws_bytes=0), WS),
            (dict(direction=3), PLAN), (dict(direction=-1), PLAN), (dict(nb_in=0), PLAN), (dict(nb_in=-5), PLAN),
            (dict(route=3), PLAN), (dict(route=-1), PLAN),
            (dict(graph=c.graph_with(num_edges=-1)), PLAN), (dict(graph=c.graph_with(num_nodes=0)), PLAN),
            (dict(graph=c.graph_with(num_nodes=-7)), PLAN), (dict(graph=c.graph_with(num_relations=0)), PLAN),
            (dict(graph=c.graph_with(num_relations=65537)), PLAN),
            (dict(graph=c.graph_with(num_edges=0x7FFF8001)), PLAN),                 # in_out: two keys per edge
            (dict(graph=c.graph_with(num_edges=0xFFFF0001), direction=0), PLAN),
            (dict(nb_in=2 ** 31 - 1, route=1, graph=c.graph_with(num_relations=65536, num_nodes=2 ** 31 - 1)), PLAN),   # 31 + 1 + 16 + 31 bits
    ):
        assert c.round(**o) == want, o
        c.untouched()


def test_quotient_refusals_launch_nothing():
    c = Call(direction=0)
    for o, want in (
            (dict(graph=None), NULL), (dict(block=None), NULL), (dict(ws=None), NULL), (dict(ne_out=None), NULL),
            (dict(src=None), NULL), (dict(dst=None), NULL), (dict(typ=None), NULL), (dict(mult=None), NULL),
            (dict(graph=c.graph_with(src=None)), NULL), (dict(graph=c.graph_with(type=None)), NULL),
            (dict(ws_bytes=c.need - 1), WS),
            (dict(nb=0), PLAN), (dict(nb=-1), PLAN), (dict(route=3), PLAN), (dict(route=-2), PLAN),
            (dict(graph=c.graph_with(num_edges=-1)), PLAN), (dict(graph=c.graph_with(num_nodes=0)), PLAN),
            (dict(graph=c.graph_with(num_relations=0)), PLAN), (dict(graph=c.graph_with(num_relations=65537)), PLAN),
            (dict(graph=c.graph_with(num_edges=0xFFFF0001)), PLAN),
            (dict(nb=2 ** 31 - 1, route=1), PLAN),                                                            # 31 + 31 + 3 bits
    ):
        assert c.quotient(**o) == want, o
        c.untouched()


@pytest.mark.parametrize("direction", (0, 1, 2))
def test_served_calls_stay_inside_their_outputs(direction):
    """exact workspace, outputs with sentinel tails: the tails stay, the results are the oracle's"""
    c = Call(direction)
    assert c.round() == OK
    torch.cuda.synchronize()
    want = R.node_partition(c.ei, c.et, N, NREL, k=1, direction=("out", "in", "in_out")[direction])
    assert c.nb.value == want.num_blocks
    assert torch.equal(c.out[:N].cpu().long(), want.block) and bool((c.out[N:] == SENT32).all())
    assert bool((c.ws[c.need:] == SENT8).all())
    block = c.out[:N].clone()
    assert c.quotient(block=block.data_ptr(), nb=want.num_blocks) == OK
    torch.cuda.synchronize()
    wi, wt, wm = R.quotient_graph(c.ei, c.et, want.block)
    ne = c.ne.value
    assert ne == wt.numel()
    got = c.q[:, :ne].cpu()
    assert torch.equal(got[:2], wi) and torch.equal(got[2], wt) and torch.equal(got[3], wm)
    assert bool((c.q[:, ne:] == SENT64).all()) and bool((c.ws[c.need:] == SENT8).all())
    # in place: block_out may alias block_in
    again = torch.zeros(N, dtype=torch.int32, device=DEV)
    assert c.round(block_in=again.data_ptr(), block_out=again.data_ptr()) == OK
    assert torch.equal(again.cpu().long(), want.block)


def test_bad_ids_are_found_on_the_device():
    """a node id, a relation id or a block id out of range: RGCN_ERR_GRAPH, and nothing outside the outputs is written"""
    L = _L()
    c = Call(direction=2)
    for row, col, val in ((0, 17, N), (1, 900, -1), (2, 5, NREL), (2, 6, -3)):
        t = torch.stack([c.ei[0], c.ei[1], c.et]).clone()
        t[row, col] = val
        d = t.to(DEV)
        g, keep = L.graph_struct(d[:2], d[2], N, NREL)
        assert c.round(graph=C.byref(g)) == GRAPH
        assert c.quotient(graph=C.byref(g)) == GRAPH
        torch.cuda.synchronize()
        assert bool((c.out[N:] == SENT32).all()) and bool((c.ws[c.need:] == SENT8).all()) and bool((c.q[:, E:] == SENT64).all())
    bad_block = torch.zeros(N, dtype=torch.int32, device=DEV)
    bad_block[int(c.ei[1, 3])] = 4
    assert c.round(block_in=bad_block.data_ptr(), nb_in=4) == GRAPH
    assert c.quotient(block=bad_block.data_ptr(), nb=4) == GRAPH
    assert c.round(block_in=bad_block.data_ptr(), nb_in=5) == OK and c.quotient(block=bad_block.data_ptr(), nb=5) == OK
