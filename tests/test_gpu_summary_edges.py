"""``summaries.node_partition`` / ``quotient_graph`` (csrc/rgcn_summary.hip and the sort and scan of csrc/rgcn_sort_scan.h it
drives) where tests/test_gpu_summary.py stops, EQUAL to the oracles of tests/summary_reference.py: round keys of exactly 64 bits
(one sort of eight passes, the owner's top bit in bit 63) and of 65 (the automatic fall-back to two sorts) at 2^24 + 1 nodes, whose
node scans run the carry loop of the scan's top level; a quotient key of exactly 64 bits, all of them set in one key; node counts
on either side of 256 and 65,536 with the top node owning edges (a sort pass more or less); node counts on either side of one
scan workgroup.  Every case asserts on the host the property that makes it an edge."""
import functools

import pytest
import torch

from tests import summary_reference as R
from tests.test_gpu_summary import _same

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DIRECTIONS = ("out", "in", "in_out")
SCAN_BLOCK = 2048                                                  # rgcn_sort_scan.h kScanBlock


def bits_for(max_value):
    """rgcn_sort_scan.h bits_for: bits that hold 0 .. max_value, at least 1"""
    return max(1, int(max_value).bit_length())


def _ceil(a, b):
    return -(-a // b)


def _S():
    from scaling_rgcn_training_amd import summaries
    return summaries


def _round_key_bits(n, r, b, direction):
    return bits_for(n - 1) + bits_for(r - 1) + bits_for(b - 1) + (1 if direction == "in_out" else 0)


# ---- 1. round keys of exactly 64 and 65 bits ----------------------------------------------------------------------------------------
N1, R1, B1 = 2 ** 24 + 1, 65536, 2 ** 22 + 1
TOP_BLOCK = (2 ** 22, 2 ** 22 + B1, 2 ** 22 + 2 * B1)              # the nodes of initial block 2^22: the block field's top bit alone


def _wide_graph():
    """100 values v with v, v + B, v + 2B, v + 3B all nodes (one initial block each), among them 0, 1 and 2^22 - 3, whose fourth
    member is node N - 1.  Member j of value i has the chain edge (i, j) -> (i + 1, j) of a type that depends on i alone, so the
    four chains look alike until something marks one of them: three extra edges on chain 1 (it splits from the others one node
    further along per round, in either direction), exact duplicates of chain 0's edges (which must split nothing), and 2,700 random
    edges with duplicates and self-loops among the members 2 and 3 and the nodes of block 2^22."""
    g = torch.Generator().manual_seed(41)
    v = torch.cat([torch.tensor([0, 1, 2 ** 22 - 3]), 2 + torch.randperm(2 ** 22 - 5, generator=g)[:97]])
    assert int(torch.unique(v).numel()) == 100 and int(v.max()) + 3 * B1 <= N1 - 1
    member = v[:, None] + B1 * torch.arange(4)[None, :]            # [100, 4]
    assert int(member[2, 3]) == N1 - 1
    chain_t = torch.tensor([0, 1, 2, 65535])[torch.randint(0, 4, (99,), generator=g)]
    src = [member[:-1].flatten(), member[:-1, 0][::3]]             # chains; every third edge of chain 0 once more
    dst = [member[1:].flatten(), member[1:, 0][::3]]
    typ = [chain_t[:, None].expand(99, 4).flatten(), chain_t[::3]]
    src.append(torch.stack([member[50, 1], member[20, 1], member[80, 1]]))      # the marks on chain 1
    dst.append(torch.stack([member[7, 1], member[20, 1], member[81, 1]]))
    typ.append(torch.tensor([65535, 0, 3]))
    pool = torch.cat([member[:, 2:].flatten(), torch.tensor(TOP_BLOCK)])
    rs, rd = pool[torch.randint(0, int(pool.numel()), (2, 2700), generator=g)]
    rt = torch.randint(0, R1, (2700,), generator=g)
    rt[:1500] %= 4                                                 # some sharing of relations
    rs[:60], rd[:60], rt[:60] = rs[60:120], rd[60:120], rt[60:120]               # exact duplicates
    rd[120:150] = rs[120:150]                                      # self-loops
    # all three fields with their top bit: owner N - 1, type 65,535, a neighbour in block 2^22 -- seen from either end
    rs[150], rd[150], rt[150] = N1 - 1, TOP_BLOCK[0], 65535
    rs[151], rd[151], rt[151] = TOP_BLOCK[1], N1 - 1, 65535
    rs[152], rd[152], rt[152] = TOP_BLOCK[2], TOP_BLOCK[0], 0
    ei = torch.stack([torch.cat(src + [rs]), torch.cat(dst + [rd])])
    et = torch.cat(typ + [rt])
    perm = torch.randperm(int(et.numel()), generator=g)
    return ei[:, perm].contiguous(), et[perm].contiguous()


@pytest.fixture(scope="module")
def wide():
    ei, et = _wide_graph()
    initial = torch.arange(N1) % B1
    assert int(initial.max()) == B1 - 1 == 2 ** 22 and initial[list(TOP_BLOCK)].tolist() == [2 ** 22] * 3
    assert int(et.min()) == 0 and int(et.max()) == R1 - 1
    owners = set(ei.flatten().tolist())
    assert {0, 1, N1 - 1} <= owners and set(TOP_BLOCK) <= owners and 3000 <= int(et.numel()) <= 4000
    want = {d: R.node_partition_sparse(ei, et, N1, R1, k=2, direction=d, initial=initial) for d in DIRECTIONS}
    for d in DIRECTIONS:
        p = want[d]
        assert p.rounds == 2 and B1 < p.counts[0] < p.counts[1]    # round 2 propagates what round 1 split
        # both rounds run at the same key width: B still needs 23 bits going into round 2
        assert bits_for(B1 - 1) == bits_for(p.counts[0] - 1) == 23
        assert _round_key_bits(N1, R1, p.counts[0], d) == _round_key_bits(N1, R1, B1, d)
    assert [_round_key_bits(N1, R1, B1, d) for d in DIRECTIONS] == [64, 64, 65]
    assert (bits_for(N1 - 1), bits_for(R1 - 1)) == (25, 16)
    assert _ceil(N1, SCAN_BLOCK) > SCAN_BLOCK                      # the three node scans loop in scan_top_kernel
    return ei.to(DEV), et.to(DEV), initial.to(DEV), want


@pytest.mark.parametrize("route", (0, 1, 2))
@pytest.mark.parametrize("direction", ("out", "in"))
def test_round_key_of_exactly_64_bits(wide, direction, route):
    ei, et, initial, want = wide
    _same(_S().node_partition(ei, et, N1, R1, k=2, direction=direction, initial=initial, _route=route), want[direction])


@pytest.mark.parametrize("route", (0, 2))
def test_round_key_of_65_bits_takes_two_sorts(wide, route):
    ei, et, initial, want = wide
    _same(_S().node_partition(ei, et, N1, R1, k=2, direction="in_out", initial=initial, _route=route), want["in_out"])


def test_round_key_of_65_bits_refuses_the_pinned_single_sort(wide):
    ei, et, initial, _ = wide
    with pytest.raises(RuntimeError):
        _S().node_partition(ei, et, N1, R1, k=2, direction="in_out", initial=initial, _route=1)


# ---- 2. a quotient key of exactly 64 bits -------------------------------------------------------------------------------------------
def _quotient_case():
    ei, et = R.random_graph(50, 200, 65536, seed=13)
    top = 2 ** 24 - 1
    block = torch.arange(50) % 5
    block[7] = block[8] = top
    et[:40] %= 3
    et[0], et[1] = 0, 65535
    ei[:, 2], et[2] = torch.tensor([7, 8]), 65535                  # (65535, 2^24 - 1, 2^24 - 1): every bit of the key set
    ei[:, 3], ei[:, 4], ei[:, 5] = torch.tensor([7, 20]), torch.tensor([21, 8]), torch.tensor([8, 8])
    assert int(block.min()) == 0 and int(block.max()) == top and int(et.min()) == 0 and int(et.max()) == 65535
    ends = (block[ei[0]] == top).long() + (block[ei[1]] == top).long()
    assert int((ends == 2).sum()) >= 2 and int((ends == 1).sum()) >= 2 and int((ends == 0).sum()) >= 100
    return ei, et, block


def _quotient_equal(ei, et, block, num_blocks, route):
    got = _S().quotient_graph(ei.to(DEV), et.to(DEV), block.to(DEV), num_blocks, _route=route)
    want = R.quotient_graph(ei, et, block)
    assert 1 < int(want[2].max()) and int(want[2].sum()) == 200
    for a, b in zip(got, want):
        assert a.dtype == torch.int64 and torch.equal(a.cpu(), b)


@pytest.mark.parametrize("route", (0, 1, 2))
def test_quotient_key_of_exactly_64_bits(route):
    ei, et, block = _quotient_case()
    num_blocks = 2 ** 24
    assert bits_for(int(et.max())) + 2 * bits_for(num_blocks - 1) == 16 + 24 + 24 == 64
    _quotient_equal(ei, et, block, num_blocks, route)


def test_quotient_key_of_66_bits():
    ei, et, block = _quotient_case()
    num_blocks = 2 ** 24 + 1
    assert bits_for(int(et.max())) + 2 * bits_for(num_blocks - 1) == 16 + 25 + 25 == 66
    with pytest.raises(RuntimeError):
        _S().quotient_graph(ei.to(DEV), et.to(DEV), block.to(DEV), num_blocks, _route=1)
    for route in (0, 2):
        _quotient_equal(ei, et, block, num_blocks, route)


# ---- 3. node counts on either side of a power of 256 ------------------------------------------------------------------------------
R3 = 3


@functools.lru_cache(maxsize=None)
def _power_case(n, with_initial, direction):
    """the graph and the oracle's partition, made once for both routes"""
    ei, et = R.random_graph(n, 4 * n, R3, seed=n)
    ei[:, 0], ei[:, 1] = torch.tensor([n - 1, 0]), torch.tensor([1, n - 1])      # the top node owns an out- and an in-edge
    initial = torch.arange(n) if with_initial else None
    return ei, et, initial, R.node_partition(ei, et, n, R3, k=3, direction=direction, initial=initial)


@pytest.mark.parametrize("route", (1, 2))
@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("n,with_initial", ((256, False), (257, False), (257, True), (65536, False), (65537, False), (65537, True)))
def test_node_counts_at_powers_of_256(n, with_initial, direction, route):
    ei, et, initial, p = _power_case(n, with_initial, direction)
    node_bits = bits_for(n - 1)
    assert node_bits == {256: 8, 257: 9, 65536: 16, 65537: 17}[n]
    assert _ceil(node_bits, 8) == {256: 1, 257: 2, 65536: 2, 65537: 3}[n]        # passes of route 2's sort by owner
    assert n - 1 in ei[0, :2].tolist() and n - 1 in ei[1, :2].tolist()
    if with_initial:      # every node its own block from the start: the block field is as wide as the node field in round 1
        assert p.counts == (n,) and p.converged
    else:                 # the block field grows from round to round, from one bit towards the node field's width
        assert p.rounds == 3 and p.counts[0] < 256 and p.counts[0] < p.counts[1] <= p.counts[2] and p.counts[2] > n // 2
    got = _S().node_partition(ei.to(DEV), et.to(DEV), n, R3, k=3, direction=direction,
                              initial=None if initial is None else initial.to(DEV), _route=route)
    _same(got, p)


# ---- the defect case 3 found: two nodes that point at each other's block -------------------------------------------------------------
@pytest.mark.parametrize("route", (0, 1, 2))
@pytest.mark.parametrize("direction", ("out", "in"))
@pytest.mark.parametrize("rel", (0, 3))
def test_two_nodes_that_see_each_other_s_block_stay_apart(rel, direction, route):
    """0 <-> 1, each a block of its own: node 0 is (block 0, one element that reads as the integer 1), node 1 (block 1, one element
    that reads as 0) -- under relation 0 in the packed key of route 1 (type 0, block 1 / 0), under relation 0 or 3 in the ranks of
    route 2 (the two smallest elements; the self-loop of relation 5 is the third).  A signature that folds the node's block in
    with the words of the elements cannot tell the two apart and returns them as ONE block, coarser than ``initial``.  (Found at
    N = 65,536, "in", route 2, round 3 of the case above: nodes 24 and 40,957.)"""
    ei, et = torch.tensor([[0, 1, 2], [1, 0, 2]]), torch.tensor([rel, rel, 5])
    initial = torch.tensor([0, 1, 2, 2])
    want = R.node_partition(ei, et, 4, 6, k=2, direction=direction, initial=initial)
    assert want.block.tolist() == [0, 1, 2, 3] and want.counts == (4, 4)
    _same(_S().node_partition(ei.to(DEV), et.to(DEV), 4, 6, k=2, direction=direction, initial=initial.to(DEV), _route=route), want)


# ---- 4. node counts on either side of one scan workgroup ----------------------------------------------------------------------------
@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("n", (2048, 2049))
def test_node_scans_at_and_past_one_workgroup(n, direction):
    assert _ceil(n, SCAN_BLOCK) == (1 if n == 2048 else 2)
    ei, et = R.random_graph(n, 3 * n, 4, seed=n)
    ei[:, 0], ei[:, 1] = torch.tensor([n - 1, 0]), torch.tensor([1, n - 1])
    want = R.node_partition(ei, et, n, 4, k=None, direction=direction)
    assert want.converged and want.rounds >= 3 and want.num_blocks > n // 2
    _same(_S().node_partition(ei.to(DEV), et.to(DEV), n, 4, k=None, direction=direction), want)
