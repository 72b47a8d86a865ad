"""``sampling.NeighborSampler`` (csrc/rgcn_sample.hip and the sort and scan of csrc/rgcn_sort_scan.h it drives) where
tests/test_gpu_sampling.py stops, every block and index EQUAL to tests/sampling_reference.py: fan-outs that fill the second, third
and fourth register of the Floyd wave (127 .. 255 against in-degrees k and k + 1 and a hub of 70,000, seeds 0 and 2^63 - 1); a bit
set of exactly 2,047 and 2,048 words, whose scan ends on a workgroup's last entry or alone in a second workgroup, with node 0 and
node N - 1 as new sources; one graph of 2^24 + 5 nodes and 4 x 2^20 + 2,049 edges (four sort passes, five trips of the scan's carry
loop, the second trip of the edge kernels' stride loop, a hub of 3,000,000 in-edges sampled); and the sort at E = 1, 2 and either
side of one and four 2,048-key segments.  Every case asserts on the host the property that makes it an edge."""
import pytest
import torch

from tests import sampling_reference as R
from tests.test_gpu_sampling import _same

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCAN_BLOCK, SEG_KEYS, EDGE_THREADS = 2048, 2048, 16384 * 256      # rgcn_sort_scan.h kScanBlock, kSegKeys; kEdgeGridMax x 256
SEED_MAX = 2 ** 63 - 1


def bits_for(max_value):
    """rgcn_sort_scan.h bits_for: bits that hold 0 .. max_value, at least 1"""
    return max(1, int(max_value).bit_length())


def _ceil(a, b):
    return -(-a // b)


def _sampler(ei, et, n, r):
    from scaling_rgcn_training_amd.sampling import NeighborSampler
    return NeighborSampler(ei.to(DEV), et.to(DEV), n, r)


def _index_equal(sampler, ix):
    ptr, src, typ = sampler._arrays
    e = int(ix.src.shape[0])
    assert torch.equal(ptr.cpu().long(), ix.ptr), "ptr"
    assert torch.equal(src[:e].cpu().long(), ix.src) and torch.equal(typ[:e].cpu().long(), ix.type), "src / type"


def _clean(sampler):
    assert bool((sampler._map == -1).all()), "the node map was not reset"


# ---- 1. the register ladder of hop_floyd_kernel ---------------------------------------------------------------------------------
N1, NREL1, HUB1, REST1 = 4200, 5, 70000, 6000
# node 0: the hub; nodes 1 .. 15: the in-degrees either side of 128, 192 and 256; node 16 and the last three: no in-edge
DEGREES1 = (HUB1, 126, 127, 128, 129, 130, 190, 191, 192, 193, 194, 254, 255, 256, 257, 258)
FANOUTS1 = (127, 128, 129, 191, 192, 193, 255)
NDST1 = (1, 2047, 2048)


def _ladder_graph():
    g = torch.Generator().manual_seed(17)
    dst = torch.cat([torch.full((d,), v, dtype=torch.int64) for v, d in enumerate(DEGREES1)])
    dst = torch.cat([dst, torch.randint(17, N1 - 3, (REST1,), generator=g)])
    e = int(dst.numel())
    dst = dst[torch.randperm(e, generator=g)]                      # a node's in-edges are scattered over the input
    src = torch.randint(0, N1, (e,), generator=g)
    typ = torch.randint(0, NREL1 - 1, (e,), generator=g)           # the last relation is empty
    src[:40] = dst[:40]                                            # self loops
    hub = torch.nonzero(dst == 0).flatten()                        # repeated triples, among the hub's in-edges
    src[hub[:40]], typ[hub[:40]] = src[hub[40:80]], typ[hub[40:80]]
    deg = torch.bincount(dst, minlength=N1)
    assert deg[:16].tolist() == list(DEGREES1) and int(deg[16]) == 0 and not bool(deg[-3:].any())
    return torch.stack([src, dst]), typ


@pytest.fixture(scope="module")
def ladder():
    ei, et = _ladder_graph()
    ix = R.build_index(ei, et, N1)
    g = torch.Generator().manual_seed(3)
    special = torch.arange(17)
    others = 17 + torch.randperm(N1 - 17, generator=g)
    dsts = {1: torch.tensor([0])}
    for n in NDST1[1:]:
        dsts[n] = torch.cat([special, others[:n - 17]])[torch.randperm(n, generator=g)]
    return ix, _sampler(ei, et, N1, NREL1), dsts


def test_the_ladder_covers_two_three_and_four_registers():
    assert sorted({_ceil(k, 64) for k in FANOUTS1}) == [2, 3, 4]
    # a full second / third register (k = 128 / 192), one slot in the third / fourth (129 / 193), one free in each (127, 191, 255)
    assert {k % 64 for k in FANOUTS1} == {63, 0, 1}
    assert [_ceil(n + 1, SCAN_BLOCK) for n in NDST1] == [1, 1, 2] and NDST1[1] + 1 == SCAN_BLOCK


@pytest.mark.parametrize("n_dst", NDST1)
@pytest.mark.parametrize("k", FANOUTS1)
def test_fanouts_in_the_second_third_and_fourth_register(ladder, k, n_dst):
    ix, sampler, dsts = ladder
    dst = dsts[n_dst]
    deg = (ix.ptr[dst + 1] - ix.ptr[dst]).tolist()
    assert max(deg) > 2 ** 16 > k                                  # the hub is sampled: draws with j past 16 bits
    if n_dst > 1:
        assert k in deg and k + 1 in deg and 0 in deg              # taken whole at d = k, sampled at k + 1, nothing at 0
    for seed, hop in ((0, 0), (SEED_MAX, 1)):
        want = R.sample_block(ix, dst, k, seed, hop)
        # a one-layer call samples hop 0; hop 1 is the second layer of a two-layer call whose first takes everything
        if hop == 0:
            got = sampler.sample(dst.to(DEV), (k,), seed)[0]
        else:
            got = sampler.sample(dst.to(DEV), (-1, k), seed)[1]
        assert int(want.edge_type.numel()) == sum(min(d, k) for d in deg)
        _same(got, want, f"k={k} n_dst={n_dst} seed={seed} hop={hop}")
    _clean(sampler)


# ---- 2. the bit set's scan at one workgroup exactly and one entry past it ---------------------------------------------------------
E2, NREL2 = 3000, 4
DST2 = torch.arange(100, 140)                                      # 40 destinations; no source lies in 100 .. 139


def _bitset_graph(n):
    """destinations 100 .. 105 have three in-edges or fewer (taken whole by either fan-out) from nodes 0, 31, 32, n - 2, n - 1 and
    both sides of several word boundaries; the other 34 share random sources, about 85 each"""
    g = torch.Generator().manual_seed(n)
    forced = sorted({0, 31, 32, n - 2, n - 1, 63, 64, 1023, 1024, 32767, 32768, 65471, 65472, 65503, n - 33, n - 32})
    f_src = torch.tensor(forced)
    f_dst = 100 + torch.arange(len(forced)) // 3
    rest = E2 - len(forced)
    r_src = torch.randint(0, n, (rest,), generator=g)
    r_src[(r_src >= 100) & (r_src < 140)] += 1000
    r_dst = torch.randint(106, 140, (rest,), generator=g)
    perm = torch.randperm(E2, generator=g)
    ei = torch.stack([torch.cat([f_src, r_src]), torch.cat([f_dst, r_dst])])[:, perm]
    return ei, torch.randint(0, NREL2, (E2,), generator=g), forced


@pytest.mark.parametrize("n,scan_len", ((65504, 2048), (65505, 2049)))
def test_bit_set_scan_at_and_past_one_workgroup(n, scan_len):
    ei, et, forced = _bitset_graph(n)
    n_words = _ceil(n, 32)
    assert n_words + 1 == scan_len and _ceil(scan_len, SCAN_BLOCK) == (1 if n == 65504 else 2)
    assert (n % 32 == 0) == (n == 65504)                           # a full last word / a last word of one node
    # (both sizes are below 65,536, so the index sorts in two passes: test_index_sort_passes_at_powers_of_256 has the third)
    assert bits_for(n - 1) == 16
    ix = R.build_index(ei, et, n)
    sampler = _sampler(ei, et, n, NREL2)
    _index_equal(sampler, ix)
    dst = DST2[torch.randperm(40, generator=torch.Generator().manual_seed(1))]
    assert not bool(torch.isin(ei[0], dst).any())                  # every source is a new source
    for k in (-1, 3):
        want = R.sample_block(ix, dst, k, 5, 0)
        new = set(want.src_nodes[40:].tolist())
        assert set(forced) <= new and {0, n - 1} <= new
        if k == 3:
            assert int(want.edge_type.numel()) < E2                # the other destinations are sampled
        _same(sampler.sample(dst.to(DEV), (k,), 5)[0], want, f"N={n} k={k}")
        _clean(sampler)


@pytest.mark.parametrize("n", (256, 257, 65536, 65537))
def test_index_sort_passes_at_powers_of_256(n):
    """the index sorts over bits_for(N - 1) bits: the last N of one and two passes, the first of two and three, with in-edges on
    the top node (its key alone has the new digit) and the top node among the sources"""
    assert _ceil(bits_for(n - 1), 8) == {256: 1, 257: 2, 65536: 2, 65537: 3}[n]
    g = torch.Generator().manual_seed(n)
    e = 4 * n if n < 1000 else 6000
    ei = torch.randint(0, n, (2, e), generator=g)
    ei[1, 10:13], ei[0, 13] = n - 1, n - 1
    ei[0, 10] = 0
    et = torch.randint(0, 3, (e,), generator=g)
    ix = R.build_index(ei, et, n)
    assert int(ix.ptr[n] - ix.ptr[n - 1]) >= 3
    sampler = _sampler(ei, et, n, 3)
    _index_equal(sampler, ix)
    dst = torch.cat([torch.tensor([n - 1]), 1 + torch.randperm(n - 2, generator=g)[:64]])      # 65 distinct, node 0 not among them
    want = R.sample_block(ix, dst, -1, 8, 0)
    assert int(want.src_nodes[65]) == 0                            # node 0, a source of the top node, is the first new source
    _same(sampler.sample(dst.to(DEV), (-1,), 8)[0], want, f"N={n}")
    _clean(sampler)


# ---- 3. one large graph -----------------------------------------------------------------------------------------------------------
N3, NREL3, E3, HUB3, NDST3 = 2 ** 24 + 5, 7, 4 * 2 ** 20 + 2049, 3_000_000, 400


@pytest.fixture(scope="module")
def large():
    g = torch.Generator().manual_seed(29)
    others = 1 + torch.randperm(N3 - 2, generator=g)[:NDST3]       # in [1, N - 2]
    others[0], others[1] = 2 ** 24, 33                             # a destination whose id needs the 25th bit
    others = torch.unique(others)
    rest = E3 - HUB3 - 2
    dst = torch.cat([torch.zeros(HUB3, dtype=torch.int64), others[torch.randint(0, int(others.numel()), (rest,), generator=g)],
                     torch.tensor([N3 - 1, N3 - 1])])
    src = torch.randint(0, N3, (E3,), generator=g)
    src[:5] = torch.tensor([0, 31, 32, N3 - 2, N3 - 1])
    src[HUB3:HUB3 + 5] = torch.tensor([0, 31, 32, N3 - 2, N3 - 1])
    perm = torch.randperm(E3, generator=g)
    ei = torch.stack([src, dst])[:, perm]
    et = torch.randint(0, NREL3, (E3,), generator=g)
    ix = R.build_index(ei, et, N3)
    deg = ix.ptr[1:] - ix.ptr[:-1]
    seeds = torch.nonzero(deg).flatten()                           # every node that has an in-edge
    seeds = seeds[torch.randperm(int(seeds.numel()), generator=g)]
    assert int(deg[0]) == HUB3 and int(deg[N3 - 1]) == 2 and 395 <= int(seeds.numel()) - 2 <= NDST3
    assert int(deg[others].min()) > 256                            # all but node N - 1 are sampled at every fan-out
    return ix, _sampler(ei, et, N3, NREL3), seeds


def test_large_index_four_sort_passes_and_the_scan_carry(large):
    ix, sampler, _ = large
    assert bits_for(N3 - 1) == 25 and _ceil(25, 8) == 4
    scan_groups = _ceil(N3 + 1, SCAN_BLOCK)
    assert scan_groups == 8193 and _ceil(scan_groups, SCAN_BLOCK) == 5      # trips of scan_top_kernel's carry loop
    assert _ceil(E3, SEG_KEYS) == 2050
    _index_equal(sampler, ix)


def test_large_take_all_strides_the_edge_kernels(large):
    ix, sampler, seeds = large
    want = R.sample_block(ix, seeds, -1, 0, 0)
    assert int(want.edge_type.numel()) == E3 > EDGE_THREADS        # some threads of expand and relabel take a second edge
    assert _ceil(_ceil(N3, 32) + 1, SCAN_BLOCK) == 257
    # (0 and N - 1 are destinations; as sources they are relabelled through the destinations' map entries)
    assert bool(torch.isin(torch.tensor([31, 32, N3 - 2]), want.src_nodes[seeds.numel():]).all())
    _same(sampler.sample(seeds.to(DEV), (-1,), 0)[0], want, "take all")
    _clean(sampler)


@pytest.mark.parametrize("k,seed", ((129, SEED_MAX), (256, 7)))
def test_large_hub_of_three_million_sampled(large, k, seed):
    ix, sampler, seeds = large
    want = R.sample_block(ix, seeds, k, seed, 0)
    assert int(want.edge_type.numel()) == (int(seeds.numel()) - 1) * k + 2
    _same(sampler.sample(seeds.to(DEV), (k,), seed)[0], want, f"k={k}")
    _clean(sampler)


# ---- 4. the sort's early return and its segment edges in this translation unit ------------------------------------------------------
N4, NREL4 = 300, 3


@pytest.mark.parametrize("e", (1, 2, 2047, 2048, 2049, 8192, 8193))
def test_sort_segment_edges(e):
    assert _ceil(e, SEG_KEYS) == {1: 1, 2: 1, 2047: 1, 2048: 1, 2049: 2, 8192: 4, 8193: 5}[e]
    g = torch.Generator().manual_seed(e)
    ei = torch.randint(0, N4, (2, e), generator=g)
    et = torch.randint(0, NREL4, (e,), generator=g)
    ix = R.build_index(ei, et, N4)
    sampler = _sampler(ei, et, N4, NREL4)
    _index_equal(sampler, ix)
    dst = torch.cat([ei[1, :1], torch.randperm(N4, generator=g)])
    dst = dst[torch.cat([torch.tensor([True]), dst[1:] != dst[0]])][:65]      # 65 distinct, the first one with an in-edge
    want = R.sample_block(ix, dst, 2, 4, 0)
    assert int(want.edge_type.numel()) >= 1
    _same(sampler.sample(dst.to(DEV), (2,), 4)[0], want, f"E={e}")
    _clean(sampler)
