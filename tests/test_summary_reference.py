"""The summary oracle (tests/summary_reference.py) on graphs worked by hand.  CPU only."""
import pytest
import torch

from tests import summary_reference as R


def test_directed_path_splits_one_node_per_round():
    """0 -> 1 -> ... -> 9, "out": round 1 splits off the node without an out-edge, every further round the node in front of the
    last one split off: min(j + 1, 10) blocks after round j, and round 10 -- the round after the last split -- finds nothing"""
    ei, et = R.path_graph(10)
    for j in range(1, 13):
        p = R.node_partition(ei, et, 10, 1, k=j, direction="out")
        assert p.counts == tuple(min(i + 1, 10) for i in range(1, min(j, 10) + 1))
        assert p.num_blocks == min(j + 1, 10) and p.rounds == min(j, 10) and p.converged == (j >= 10)
    full = R.node_partition(ei, et, 10, 1, k=None, direction="out")
    assert full.rounds == 10 and full.converged and full.block.tolist() == list(range(10))
    assert R.node_partition(ei, et, 10, 1, k=None, direction="out", max_rounds=9).converged is False
    # after two rounds: {0..7}, {8}, {9}, numbered by smallest member
    assert R.node_partition(ei, et, 10, 1, k=2).block.tolist() == [0] * 8 + [1, 2]


def test_duplicate_edge_does_not_split():
    ei = torch.tensor([[0, 1, 1], [2, 2, 2]])
    et = torch.zeros(3, dtype=torch.int64)
    p = R.node_partition(ei, et, 3, 1, k=3, direction="out")
    assert p.block.tolist() == [0, 0, 1] and p.converged
    # ... but another relation does
    et2 = torch.tensor([0, 0, 1])
    assert R.node_partition(ei, et2, 3, 2, k=1, direction="out").block.tolist() == [0, 1, 2]


def test_in_out_keeps_the_direction_of_an_element():
    """node 0 has only an outgoing type-0 edge, node 3 only an incoming one: equal as sets of (type, block), different with the
    direction bit.  (0 -> 1, 2 -> 3: the other ends mirror them.)"""
    ei = torch.tensor([[0, 2], [1, 3]])
    et = torch.zeros(2, dtype=torch.int64)
    p = R.node_partition(ei, et, 4, 1, k=1, direction="in_out")
    assert p.block.tolist() == [0, 1, 0, 1]
    assert R.node_partition(ei, et, 4, 1, k=1, direction="out").block.tolist() == [0, 1, 0, 1]
    assert R.node_partition(ei, et, 4, 1, k=1, direction="in").block.tolist() == [0, 1, 0, 1]
    # a self-loop is an ordinary edge: out AND in element on one node
    p = R.node_partition(torch.tensor([[0, 1], [0, 2]]), et, 3, 1, k=1, direction="in_out")
    assert p.block.tolist() == [0, 1, 2]


def test_initial_is_respected_and_only_refined():
    ei, et = R.path_graph(4)
    # without edges in common, 0 and 1 would stay together for one round; the initial partition separates them from the start
    init = torch.tensor([7, 3, 7, 7])
    p = R.node_partition(ei, et, 4, 1, k=1, direction="out", initial=init)
    # blocks of `init`: {0, 2, 3} and {1}; round 1: 0 sees block of 1, 2 sees block of 3 (= its own), 3 sees nothing
    assert p.block.tolist() == [0, 1, 2, 3]
    q = R.node_partition(torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 4, 1, k=5, initial=init)
    assert q.block.tolist() == [0, 1, 0, 0] and q.rounds == 1 and q.converged and q.counts == (2,)
    # every block of the result lies inside one block of `initial`
    ei, et = R.random_graph(40, 120, 3, seed=2)
    init = torch.arange(40) % 3
    p = R.node_partition(ei, et, 40, 3, k=2, direction="in_out", initial=init)
    for b in range(p.num_blocks):
        assert len(set(init[p.block == b].tolist())) == 1


def test_quotient_counts_and_order():
    ei = torch.tensor([[0, 1, 2, 2, 0], [2, 2, 0, 0, 2]])
    et = torch.tensor([1, 1, 0, 0, 1])
    block = torch.tensor([0, 0, 1])
    qi, qt, qm = R.quotient_graph(ei, et, block)
    assert qi.tolist() == [[1, 0], [0, 1]] and qt.tolist() == [0, 1] and qm.tolist() == [2, 3]


def _equal(a, b, what):
    assert a.block.dtype == b.block.dtype == torch.int64 and torch.equal(a.block, b.block), what
    assert (a.num_blocks, a.rounds, a.counts, a.converged) == (b.num_blocks, b.rounds, b.counts, b.converged), what


@pytest.mark.parametrize("direction", ("out", "in", "in_out"))
@pytest.mark.parametrize("k", (1, 3, None))
def test_the_sparse_oracle_equals_the_set_oracle(direction, k):
    """graphs where most nodes own no edge (the form tests/test_gpu_summary_edges.py uses at 2^24 nodes), with and without an
    initial partition whose ids are neither dense nor in canonical order; then the path and the hub graph"""
    for seed, (n, pool, e, r) in enumerate(((600, 40, 150, 3), (900, 25, 60, 2), (70, 70, 200, 5))):
        g = torch.Generator().manual_seed(seed)
        nodes = torch.randperm(n, generator=g)[:pool]
        nodes[0], nodes[1] = 0, n - 1                                    # (twice in the pool at worst)
        ei = nodes[torch.randint(0, pool, (2, e), generator=g)]
        et = torch.randint(0, r, (e,), generator=g)
        ei[:, :5] = ei[:, 5:10]                                          # duplicate edges
        et[:5] = et[5:10]
        ei[1, 10:14] = ei[0, 10:14]                                      # self-loops
        initial = 9 - torch.arange(n) % 7 * 3 % 10
        for init in (None, initial):
            want = R.node_partition(ei, et, n, r, k=k, direction=direction, initial=init)
            _equal(R.node_partition_sparse(ei, et, n, r, k=k, direction=direction, initial=init), want, (seed, init is None))
        assert want.num_blocks > 7                                       # the edges split the initial blocks
    ei, et = R.path_graph(10)
    _equal(R.node_partition_sparse(ei, et, 10, 1, k=k, direction=direction),
           R.node_partition(ei, et, 10, 1, k=k, direction=direction), "path")
    _equal(R.node_partition_sparse(ei, et, 10, 1, k=None, direction=direction, max_rounds=6),
           R.node_partition(ei, et, 10, 1, k=None, direction=direction, max_rounds=6), "path, cut short")
    ei, et, n, init, _ = R.hub_graph(deg=50, lead=5)
    _equal(R.node_partition_sparse(ei, et, n, 1, k=k, direction=direction, initial=init),
           R.node_partition(ei, et, n, 1, k=k, direction=direction, initial=init), "hub")


def test_hub_graph_is_what_it_says():
    ei, et, n, init, (h1, h2, h3) = R.hub_graph(deg=50, lead=5)
    p = R.node_partition(ei, et, n, 1, k=1, direction="out", initial=init)
    assert p.block[h1] == p.block[h3] != p.block[h2]
    assert int((ei[0] == h3).sum()) > int((ei[0] == h1).sum()) == 50
