"""numpy twin of csrc/rgcn_transfer.hip, written from the contract in include/rgcn_mi355x.h (not from the kernels): the fractional
labels of a node partition (integer sums, double quotient, one rounding to float32), the uniform draw of an unmapped node (wrapping
u64 arithmetic) and the three gather modes."""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
MODES = ("stack", "concat", "sum")


def mix(z):
    """splitmix64's finaliser on uint64 arrays (wrapping)"""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def draw(seed, s, nodes, width):
    """float32 [len(nodes), width]: value(seed, s, node, col) = (mix(mix(seed + GOLDEN (s + 1)) + node width + col) >> 40) 2^-24"""
    nodes = np.asarray(nodes, dtype=np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        key = mix(np.uint64(seed) + GOLDEN * np.uint64(s + 1))
        ctr = key + nodes[:, None] * np.uint64(width) + np.arange(width, dtype=np.uint64)[None, :]
    bits = mix(ctr) >> np.uint64(40)
    return (bits.astype(np.float64) * 2.0 ** -24).astype(np.float32)      # (24 bits: exact in either format)


def block_labels(block, num_blocks, train_idx, y):
    """(size int32 [B], y_sum float32 [B, C], nonzero int32 [B]); ids out of range are skipped"""
    block, train_idx, y = (np.asarray(a, dtype=np.int64) for a in (block, train_idx, y))
    n, c = block.shape[0], y.shape[1]
    ok = (block >= 0) & (block < num_blocks)
    size = np.bincount(block[ok], minlength=num_blocks).astype(np.int64)
    cnt = np.zeros((num_blocks, c), dtype=np.int64)
    good = (train_idx >= 0) & (train_idx < n)
    rows = np.nonzero(good)[0]
    b = block[train_idx[rows]]
    keep = (b >= 0) & (b < num_blocks)
    np.add.at(cnt, b[keep], y[rows[keep]])
    y_sum = (cnt.astype(np.float64) / np.maximum(1, size).astype(np.float64)[:, None]).astype(np.float32)
    return size.astype(np.int32), y_sum, (cnt.sum(1) != 0).astype(np.int32)


def summary_labels(block, num_blocks, train_idx, y):
    """(x_train_sum, y_train_sum, size) as transfer.summary_labels returns them"""
    size, y_sum, nonzero = block_labels(block, num_blocks, train_idx, y)
    x = np.nonzero(nonzero)[0].astype(np.int64)
    return x, y_sum[x], size


def pieces(tables, maps, num_nodes, nodes, seed):
    """the S pieces [M, E] of the nodes `nodes` (None: all): table row, draw where the map says -1, zeros where an id is out of range"""
    width = tables[0].shape[1]
    nodes = np.arange(num_nodes, dtype=np.int64) if nodes is None else np.asarray(nodes, dtype=np.int64)
    node_ok = (nodes >= 0) & (nodes < num_nodes)
    safe = np.where(node_ok, nodes, 0)
    out = []
    for s, (t, m) in enumerate(zip(tables, maps)):
        t, m = np.asarray(t, dtype=np.float32), np.asarray(m, dtype=np.int64)
        row = m[safe] if num_nodes else np.zeros(0, dtype=np.int64)
        piece = np.zeros((nodes.shape[0], width), dtype=np.float32)
        mapped = node_ok & (row >= 0) & (row < t.shape[0])
        piece[mapped] = t[row[mapped]]
        fill = node_ok & (row == -1)
        piece[fill] = draw(seed, s, nodes[fill], width)
        out.append(piece)
    return out


def gather(tables, maps, num_nodes, nodes, mode, seed):
    return combine(pieces(tables, maps, num_nodes, nodes, seed), mode)


def combine(ps, mode):
    """the S pieces as one tensor: [S, M, E], [M, S E] or [M, E]"""
    if mode == "stack":
        return np.stack(ps)
    if mode == "concat":
        return np.concatenate(ps, axis=1)
    acc = np.zeros_like(ps[0])
    for p in ps:      # ((0 + t_0) + t_1) + ... in float32: Python's sum(list)
        acc = acc + p
    return acc
