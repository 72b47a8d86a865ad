"""The two rows kernels (csrc/rgcn_rows.hip, csrc/rgcn_dw_root.hip) past their first trip: tests/test_gpu_bipartite.py stops at 20,000 rows, where every wave
of both kernels makes exactly one trip through its loop.  Here the row counts are the smallest at which

  rgcn_rows_transform_kernel   (at most kRowsTfMaxBlocks = 512 workgroups of kRowsTfWaves = 8 waves, 16 rows per wave and trip: a
                               second trip above 65,536 rows) consumes its look-ahead registers (KT <= 4) or reloads (KT = 8),
                               reaches a partial last tile on a later trip and reads ``add`` aliased to ``y`` across trips;
  rgcn_dw_root_kernel<false>   (rgcn_rows_dw: ranges of ceil(ksteps / 16) k-steps until 2048 / nq ranges are reached: a second trip of the double
                               batch above 131,072 / 65,536 / 32,768 rows at nq = 1 / 2 / 4) runs its second load_batch(0) /
                               compute_batch(1) round on the running 32-bit offsets, over ranges that are no multiple of 16
                               k-steps, and the reduce kernel folds 512, 1024 and 2048 slabs per quadrant.

Every case computes the trip counts it claims from the host code's formulas and asserts them BEFORE launching: a change of a
constant that lets a case drift back to one trip fails here.  Reference: plain torch float64 on the device (x @ W, x^T g, the
condition the same products on absolute values), judged by bound (1) of oracle/tolerance.py; never another kernel.

rgcn_rows_dw and rgcn_bwd_dw_root are two instantiations of ONE kernel template with one reduce kernel behind them: the last test
holds them to the same bits wherever both apply and cut the rows into the same ranges."""
import pytest
import torch

from tests.test_gpu_bipartite import _bound1, _padded

pytestmark = pytest.mark.gpu

# csrc/rgcn_rows.hip: kRowsTfMaxBlocks, kRowsTfWaves (= kRowsTfThreads / 64); csrc/rgcn_dw_root.hip: kDwRootBatch.  kRowsDwMaxWaves is
# read from the library (the workspace holds one 64 x 64 slab of floats per wave).
TF_MAX_BLOCKS, TF_WAVES, DW_BATCH = 512, 8, 8

# rows -> (transform trips per wave (min, max), {nq: d_w trips per range (min, max)})
ROWS = {
    66_565: ((1, 2), {1: (1, 1), 2: (1, 2), 4: (2, 3)}),            # the partial last tile (5 rows) falls on a second trip
    133_125: ((2, 3), {1: (1, 2), 2: (2, 3), 4: (5, 5)}),
    300_007: ((4, 5), {1: (3, 3), 2: (5, 5), 4: (10, 10)}),         # ranges of 36..37 / 73..74 / 146..147 k-steps
}
# (din, dout): KT = 1, nq = 2 | KT = 2 | KT = 4, nq = 1 | KT = 8 | nq = 2 | KT = 8, nq = 4, LDS above 64 KiB
WIDTHS = [(5, 128), (20, 7), (64, 64), (65, 63), (128, 5), (128, 128)]
KT = {(5, 128): 1, (20, 7): 2, (64, 64): 4, (65, 63): 8, (128, 5): 8, (128, 128): 8}
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from scaling_rgcn_training_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def transform_trips(rows):
    """(min, max) trips of a wave of rgcn_rows_transform_kernel that has a tile at all, and the wave and trip of the last tile"""
    tiles = (rows + 15) // 16
    blocks = min(TF_MAX_BLOCKS, (tiles + TF_WAVES - 1) // TF_WAVES)
    step = blocks * TF_WAVES
    trips = [(tiles - w + step - 1) // step for w in range(min(step, tiles))]
    return (min(trips), max(trips)), ((tiles - 1) % step, (tiles - 1) // step + 1)


def dw_ranges(rows, nq, max_waves):
    """(parts, [k-steps of every range]) of rgcn_rows_dw"""
    ksteps = (rows + 3) // 4
    want = (ksteps + 2 * DW_BATCH - 1) // (2 * DW_BATCH)
    parts = min(want, max_waves // nq)
    return parts, [ksteps * (p + 1) // parts - ksteps * p // parts for p in range(parts)]


def dw_trips(lengths):
    t = [(n + 2 * DW_BATCH - 1) // (2 * DW_BATCH) for n in lengths]
    return min(t), max(t)


def test_the_row_counts_are_the_smallest_of_their_regime(dev):
    """one row fewer than 65,537 / 131,073 / 65,537 / 32,769 and every wave of the kernel makes one trip"""
    from scaling_rgcn_training_amd import _lib
    max_waves = _lib.load().rgcn_rows_dw_workspace_bytes(64, 64) // (4 * 64 * 64)
    assert max_waves == 2048
    assert transform_trips(TF_MAX_BLOCKS * TF_WAVES * 16)[0] == (1, 1) and transform_trips(TF_MAX_BLOCKS * TF_WAVES * 16 + 1)[0] == (1, 2)
    for nq in (1, 2, 4):
        edge = max_waves // nq * 2 * DW_BATCH * 4
        assert dw_trips(dw_ranges(edge, nq, max_waves)[1]) == (1, 1) and dw_trips(dw_ranges(edge + 1, nq, max_waves)[1]) == (1, 2)
    assert transform_trips(20_000)[0] == (1, 1) and all(dw_trips(dw_ranges(20_000, nq, max_waves)[1]) == (1, 1) for nq in (1, 2, 4))


@pytest.mark.parametrize("din,dout", WIDTHS)
@pytest.mark.parametrize("rows", list(ROWS))
def test_rows_transform_past_the_first_trip(dev, rows, din, dout):
    from scaling_rgcn_training_amd import _lib
    # ---- the regime
    trips, (last_wave, last_trip) = transform_trips(rows)
    assert trips == ROWS[rows][0], (rows, trips)
    assert trips[1] >= 2 and rows % 16 != 0 and last_trip == trips[1], "a partial last tile, reached on the last trip"
    assert {16: 1, 32: 2, 64: 4, 128: 8}[_lib.load().rgcn_padded_width(din)] == KT[(din, dout)]
    print(f"\nrows_transform {rows}x{din}x{dout}: KT {KT[(din, dout)]}, trips per wave {trips}, last tile on wave {last_wave} trip {last_trip}")
    # ---- inputs and the float64 reference (one per case; W is the same matrix in both orientations)
    gen = torch.Generator().manual_seed(rows + din * 131 + dout)
    d4 = (dout + 3) // 4 * 4
    x = _padded(rows, din, 8, dev, gen)
    w = torch.randn(din, dout, generator=gen).to(dev)
    wt = w.t().contiguous()
    bias = torch.randn(dout, generator=gen).to(dev)
    add0 = _padded(rows, dout, 4, dev, gen)
    add0[:, d4:] = 7.0
    base = x[:, :din].double() @ w.double()
    base_c = x[:, :din].double().abs() @ w.double().abs()
    a64 = add0[:, :dout].double()
    for transpose in (False, True):
        for add_mode in ("none", "separate", "alias"):
            for with_bias in (False, True):
                add = None if add_mode == "none" else add0.clone()
                y = add if add_mode == "alias" else torch.full((rows, d4 + 4), NAN, device=dev)
                b = bias if with_bias else None
                res = _lib.rows_transform(x, din, wt if transpose else w, dout, transpose=transpose, add=add, bias=b, y=y)
                assert res is y
                ref, cond = base, base_c
                if add is not None:
                    ref, cond = ref + a64, cond + a64.abs()
                if with_bias:
                    ref, cond = ref + bias.double(), cond + bias.double().abs()
                tag = f"rows_transform {rows}x{din}x{dout} t={transpose} add={add_mode} bias={with_bias}"
                _bound1(y[:, :dout], ref, cond, tag)
                padc = y[:, dout:d4]
                assert not bool(padc.any()) and not bool(torch.signbit(padc).any()), tag                 # +0.0
                beyond = y[:, d4:]
                assert bool((beyond == 7.0).all() if add_mode == "alias" else beyond.isnan().all()), tag   # untouched
                if add_mode == "separate":
                    assert torch.equal(add, add0), tag                                                   # read only
                if add_mode != "none" and with_bias:
                    add2 = add0.clone()
                    y2 = add2 if add_mode == "alias" else torch.full_like(y, NAN)
                    _lib.rows_transform(x, din, wt if transpose else w, dout, transpose=transpose, add=add2, bias=b, y=y2)
                    assert torch.equal(y[:, :d4], y2[:, :d4]), tag                                       # bit-reproducible


@pytest.mark.parametrize("din,dout", WIDTHS)
@pytest.mark.parametrize("rows", list(ROWS))
def test_rows_dw_past_the_first_trip(dev, rows, din, dout):
    from scaling_rgcn_training_amd import _lib
    lib = _lib.load()
    # ---- the regime
    ws_bytes = lib.rgcn_rows_dw_workspace_bytes(din, dout)
    max_waves = ws_bytes // (4 * 64 * 64)                        # kRowsDwMaxWaves: one 64 x 64 slab of floats per wave
    nq = ((din + 63) // 64) * ((dout + 63) // 64)
    parts, lengths = dw_ranges(rows, nq, max_waves)
    trips = dw_trips(lengths)
    assert trips == ROWS[rows][1][nq], (rows, nq, trips)
    if rows == 300_007:
        assert parts == max_waves // nq and parts in (512, 1024, 2048) and all(n % (2 * DW_BATCH) for n in lengths)
        assert (min(lengths), max(lengths)) == {1: (36, 37), 2: (73, 74), 4: (146, 147)}[nq]
    print(f"\nrows_dw {rows}x{din}x{dout}: nq {nq}, {parts} ranges of {min(lengths)}..{max(lengths)} k-steps, trips {trips}")
    # ---- inputs, the float64 reference
    gen = torch.Generator().manual_seed(rows + din * 137 + dout)
    x = _padded(rows, din, 8, dev, gen)
    g = _padded(rows, dout, 4, dev, gen)
    ref = x[:, :din].double().t() @ g[:, :dout].double()
    cond = x[:, :din].double().abs().t() @ g[:, :dout].double().abs()
    runs = []
    for _ in range(2):
        # d_w is dense: written into the head of a longer buffer, the floats behind it stay.  The workspace starts as NaN: a slab the
        # reduce kernel reads and no wave wrote would show in d_w
        buf = torch.full((din * dout + 64,), 7.0, device=dev)
        ws = torch.full((ws_bytes // 4,), NAN, device=dev)
        _lib.check(lib.rgcn_rows_dw(x.data_ptr(), x.stride(0), din, g.data_ptr(), g.stride(0), dout, rows, ws.data_ptr(), ws_bytes,
                                    buf.data_ptr(), torch.cuda.current_stream().cuda_stream), "rgcn_rows_dw")
        assert bool((buf[din * dout:] == 7.0).all())
        runs.append(buf[:din * dout].view(din, dout))
    _bound1(runs[0], ref, cond, f"rows_dw {rows}x{din}x{dout}")
    assert torch.equal(runs[0], runs[1]), "bit-reproducible"
    assert torch.equal(_lib.rows_dw(x, din, g, dout), runs[0]), "the binding's own call"


@pytest.mark.parametrize("din,dout", [(64, 64), (61, 3), (4, 64), (33, 20)])
@pytest.mark.parametrize("rows", [259, 4099, 65_536])
def test_rows_dw_is_the_root_kernel(dev, rows, din, dout):
    """rgcn_rows_dw and rgcn_bwd_dw_root run one kernel template and one reduce kernel: up to 64 columns per side (one quadrant) and
    where both cut the rows into the same ranges -- min(want, 2048) against clamp(want, 4, 1024), want = ceil(ksteps / 16) -- the two
    products are the same bits.  259 rows: five ranges, the last k-step three rows past the end; 65,536: exactly the root entry's
    cap of 1024 ranges.  The widths leave partial 16-byte pieces and lanes beyond the width on either operand."""
    from scaling_rgcn_training_amd import _lib
    want = ((rows + 3) // 4 + 2 * DW_BATCH - 1) // (2 * DW_BATCH)
    assert 4 <= want <= 1024 and want == {259: 5, 4099: 65, 65_536: 1024}[rows]
    gen = torch.Generator().manual_seed(rows + din * 139 + dout)
    x = _padded(rows, din, 8, dev, gen)
    g = _padded(rows, dout, 4, dev, gen)
    x[:, (din + 3) // 4 * 4:] = 7.0                                # beyond the 16-byte pieces of the width nothing is read
    g[:, (dout + 3) // 4 * 4:] = 7.0
    d_root = torch.full((din, dout), NAN, device=dev)
    d_bias = torch.full((dout,), NAN, device=dev)
    _lib.bwd_dw_root(x, din, g, dout, d_root, d_bias)
    assert torch.equal(_lib.rows_dw(x, din, g, dout), d_root), f"rows_dw vs bwd_dw_root {rows}x{din}x{dout}"
