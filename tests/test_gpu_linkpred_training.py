"""``Trainer.train_link_prediction`` against a CPU twin built like tests/twins.py: the same ``Emb_Layers`` encoder on
the oracle's layers, a torch DistMult decoder, the same Adam, and the negatives ``corrupt`` returned on the GPU.  A 200-node,
2,000-edge, 4-relation graph (8 relations with inverses), dim 16, 15 full-batch epochs, 2 negatives per positive; 40 held-out triples
are ranked on both sides after every epoch."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from tests import linkpred_reference as R
from tests.twins import cpu_twin

pytestmark = pytest.mark.gpu

N, E, NREL, DIM, EPOCHS, NEG, HELD = 200, 2000, 4, 16, 15, 2, 40


class TorchDistMult(nn.Module):
    """the torch formulation the kernels replace, for the twin"""

    def __init__(self, rel):
        super().__init__()
        self.rel = nn.Parameter(rel.detach().cpu().clone())

    def forward(self, z, s, r, o):
        return (z[s] * self.rel[r] * z[o]).sum(-1)


def _setup(seed=0):
    from scaling_rgcn_training_amd.data import Data
    from scaling_rgcn_training_amd.layers import Emb_Layers
    from scaling_rgcn_training_amd.linkpred import DistMult, with_inverse_edges
    g = torch.Generator().manual_seed(seed)
    tri = torch.stack([torch.randint(0, N, (E + HELD,), generator=g), torch.randint(0, NREL, (E + HELD,), generator=g),
                       torch.randint(0, N, (E + HELD,), generator=g)], 1)
    train, held = tri[:E].contiguous(), tri[E:].contiguous()
    data = Data()
    data.edge_index, data.edge_type = with_inverse_edges(torch.stack([train[:, 0], train[:, 2]]), train[:, 1].clone(), NREL)
    torch.manual_seed(seed)
    model, decoder = Emb_Layers(2 * NREL, DIM, DIM, N, DIM), DistMult(NREL, DIM)
    return data, train, held, model, decoder


def _gpu_run(data, train, held, model, decoder, epochs=EPOCHS, neg=NEG, batch_size=None):
    from scaling_rgcn_training_amd.trainer import Trainer

    class Recording(Trainer):
        def _lp_negatives(self, *args):
            out = super()._lp_negatives(*args)
            self.negatives.append(tuple(t.cpu() for t in out))
            return out

        def _lp_ranks(self, z, dec, s, r, o, side, filt):
            out = super()._lp_ranks(z, dec, s, r, o, side, filt)
            self.counts.append(tuple(t.cpu().numpy() for t in out))
            return out

    t = Recording(None, DIM, epochs, DIM, 0.01, 0.0, verbose=False, hipgraph=False)
    t.negatives, t.counts = [], []
    losses, mrrs = t.train_link_prediction(copy.deepcopy(model), copy.deepcopy(decoder), data, train, held, num_negatives=neg,
                                           batch_size=batch_size, seed=3)
    return losses, mrrs, t.negatives, t.counts


def _twin_run(data, train, held, model, decoder, negatives, epochs=EPOCHS, neg=NEG, batch_size=None):
    """(losses, mrrs, bands) of the CPU twin fed the negatives the GPU run drew"""
    from scaling_rgcn_training_amd.trainer import Trainer

    class Twin(Trainer):
        device = torch.device("cpu")

        def _lp_negatives(self, *args):
            return self.replay.pop(0)

        def _lp_ranks(self, z, dec, s, r, o, side, filt):
            """exact counts on the twin's fp32 parameters in float64, and the band a fp32 ranking pass may land in"""
            anchor, target = (s, o) if side == "object" else (o, s)
            ptr, idx = filt.lists(s, r, o, side)
            lists = [idx[int(ptr[i]):int(ptr[i + 1])].tolist() for i in range(len(s))]
            zn, rn = z.detach().numpy(), dec.rel.detach().numpy()
            sc, _ = R.rank_scores(zn, rn, anchor.numpy(), r.numpy())
            g, e = R.rank_counts(sc, target.numpy(), lists)
            self.bands.append(R.rank_band(zn, rn, anchor.numpy(), r.numpy(), target.numpy(), lists))
            return torch.as_tensor(g), torch.as_tensor(e)

    twin = Twin(None, DIM, epochs, DIM, 0.01, 0.0, verbose=False, hipgraph=False)
    twin.replay, twin.bands = list(negatives), []
    t_losses, t_mrrs = twin.train_link_prediction(cpu_twin(model), TorchDistMult(decoder.rel), data, train, held, num_negatives=neg,
                                                  batch_size=batch_size, seed=3)
    assert not twin.replay
    return t_losses, t_mrrs, twin.bands


def test_loss_curve_and_filtered_mrr_match_the_cpu_twin():
    data, train, held, model, decoder = _setup()
    losses, mrrs, negatives, counts = _gpu_run(data, train, held, model, decoder)
    assert len(losses) == EPOCHS and len(mrrs) == EPOCHS and len(negatives) == EPOCHS and len(counts) == 2 * EPOCHS
    # the negatives are the restatement's, step by step
    s, r, o = (train[:, c].numpy() for c in range(3))
    for epoch in (0, EPOCHS - 1):
        step_seed = (3 * 0x9E3779B97F4A7C15 + epoch * 0xD1B54A32D192ED03) % (2 ** 63)
        for got, ref in zip(negatives[epoch], R.corrupt(s, r, o, N, NEG, step_seed)):
            assert np.array_equal(got.numpy(), ref)

    t_losses, t_mrrs, bands = _twin_run(data, train, held, model, decoder, negatives)
    print("link prediction losses  gpu", [f"{v:.6f}" for v in losses])
    print("link prediction losses twin", [f"{v:.6f}" for v in t_losses])
    print("filtered MRR  gpu", [f"{v:.6f}" for v in mrrs])
    print("filtered MRR twin", [f"{v:.6f}" for v in t_mrrs])
    outside = sum(int(((g < lo) | (g > hi)).sum()) for (g, _), (lo, hi) in zip(counts, bands))
    open_ = sum(int((lo != hi).sum()) for lo, hi in bands)
    print(f"rank counts outside the twin's float64 band: {outside} of {2 * EPOCHS * HELD}; open bands: {open_}")
    assert losses[-1] < losses[0]
    np.testing.assert_allclose(losses, t_losses, rtol=2e-4, atol=2e-5)
    # the filtered MRR: equal on both, up to the queries whose band is open
    for epoch in range(EPOCHS):
        g = np.concatenate([counts[2 * epoch][0], counts[2 * epoch + 1][0]])
        e = np.concatenate([counts[2 * epoch][1], counts[2 * epoch + 1][1]])
        lo = np.concatenate([bands[2 * epoch][0], bands[2 * epoch + 1][0]])
        hi = np.concatenate([bands[2 * epoch][1], bands[2 * epoch + 1][1]])
        assert ((g >= lo) & (g <= hi)).all(), f"epoch {epoch}: a rank count outside the float64 band"
        assert mrrs[epoch] == pytest.approx(R.metrics(g, e)["mrr"], abs=1e-12)
        if (lo == hi).all() and not e.any():
            assert mrrs[epoch] == pytest.approx(t_mrrs[epoch], abs=1e-12)


def test_a_second_run_reproduces_the_losses_bit_for_bit():
    data, train, held, model, decoder = _setup(seed=1)
    a = _gpu_run(data, train, held, model, decoder)
    b = _gpu_run(data, train, held, model, decoder)
    assert a[0] == b[0] and a[1] == b[1]
    for x, y in zip(a[2], b[2]):
        assert all(torch.equal(p, q) for p, q in zip(x, y))


def test_mini_batches_match_the_cpu_twin_and_repeat():
    """``batch_size=300``: 7 batches per epoch from one seeded permutation, the last of 200 triples; 5 epochs, 3 negatives each, on
    the graph of the full-batch test.  The bands are the twin's: they bound the rounding of a fp32 ranking pass over the TWIN's
    parameters, so they hold only while the two runs' parameters agree to fp32 rounding (max |z - z_twin| stays near 7e-7 here).
    That is a property of the graph and the initial weights, not of the kernels: Adam's first step is lr g / (|g| + 1e-8), and
    where an element's first gradient lies within the rounding of the two gradient computations (|g| < 1e-7 against a largest
    |g_gpu - g_twin| of 9e-8) the two runs step apart.  On another initialisation (``_setup(seed=2)``) one element of
    ``rgcn2.weight`` did: 6e-5 apart after step 0, z 2e-4 apart after step 1, and 5 of 400 counts one off a closed band of the
    twin while every count lay inside the band of the GPU run's own parameters."""
    from scaling_rgcn_training_amd.trainer import _step_seed
    epochs, neg, batch, seed = 5, 3, 300, 3
    data, train, held, model, decoder = _setup()
    run = lambda: _gpu_run(data, train, held, model, decoder, epochs=epochs, neg=neg, batch_size=batch)
    losses, mrrs, negatives, counts = run()
    assert len(losses) == epochs and len(mrrs) == epochs and len(negatives) == 7 * epochs and len(counts) == 2 * epochs
    # the negatives of (epoch, batch): the restatement's at that step's seed, on the batch rows of the seeded permutation
    perm_gen = torch.Generator().manual_seed(seed)
    for epoch in range(epochs):
        perm = torch.randperm(E, generator=perm_gen)
        for b in range(7):
            rows = perm[b * batch:(b + 1) * batch]
            assert len(rows) == (200 if b == 6 else batch)
            s, r, o = (train[rows, c].numpy() for c in range(3))
            for got, ref in zip(negatives[7 * epoch + b], R.corrupt(s, r, o, N, neg, _step_seed(seed, epoch, b))):
                assert np.array_equal(got.numpy(), ref), (epoch, b)
    t_losses, t_mrrs, bands = _twin_run(data, train, held, model, decoder, negatives, epochs=epochs, neg=neg, batch_size=batch)
    print("mini-batch link prediction losses  gpu", [f"{v:.6f}" for v in losses])
    print("mini-batch link prediction losses twin", [f"{v:.6f}" for v in t_losses])
    outside = sum(int(((g < lo) | (g > hi)).sum()) for (g, _), (lo, hi) in zip(counts, bands))
    print(f"mini-batch rank counts outside the twin's float64 band: {outside} of {2 * epochs * HELD}; open bands: "
          f"{sum(int((lo != hi).sum()) for lo, hi in bands)}")
    assert losses[-1] < losses[0]
    np.testing.assert_allclose(losses, t_losses, rtol=2e-4, atol=2e-5)
    for (g, e), (lo, hi) in zip(counts, bands):
        assert ((g >= lo) & (g <= hi)).all(), "a rank count outside the float64 band"
    for epoch in range(epochs):
        g = np.concatenate([counts[2 * epoch][0], counts[2 * epoch + 1][0]])
        e = np.concatenate([counts[2 * epoch][1], counts[2 * epoch + 1][1]])
        assert mrrs[epoch] == pytest.approx(R.metrics(g, e)["mrr"], abs=1e-12)
    # a second run: the same bits
    again = run()
    assert again[0] == losses and again[1] == mrrs
    for x, y in zip(again[2], negatives):
        assert all(torch.equal(p, q) for p, q in zip(x, y))
    for x, y in zip(again[3], counts):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))
