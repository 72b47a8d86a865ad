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


def _gpu_run(data, train, held, model, decoder):
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

    t = Recording(None, DIM, EPOCHS, DIM, 0.01, 0.0, verbose=False, hipgraph=False)
    t.negatives, t.counts = [], []
    losses, mrrs = t.train_link_prediction(copy.deepcopy(model), copy.deepcopy(decoder), data, train, held, num_negatives=NEG, seed=3)
    return losses, mrrs, t.negatives, t.counts


def test_loss_curve_and_filtered_mrr_match_the_cpu_twin():
    from scaling_rgcn_training_amd.trainer import Trainer
    data, train, held, model, decoder = _setup()
    losses, mrrs, negatives, counts = _gpu_run(data, train, held, model, decoder)
    assert len(losses) == EPOCHS and len(mrrs) == EPOCHS and len(negatives) == EPOCHS and len(counts) == 2 * EPOCHS
    # the negatives are the restatement's, step by step
    s, r, o = (train[:, c].numpy() for c in range(3))
    for epoch in (0, EPOCHS - 1):
        step_seed = (3 * 0x9E3779B97F4A7C15 + epoch * 0xD1B54A32D192ED03) % (2 ** 63)
        for got, ref in zip(negatives[epoch], R.corrupt(s, r, o, N, NEG, step_seed)):
            assert np.array_equal(got.numpy(), ref)

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

    twin = Twin(None, DIM, EPOCHS, DIM, 0.01, 0.0, verbose=False, hipgraph=False)
    twin.replay, twin.bands = list(negatives), []
    t_losses, t_mrrs = twin.train_link_prediction(cpu_twin(model), TorchDistMult(decoder.rel), data, train, held, num_negatives=NEG, seed=3)
    print("link prediction losses  gpu", [f"{v:.6f}" for v in losses])
    print("link prediction losses twin", [f"{v:.6f}" for v in t_losses])
    print("filtered MRR  gpu", [f"{v:.6f}" for v in mrrs])
    print("filtered MRR twin", [f"{v:.6f}" for v in t_mrrs])
    outside = sum(int(((g < lo) | (g > hi)).sum()) for (g, _), (lo, hi) in zip(counts, twin.bands))
    open_ = sum(int((lo != hi).sum()) for lo, hi in twin.bands)
    print(f"rank counts outside the twin's float64 band: {outside} of {2 * EPOCHS * HELD}; open bands: {open_}")
    assert losses[-1] < losses[0]
    np.testing.assert_allclose(losses, t_losses, rtol=2e-4, atol=2e-5)
    # the filtered MRR: equal on both, up to the queries whose band is open
    for epoch in range(EPOCHS):
        g = np.concatenate([counts[2 * epoch][0], counts[2 * epoch + 1][0]])
        e = np.concatenate([counts[2 * epoch][1], counts[2 * epoch + 1][1]])
        lo = np.concatenate([twin.bands[2 * epoch][0], twin.bands[2 * epoch + 1][0]])
        hi = np.concatenate([twin.bands[2 * epoch][1], twin.bands[2 * epoch + 1][1]])
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
