"""``Trainer.train_link_prediction`` with the ComplEx and TransE decoders against a CPU twin, on the 200-node,
2,000-edge, 4-relation graph of tests/test_gpu_linkpred_training.py: the same encoder on the oracle's layers, the torch formulation
of the decoder, the same Adam and the negatives the GPU run drew.  ComplEx trains under ``loss="bce"``, TransE under
``loss="margin"``; 5 full-batch epochs, 2 negatives per positive, 40 held-out triples ranked on both sides after every epoch."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from tests import kge_reference as K
from tests import linkpred_reference as R
from tests import test_gpu_linkpred_training as T
from tests.test_gpu_linkpred_training import DIM, NEG
from tests.test_kge_reference import torch_score
from tests.twins import cpu_twin

pytestmark = pytest.mark.gpu

EPOCHS = 5
CASES = [("complex", "bce"), ("transe", "margin")]


class TorchDecoder(nn.Module):
    """the torch formulation the kernels replace, for the twin"""

    def __init__(self, dec, rel):
        super().__init__()
        self.dec, self.rel = dec, nn.Parameter(rel.detach().cpu().clone())

    def forward(self, z, s, r, o):
        return torch_score(self.dec, z, self.rel, s, r, o)


def _setup(dec, seed=0):
    """the graph, the split and the encoder of tests/test_gpu_linkpred_training.py with another decoder"""
    from scaling_rgcn_training_amd import linkpred as L
    data, train, held, model, _ = T._setup(seed)
    torch.manual_seed(seed)
    return data, train, held, model, {"complex": L.ComplEx, "transe": L.TransE, "distmult": L.DistMult}[dec](T.NREL, DIM)


def _run(trainer_cls, data, train, held, model, decoder, **kw):
    t = trainer_cls(None, DIM, EPOCHS, DIM, 0.01, 0.0, verbose=False, hipgraph=False)
    t.negatives, t.counts, t.bands = [], [], []
    losses, mrrs = t.train_link_prediction(model, decoder, data, train, held, num_negatives=NEG, seed=3, **kw)
    return losses, mrrs, t


def _gpu_run(setup, **kw):
    from scaling_rgcn_training_amd.trainer import Trainer

    class Recording(Trainer):
        def _lp_negatives(self, *args):
            out = super()._lp_negatives(*args)
            self.negatives.append(tuple(t.cpu() for t in out))
            return out

        def _lp_ranks(self, *args):
            out = super()._lp_ranks(*args)
            self.counts.append(tuple(t.cpu().numpy() for t in out))
            return out

    data, train, held, model, decoder = setup
    return _run(Recording, data, train, held, copy.deepcopy(model), copy.deepcopy(decoder), **kw)


@pytest.mark.parametrize("dec,loss", CASES)
def test_loss_curve_and_rank_counts_match_the_cpu_twin(dec, loss):
    from scaling_rgcn_training_amd.trainer import Trainer
    setup = _setup(dec)
    data, train, held, model, decoder = setup
    losses, mrrs, gpu = _gpu_run(setup, loss=loss)
    assert len(losses) == EPOCHS and len(mrrs) == EPOCHS and len(gpu.counts) == 2 * EPOCHS

    class Twin(Trainer):
        device = torch.device("cpu")

        def _lp_negatives(self, *args):
            return self.replay.pop(0)

        def _lp_ranks(self, z, module, s, r, o, side, filt):
            """exact counts on the twin's fp32 parameters in float64, and the band a fp32 ranking pass may land in"""
            anchor, target = (s, o) if side == "object" else (o, s)
            ptr, idx = filt.lists(s, r, o, side)
            lists = [idx[int(ptr[i]):int(ptr[i + 1])].tolist() for i in range(len(s))]
            sc, cond = K.rank_scores(dec, z.detach().numpy(), module.rel.detach().numpy(), anchor.numpy(), r.numpy(), side)
            self.bands.append(K.rank_band(sc, cond, target.numpy(), lists))
            return tuple(torch.as_tensor(c) for c in R.rank_counts(sc, target.numpy(), lists))

    Twin.replay = list(gpu.negatives)
    t_losses, t_mrrs, twin = _run(Twin, data, train, held, cpu_twin(model), TorchDecoder(dec, decoder.rel), loss=loss)
    print(f"{dec} / {loss} losses  gpu", [f"{v:.6f}" for v in losses])
    print(f"{dec} / {loss} losses twin", [f"{v:.6f}" for v in t_losses])
    print(f"{dec} / {loss} filtered MRR gpu", [f"{v:.4f}" for v in mrrs], "twin", [f"{v:.4f}" for v in t_mrrs])
    assert losses[-1] < losses[0]
    np.testing.assert_allclose(losses, t_losses, rtol=2e-4, atol=2e-5)
    for (g, e), (lo, hi) in zip(gpu.counts, twin.bands):
        assert ((g >= lo) & (g <= hi)).all(), "a rank count outside the twin's float64 band"
    # a second run: the same bits
    again = _gpu_run(setup, loss=loss)
    assert again[0] == losses and again[1] == mrrs
    assert all(np.array_equal(p, q) for x, y in zip(again[2].counts, gpu.counts) for p, q in zip(x, y))


def test_bce_is_the_default_bit_for_bit():
    setup = _setup("distmult", seed=1)
    a, b = _gpu_run(setup), _gpu_run(setup, loss="bce")
    assert a[0] == b[0] and a[1] == b[1]
    with pytest.raises(ValueError, match="loss"):
        _gpu_run(setup, loss="hinge")
