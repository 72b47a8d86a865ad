"""``Trainer.train_minibatch(..., block_kernels=True)``: the setup of tests/test_gpu_sampling.py::test_train_minibatch on the
kernels of csrc/rgcn_minibatch.hip -- finite losses, every parameter moves, the same batches, eager mode, and NO entry added to
the graph-plan cache by the mini-batch steps; a run with ``block_kernels=False`` beside it behaves as the existing test expects."""
import copy

import numpy as np
import pytest
import torch

from tests import sampling_reference as R

pytestmark = pytest.mark.gpu

MR, EMB, HID = 4, 16, 12


def _setup():
    from scaling_rgcn_training_amd.data import Data
    from scaling_rgcn_training_amd.layers import Emb_Layers
    n, c = 400, 4
    ei, et = R.hub_graph(n, 3000, MR, seed=31, hub_edges=200)
    g = torch.Generator().manual_seed(2)
    y = torch.nn.functional.one_hot(torch.randint(0, c, (n,), generator=g), c).float()
    perm = torch.randperm(n, generator=g)
    data = Data(edge_index=ei)
    data.edge_type = et
    data.x_train, data.y_train = perm[:100], y[perm[:100]]
    data.x_val, data.y_val = perm[100:160], y[perm[100:160]]

    class _Graph:
        pass

    gobj = _Graph()
    gobj.training_data = data
    torch.manual_seed(0)
    return gobj, data, Emb_Layers(MR, HID, c, n, EMB, None)


KEYS = ("embedding.weight", "rgcn1.weight", "rgcn1.root", "rgcn1.bias", "rgcn2.weight", "rgcn2.root", "rgcn2.bias")


def _train(block_kernels):
    from scaling_rgcn_training_amd import plan
    from scaling_rgcn_training_amd.trainer import Trainer, bce_loss
    gobj, data, model = _setup()
    before = copy.deepcopy(model.state_dict())
    tr = Trainer(None, HID, epochs=3, emb_dim=EMB, lr=0.01, weight_d=5e-5, verbose=False)
    cache = plan._CACHE
    cache.clear()
    # sum_graph=True: no full-graph validation forward, so whatever enters the plan cache comes from the mini-batch steps
    kw = dict(block_kernels=True) if block_kernels else {}
    acc, losses, f1w, f1m = tr.train_minibatch(model, gobj, bce_loss, torch.sigmoid, batch_size=32, fanouts=(4, 3), sum_graph=True,
                                               seed=3, **kw)
    torch.cuda.synchronize()
    assert tr.last_train_mode == "eager"
    assert len(losses) == 3 and acc == [] and all(np.isfinite(losses))
    assert [int(b.numel()) for b in tr.last_batches] == [32, 32, 32, 4]
    assert sorted(torch.cat(tr.last_batches).cpu().tolist()) == sorted(data.x_train.tolist())
    after = {k: v.cpu() for k, v in model.state_dict().items()}
    for k in KEYS:
        assert not torch.equal(after[k], before[k]), k
    return losses, after, len(cache)


def test_train_minibatch_on_block_kernels():
    losses_b, after_b, cached_b = _train(True)
    assert cached_b == 0, "a mini-batch step on the block kernels built a graph plan"
    losses_p, after_p, cached_p = _train(False)
    assert cached_p > 0          # (the bipartite path does build plans: the cache probe sees them)
