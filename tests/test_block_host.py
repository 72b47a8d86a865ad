"""Host-side contract of the mini-batch block kernels' Python layer: every refusal of ``RGCNConv.forward_block`` /
``sampling.block_index`` is raised before the HIP library is loaded, ``block_kernels`` is validated, and ``forward_blocks`` /
``train_minibatch`` keep their positional order."""
import inspect

import pytest
import torch

from scaling_rgcn_training_amd import _lib
from scaling_rgcn_training_amd.conv import RGCNConv
from scaling_rgcn_training_amd.sampling import Block, BlockIndex, block_index


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the HIP library was loaded before the refusal")
    monkeypatch.setattr(_lib, "load", boom)


def _block(n_src=6, n_dst=3, e=5):
    return Block(torch.zeros(2, e, dtype=torch.int64), torch.zeros(e, dtype=torch.int64), n_src, n_dst, torch.arange(n_src))


def test_forward_block_refusals():
    b, x = _block(), torch.zeros(6, 8)
    with pytest.raises(NotImplementedError, match="featureless"):
        RGCNConv(8, 4, 2, featureless=True).forward_block(None, b)
    with pytest.raises(NotImplementedError, match="max"):
        RGCNConv(8, 4, 2, aggr="max").forward_block(x, b)
    with pytest.raises(NotImplementedError, match="wide"):
        RGCNConv(200, 4, 2, wide=True).forward_block(torch.zeros(6, 200), b)
    with pytest.raises(NotImplementedError, match="in_channels"):
        RGCNConv((8, 5), 4, 2).forward_block(x, b)
    conv = RGCNConv(8, 4, 2)
    conv.dist = object()
    with pytest.raises(NotImplementedError, match="dist"):
        conv.forward_block(x, b)
    conv.dist = None
    with pytest.raises(ValueError, match="n_dst"):
        conv.forward_block(torch.zeros(2, 8), _block(n_src=2, n_dst=3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv.forward_block(x, b)                                   # CPU tensors
    with pytest.raises(ValueError, match="float32"):
        conv.forward_block(x.double(), b)
    with pytest.raises(NotImplementedError):
        conv.forward_block(torch.zeros(6, dtype=torch.int64), b)
    with pytest.raises(NotImplementedError):
        conv.forward_block((x, x[:3]), b)
    for bad in (torch.zeros(6, 7), torch.zeros(5, 8), torch.zeros(6, 8, 1)):
        with pytest.raises(ValueError):
            conv.forward_block(bad, b)
    with pytest.raises(ValueError, match="edge_index"):
        conv.forward_block(x, Block(torch.zeros(2, 5, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), 6, 3, None))


def test_block_index_refusals():
    b = _block()
    with pytest.raises(RuntimeError, match="GPU"):
        block_index(b, 2)
    with pytest.raises(ValueError):
        block_index(b, 2, "max")
    with pytest.raises(ValueError):
        block_index(b, 0)
    with pytest.raises(ValueError):
        block_index(_block(n_src=2, n_dst=3), 2)
    with pytest.raises(ValueError):
        block_index(_block(n_src=2, n_dst=0), 2)
    with pytest.raises(ValueError):
        block_index(Block(torch.zeros(2, 5, dtype=torch.int32), torch.zeros(5, dtype=torch.int32), 6, 3, None), 2)
    assert BlockIndex.__doc__


def test_block_kernels_keyword():
    from scaling_rgcn_training_amd.layers import Emb_Layers
    from scaling_rgcn_training_amd.trainer import Trainer
    fb = inspect.signature(Emb_Layers.forward_blocks)
    assert list(fb.parameters) == ["self", "blocks", "activation", "block_kernels"] and fb.parameters["block_kernels"].default is False
    tm = inspect.signature(Trainer.train_minibatch)
    assert list(tm.parameters) == ["self", "model", "graph", "loss_f", "activation", "batch_size", "fanouts", "sum_graph", "seed",
                                   "block_kernels"]
    assert tm.parameters["block_kernels"].default is False and tm.parameters["seed"].default == 0
    model = Emb_Layers(2, 4, 3, 10, 8, None)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="block_kernels"):
            model.forward_blocks([_block(), _block()], torch.sigmoid, bad)
        with pytest.raises(ValueError, match="block_kernels"):
            Trainer(None, 4, epochs=1, emb_dim=8, lr=0.01, weight_d=0.0, verbose=False).train_minibatch(
                model, None, None, torch.sigmoid, 4, (2, 2), block_kernels=bad)
    with pytest.raises(ValueError, match="2 blocks"):
        model.forward_blocks([_block()], torch.sigmoid, True)
