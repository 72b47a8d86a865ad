"""``Trainer(..., sparse_embedding=True).train_minibatch(...)`` on a 2,000-node / 20,000-edge / 5-relation graph, 64
training rows in batches of 32, fan-outs (3, 3), block kernels, 2 epochs, for the three models:
  * a by-hand twin -- the dense path's table gradient at ``src_nodes`` fed to the float64 row-wise Adam of
    tests/row_adam_reference.py, the other parameters under ``torch.optim.Adam`` -- ends with the trained table, per row within
    (steps of the row) x (2^-22 max|p| + 2^-18 lr); the same twin without block kernels (``emb``, ``att``) and with batches of 48,
    whose last one holds 16 rows (``emb``);
  * rows outside the union of every step's ``src_nodes`` keep their bits at ``weight_d = 0.01`` (under the dense optimizer they move);
  * after the first step the other parameters equal the dense run's bit for bit at ``weight_d = 0``;
  * with a frozen embedding the flag changes nothing; ``forward_blocks`` is today's output and ``forward_blocks_from_rows``
    equals it;
  * ``forward_blocks`` and ``train_minibatch`` keep their signatures (tests/test_block_host.py pins them): the rows go to the
    method ``forward_blocks_from_rows``, the flag to the trainer's constructor."""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import rgcn_oracle as O
from tests.row_adam_reference import row_adam_step, tolerance

pytestmark = pytest.mark.gpu

N, EDGES, REL, CLASSES = 2000, 20000, 5, 4
EMB, HID, SUMS = 12, 12, 3
EPOCHS, BATCH, FANOUTS, SEED, LR = 2, 32, (3, 3), 3, 0.01
KINDS = ("emb", "mlp", "att")


def _graph():
    from scaling_rgcn_training_amd.data import Data
    ei, et = O.synthetic_graph(N, EDGES, REL, seed=41)
    g = torch.Generator().manual_seed(2)
    y = torch.nn.functional.one_hot(torch.randint(0, CLASSES, (N,), generator=g), CLASSES).float()
    perm = torch.randperm(N, generator=g)
    data = Data(edge_index=ei)
    data.edge_type = et
    data.x_train, data.y_train = perm[:64], y[perm[:64]]
    data.x_val, data.y_val = perm[64:100], y[perm[64:100]]

    class _Graph:
        pass

    gobj = _Graph()
    gobj.training_data = data
    return gobj


def _model(kind, freeze=False):
    from scaling_rgcn_training_amd.layers import Emb_ATT_Layers, Emb_Layers, Emb_MLP_Layers
    torch.manual_seed(0)
    if kind == "emb":
        model = Emb_Layers(REL, HID, CLASSES, N, EMB, None)
        if freeze:
            model.load_embedding(torch.randn(N, EMB), freeze=True)
    elif kind == "mlp":
        model = Emb_MLP_Layers(REL, HID, CLASSES, N, EMB, SUMS)
        model.load_embedding(torch.randn(N, SUMS * EMB), freeze=freeze)
    else:
        model = Emb_ATT_Layers(REL, HID, CLASSES, None, EMB, SUMS)
        model.load_embedding(torch.randn(SUMS, N, EMB), freeze=freeze)
    return model


def _train(model, wd, sparse, epochs=EPOCHS, loss_f=None, batch_size=BATCH, block_kernels=True):
    from scaling_rgcn_training_amd.trainer import Trainer, bce_loss
    gobj = _graph()
    kw = dict(sparse_embedding=True) if sparse else {}
    tr = Trainer(None, HID, epochs=epochs, emb_dim=EMB, lr=LR, weight_d=wd, verbose=False, **kw)
    assert tr.sparse_embedding is sparse
    torch.manual_seed(5)                 # the attention model's dropout
    _, losses, _, _ = tr.train_minibatch(model, gobj, loss_f or bce_loss, torch.sigmoid, batch_size=batch_size, fanouts=FANOUTS,
                                         sum_graph=True, seed=SEED, block_kernels=block_kernels)
    torch.cuda.synchronize()
    assert len(losses) == epochs and all(np.isfinite(losses))
    return tr


def _steps(epochs=EPOCHS, batch_size=BATCH):
    """(epoch, rows of x_train, their node ids, blocks) of every step of ``train_minibatch(seed=SEED)``: the trainer's permutation
    and step seeds, the sampler asked again"""
    from scaling_rgcn_training_amd.sampling import NeighborSampler
    dev = torch.device("cuda:0")
    data = _graph().training_data
    sampler = NeighborSampler(data.edge_index.to(dev), data.edge_type.to(dev), N, REL)
    x_train = data.x_train.to(dev)
    perm_gen = torch.Generator().manual_seed(SEED)
    out = []
    for epoch in range(epochs):
        perm = torch.randperm(64, generator=perm_gen).to(dev)
        for b, start in enumerate(range(0, 64, batch_size)):
            rows = perm[start:start + batch_size]
            step_seed = (SEED * 0x9E3779B97F4A7C15 + epoch * 0xD1B54A32D192ED03 + b * 0x2545F4914F6CDD1D) % (2 ** 63)
            out.append((epoch, rows, x_train[rows], sampler.sample(x_train[rows], FANOUTS, step_seed)))
    return out


def _table(model):
    return model.embedding_table().detach()


def _rows(t, idx):
    return t[:, idx] if t.dim() == 3 else t[idx]


@functools.lru_cache(maxsize=None)
def _sparse_run(kind):
    """(initial table, trained table, the trainer's last batches) of the sparse run at weight_d = 0.01; computed once"""
    model = _model(kind)
    before = _table(model).clone()
    tr = _train(model, 0.01, True)
    return before, _table(model).cpu(), [b.cpu() for b in tr.last_batches]


@functools.lru_cache(maxsize=None)
def _union():
    steps = _steps()
    listed = torch.zeros(N, dtype=torch.bool)
    for _, _, _, blocks in steps:
        listed[blocks[0].src_nodes.cpu()] = True
    return listed, [batch.cpu() for epoch, _, batch, _ in steps if epoch == EPOCHS - 1]


def _by_hand_twin(kind, trained, batch_size=BATCH, block_kernels=True):
    from scaling_rgcn_training_amd.trainer import bce_loss
    dev = torch.device("cuda:0")
    model = _model(kind).to(dev)
    table = model.embedding_table()
    ref = [table.detach().cpu().double().numpy().copy(), np.zeros(tuple(table.shape)), np.zeros(tuple(table.shape)),
           np.zeros(N, dtype=np.int64)]
    hyper = {k: float(np.float32(v)) for k, v in dict(lr=LR, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01).items()}
    opt = torch.optim.Adam([p for p in model.parameters() if p is not table], lr=LR, weight_decay=0.01)
    targets = _graph().training_data.y_train.to(dev).to(torch.float32)
    steps = _steps(batch_size=batch_size)
    torch.manual_seed(5)
    model.train()
    for _, rows, _, blocks in steps:
        opt.zero_grad()
        table.grad = None
        bce_loss(model.forward_blocks(blocks, torch.sigmoid, block_kernels), targets[rows]).backward()      # the dense path
        opt.step()
        src = blocks[0].src_nodes
        assert row_adam_step(*ref, src.cpu().numpy(), _rows(table.grad, src).cpu().double().numpy(), hyper) == 0
        with torch.no_grad():
            table.copy_(torch.from_numpy(ref[0]).to(torch.float32))
    assert ref[3].max() <= len(steps) and ref[3].max() >= 1
    per_row = tolerance(ref[3].astype(np.float64), np.abs(ref[0]).max(), LR)[:, None]
    err = np.abs(trained.double().numpy() - ref[0])
    touched = ref[3] > 0
    print(f"twin {kind} batch_size={batch_size} block_kernels={block_kernels}: {int(touched.sum())} rows touched, "
          f"max error {err.max():.3e}, largest error / tolerance {np.max(err[..., touched, :] / per_row[touched]):.3f}")
    assert np.all(err <= per_row)
    return steps


@pytest.mark.parametrize("kind", KINDS)
def test_by_hand_twin(kind):
    _, trained, _ = _sparse_run(kind)
    _by_hand_twin(kind, trained)


@pytest.mark.parametrize("kind", ["emb", "att"])
def test_by_hand_twin_without_block_kernels(kind):
    """``forward_blocks_from_rows(..., block_kernels=False)``: the layers run on their graph-plan kernels, the table on RowAdam"""
    model = _model(kind)
    _train(model, 0.01, True, block_kernels=False)
    _by_hand_twin(kind, _table(model).cpu(), block_kernels=False)


def test_by_hand_twin_with_a_short_last_batch():
    """batches of 48 over the 64 training rows: every epoch ends with a batch of 16"""
    model = _model("emb")
    tr = _train(model, 0.01, True, batch_size=48)
    assert [len(b) for b in tr.last_batches] == [48, 16]
    steps = _by_hand_twin("emb", _table(model).cpu(), batch_size=48)
    assert [len(rows) for _, rows, _, _ in steps] == [48, 16, 48, 16]


@pytest.mark.parametrize("kind", KINDS)
def test_rows_no_step_gathered_keep_their_bits(kind):
    before, trained, last_batches = _sparse_run(kind)
    listed, last_epoch = _union()
    assert len(last_batches) == len(last_epoch) == 2 and all(torch.equal(a, b) for a, b in zip(last_batches, last_epoch))
    assert 64 < int(listed.sum()) < N
    assert torch.equal(_rows(trained, ~listed), _rows(before.cpu(), ~listed))
    moved = (_rows(trained, listed) != _rows(before.cpu(), listed))
    assert bool(moved.any(dim=-1).all())             # weight decay alone moves every listed row


def test_dense_run_moves_those_rows():
    """what tells the two paths apart: the dense optimizer decays every row of the table"""
    model = _model("emb")
    before = _table(model).clone()
    _train(model, 0.01, False)
    listed, _ = _union()
    assert bool((_table(model).cpu()[~listed] != before.cpu()[~listed]).any(dim=-1).all())


class _SnapAtSecondStep:
    """the loss of the trainer; on its second call -- after the first step, before anything of the second -- it copies every
    parameter that is not the embedding table"""

    def __init__(self, model):
        self.model, self.calls, self.state = model, 0, None

    def __call__(self, pred, target):
        from scaling_rgcn_training_amd.trainer import bce_loss
        self.calls += 1
        if self.calls == 2:
            self.state = {k: v.detach().clone() for k, v in self.model.named_parameters() if not k.startswith("embedding")}
        return bce_loss(pred, target)


@pytest.mark.parametrize("kind", KINDS)
def test_first_step_leaves_the_other_parameters_as_the_dense_run(kind):
    states = []
    for sparse in (True, False):
        model = _model(kind)
        snap = _SnapAtSecondStep(model)
        _train(model, 0.0, sparse, epochs=1, loss_f=snap)
        assert snap.calls == 2 and snap.state
        states.append(snap.state)
    assert states[0].keys() == states[1].keys() and "rgcn1.weight" in states[0]
    initial = dict(_model(kind).named_parameters())
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), k
        assert not torch.equal(states[0][k].cpu(), initial[k].detach()), k


@pytest.mark.parametrize("kind", KINDS)
def test_frozen_embedding_ignores_the_flag(kind):
    out = []
    for sparse in (True, False):
        model = _model(kind, freeze=True)
        _train(model, 0.01, sparse)
        out.append({k: v.cpu() for k, v in model.state_dict().items()})
    assert out[0].keys() == out[1].keys()
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k
    frozen = _table(_model(kind, freeze=True))
    assert torch.equal(_table(model).cpu(), frozen)


def test_sparse_embedding_must_be_a_bool():
    from scaling_rgcn_training_amd.trainer import Trainer
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="sparse_embedding"):
            Trainer(None, HID, epochs=1, emb_dim=EMB, lr=LR, weight_d=0.0, verbose=False, sparse_embedding=bad)
        tr = Trainer(None, HID, epochs=1, emb_dim=EMB, lr=LR, weight_d=0.0, verbose=False)
        tr.sparse_embedding = bad
        with pytest.raises(ValueError, match="sparse_embedding"):
            tr.train_minibatch(_model("emb"), None, None, torch.sigmoid, 4, (2, 2))
    assert Trainer(None, HID, epochs=1, emb_dim=EMB, lr=LR, weight_d=0.0, verbose=False).sparse_embedding is False


@pytest.mark.parametrize("kind", KINDS)
def test_forward_blocks_without_rows_is_todays_output(kind):
    dev = torch.device("cuda:0")
    blocks = _steps(1)[0][3]
    model = _model(kind).to(dev).eval()              # eval: no dropout between the calls
    table = model.embedding_table()
    today = model._tail_blocks(model._block_input(blocks[0].src_nodes), blocks, torch.sigmoid, True)
    out = model.forward_blocks(blocks, torch.sigmoid, True)
    assert torch.equal(out, today)
    out.sum().backward()
    assert table.grad is not None and tuple(table.grad.shape) == tuple(table.shape)      # the dense autograd path
    # the same rows as a leaf: the same output, and the leaf's gradient is the table gradient's rows
    twin = copy.deepcopy(model)
    twin.zero_grad()
    rows = twin.embedding_rows(blocks[0].src_nodes)
    assert rows.is_leaf and rows.requires_grad and rows.shape[-2] == blocks[0].n_src
    out2 = twin.forward_blocks_from_rows(blocks, torch.sigmoid, rows, True)
    assert torch.equal(out2, out)
    out2.sum().backward()
    assert twin.embedding_table().grad is None
    assert torch.equal(rows.grad, _rows(table.grad, blocks[0].src_nodes))
    assert torch.equal(twin.rgcn1.weight.grad, model.rgcn1.weight.grad)
