"""The per-epoch contract of ``Trainer.train``, ``train_minibatch`` and ``train_link_prediction`` on stubs, CPU only: the order of
the validation forward and the training step, which step gets which sampler seed, how the permutation is cut into batches, what
is printed, and that losses and parameters are those of the loop written out by hand here.  No kernel runs."""
import copy
import types

import numpy as np
import pytest
import torch
from torch import nn

from scaling_rgcn_training_amd import trainer as T
from scaling_rgcn_training_amd.data import Data

N, CLASSES, N_TRAIN, N_VAL, EPOCHS, LR, WD = 40, 3, 25, 15, 11, 0.05, 1e-3
NREL, SEED = 2, 12345


def step_seed(seed, epoch, b):
    return (seed * 0x9E3779B97F4A7C15 + epoch * 0xD1B54A32D192ED03 + b * 0x2545F4914F6CDD1D) % (2 ** 63)


class StubModel(nn.Module):
    """``forward`` logs (kind, training, grad enabled); ``forward_blocks`` takes TWO arguments (a third would raise)"""

    def __init__(self):
        super().__init__()
        self.embedding = nn.Embedding(N, CLASSES)
        self.rgcn1 = types.SimpleNamespace(num_relations=NREL)
        self.events = []

    def forward(self, data, activation):
        self.events.append(("full", self.training, torch.is_grad_enabled()))
        return activation(self.embedding.weight)

    def forward_blocks(self, blocks, activation):
        self.events.append(("blocks", self.training, torch.is_grad_enabled()))
        return activation(self.embedding(blocks))


class StubSampler:
    """the "blocks" of a batch are the batch itself; every call is recorded with the table as it stood"""

    def __init__(self, model):
        self.model, self.calls, self.tables = model, [], []

    def sample(self, batch, fanouts, seed):
        self.calls.append((batch.clone(), fanouts, seed))
        self.tables.append(self.model.embedding.weight.detach().clone())
        return batch


class StubDecoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.rel = nn.Parameter(torch.randn(NREL, CLASSES))
        self.checks = 0

    def forward(self, z, s, r, o):
        return (z[s] * self.rel[r] * z[o]).sum(-1)

    def check(self):
        self.checks += 1


class CpuTrainer(T.Trainer):
    device = torch.device("cpu")

    def __init__(self, **kw):
        super().__init__(None, 4, EPOCHS, CLASSES, LR, WD, **kw)
        self.sampler = None
        self.negatives, self.ranks = [], []

    def _sampler(self, graph, training_data, model):
        if self.sampler is None:
            self.sampler = StubSampler(model)
        return self.sampler

    def _lp_negatives(self, s, r, o, num_nodes, num_negatives, seed):
        self.negatives.append((s.clone(), r.clone(), o.clone(), num_nodes, num_negatives, seed))
        return s.repeat(num_negatives), r.repeat(num_negatives), ((o + 1) % num_nodes).repeat(num_negatives)

    def _lp_ranks(self, z, decoder, s, r, o, side, filt):
        self.ranks.append((side, filt, s.clone(), r.clone(), o.clone()))
        greater = torch.arange(s.shape[0], dtype=torch.int64) + len(self.ranks)
        return greater, torch.ones_like(greater)


def _graph():
    g = torch.Generator().manual_seed(7)
    nodes = torch.randperm(N, generator=g)
    data = Data(edge_index=torch.zeros(2, 0, dtype=torch.int64), edge_type=torch.zeros(0, dtype=torch.int64))
    data.x_train, data.x_val = nodes[:N_TRAIN].clone(), nodes[N_TRAIN:].clone()
    labels = torch.eye(CLASSES)[torch.randint(0, CLASSES, (N,), generator=g)]
    data.y_train, data.y_val = labels[data.x_train].clone(), labels[data.x_val].clone()
    return types.SimpleNamespace(training_data=data, num_nodes=N)


def _model():
    torch.manual_seed(3)
    return StubModel()


def _validate(model, data):
    """(accuracy, weighted F1, macro F1) of the table as it stands, written out: sigmoid, round, exact-match rows"""
    with torch.no_grad():
        hard = np.round(torch.sigmoid(model.embedding.weight)[data.x_val].numpy()).astype(np.int64)
    y = data.y_val.numpy().astype(np.int64)
    return float((hard == y).all(axis=1).mean()), T._f1(y, hard, "weighted"), T._f1(y, hard, "macro")


def _train_by_hand(model, data, sum_graph):
    opt = torch.optim.Adam(model.parameters(), lr=LR, weight_decay=WD)
    accs, losses, f1_ws, f1_ms, lines = [], [], [], [], []
    for epoch in range(EPOCHS):
        if not sum_graph:
            acc, f1_w, f1_m = _validate(model, data)
            lines.append(f"Accuracy on validation set = {acc}")
            accs.append(acc)
            f1_ws.append(f1_w)
            f1_ms.append(f1_m)
        opt.zero_grad()
        loss = T.bce_loss(torch.sigmoid(model.embedding.weight)[data.x_train], data.y_train)
        loss.backward()
        opt.step()
        losses.append(loss.item())
        if epoch % 10 == 0:
            lines.append(f"Epoch: {epoch}, Loss: {losses[-1]:.4f}")
    return accs, losses, f1_ws, f1_ms, lines


def _cuts(n, batch_size, seed=SEED):
    """per epoch the consecutive cuts of one ``randperm`` from ONE generator per call"""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(EPOCHS):
        perm = torch.randperm(n, generator=gen)
        out.append([perm[start:start + batch_size] for start in range(0, n, batch_size)])
    return out


def _minibatch_by_hand(model, data, batch_size):
    opt = torch.optim.Adam(model.parameters(), lr=LR, weight_decay=WD)
    losses, tables = [], []
    for rows_of_epoch in _cuts(N_TRAIN, batch_size):
        batch_losses = []
        for rows in rows_of_epoch:
            tables.append(model.embedding.weight.detach().clone())
            opt.zero_grad()
            loss = T.bce_loss(torch.sigmoid(model.embedding(data.x_train[rows])), data.y_train[rows])
            loss.backward()
            opt.step()
            batch_losses.append(loss.detach())
        losses.append(float(torch.stack(batch_losses).mean().item()))
    return losses, tables


@pytest.fixture
def draws(monkeypatch):
    """counts the generators made and the permutations drawn through the ``torch`` module"""
    count = types.SimpleNamespace(generators=0, randperms=0)
    generator, randperm = torch.Generator, torch.randperm

    def counting_generator(*a, **kw):
        count.generators += 1
        return generator(*a, **kw)

    def counting_randperm(*a, **kw):
        count.randperms += 1
        return randperm(*a, **kw)

    monkeypatch.setattr(torch, "Generator", counting_generator)
    monkeypatch.setattr(torch, "randperm", counting_randperm)
    return count


# ---- train -------------------------------------------------------------------------------------------------------------------
def test_train_validates_then_steps_and_prints(capsys):
    graph, model = _graph(), _model()
    accs_h, losses_h, f1_ws_h, f1_ms_h, lines = _train_by_hand(copy.deepcopy(model), graph.training_data, sum_graph=False)
    tr = CpuTrainer(verbose=True)
    capsys.readouterr()
    accs, losses, f1_ws, f1_ms = tr.train(model, graph, T.bce_loss, torch.sigmoid, sum_graph=False)
    printed = capsys.readouterr().out
    assert model.events == [("full", False, False), ("full", True, True)] * EPOCHS
    assert len(accs) == len(losses) == len(f1_ws) == len(f1_ms) == EPOCHS
    assert len(lines) == EPOCHS + 2 and printed == "".join(line + "\n" for line in lines)
    assert losses == losses_h and accs == accs_h and f1_ws == f1_ws_h and f1_ms == f1_ms_h
    assert all(type(v) is float for v in losses)
    assert tr.last_train_mode == "eager" and model.training


def test_train_on_a_summary_graph_does_not_validate(capsys):
    graph, model = _graph(), _model()
    _, losses_h, _, _, lines = _train_by_hand(copy.deepcopy(model), graph.training_data, sum_graph=True)
    tr = CpuTrainer(verbose=True)
    capsys.readouterr()
    accs, losses, f1_ws, f1_ms = tr.train(model, graph, T.bce_loss, torch.sigmoid)       # sum_graph=True is the default
    assert capsys.readouterr().out == "".join(line + "\n" for line in lines) and len(lines) == 2
    assert model.events == [("full", True, True)] * EPOCHS
    assert accs == [] and f1_ws == [] and f1_ms == [] and losses == losses_h


def test_train_silent_and_eval_with_grad(capsys):
    graph, model = _graph(), _model()
    tr = CpuTrainer(verbose=False, eval_no_grad=False)
    capsys.readouterr()
    tr.train(model, graph, T.bce_loss, torch.sigmoid, sum_graph=False)
    assert capsys.readouterr().out == ""
    assert model.events == [("full", False, True), ("full", True, True)] * EPOCHS


# ---- train_minibatch ---------------------------------------------------------------------------------------------------------
def test_minibatch_batches_seeds_and_steps(capsys, draws):
    graph, model = _graph(), _model()
    data = graph.training_data
    losses_h, tables_h = _minibatch_by_hand(copy.deepcopy(model), data, 8)
    draws.generators = draws.randperms = 0
    tr = CpuTrainer(verbose=True)
    capsys.readouterr()
    accs, losses, f1_ws, f1_ms = tr.train_minibatch(model, graph, T.bce_loss, torch.sigmoid, 8, (3, (1, 2)), sum_graph=True, seed=SEED)
    assert draws.generators == 1 and draws.randperms == EPOCHS
    assert capsys.readouterr().out == "".join(f"Epoch: {e}, Loss: {losses[e]:.4f}\n" for e in (0, 10))
    calls = tr.sampler.calls
    assert len(calls) == 4 * EPOCHS and [int(c[0].numel()) for c in calls[:4]] == [8, 8, 8, 1]
    cuts = _cuts(N_TRAIN, 8)
    for epoch in range(EPOCHS):
        for b in range(4):
            batch, fanouts, seed = calls[4 * epoch + b]
            assert torch.equal(batch, data.x_train[cuts[epoch][b]])
            assert fanouts == [3, [1, 2]] and seed == step_seed(SEED, epoch, b)
    assert len(tr.last_batches) == 4 and all(torch.equal(a, data.x_train[rows]) for a, rows in zip(tr.last_batches, cuts[-1]))
    assert model.events == [("blocks", True, True)] * (4 * EPOCHS)
    assert accs == [] and f1_ws == [] and f1_ms == [] and losses == losses_h
    # one optimizer step per batch: the table every step started from is the hand loop's
    assert len(tables_h) == len(tr.sampler.tables) and all(torch.equal(a, b) for a, b in zip(tr.sampler.tables, tables_h))
    assert tr.last_train_mode == "eager"


def test_minibatch_validates_on_the_full_graph_first(capsys):
    graph, model = _graph(), _model()
    tr = CpuTrainer(verbose=True)
    capsys.readouterr()
    accs, losses, f1_ws, f1_ms = tr.train_minibatch(model, graph, T.bce_loss, torch.sigmoid, 8, (3, 3), sum_graph=False, seed=SEED)
    assert model.events == ([("full", False, False)] + [("blocks", True, True)] * 4) * EPOCHS
    assert len(accs) == len(losses) == len(f1_ws) == len(f1_ms) == EPOCHS
    lines = capsys.readouterr().out.splitlines()
    expected = [f"Accuracy on validation set = {a}" for a in accs]
    expected[1:1] = [f"Epoch: 0, Loss: {losses[0]:.4f}"]
    expected.append(f"Epoch: 10, Loss: {losses[10]:.4f}")
    assert lines == expected
    # the first validation saw the initial table
    assert (accs[0], f1_ws[0], f1_ms[0]) == _validate(_model(), graph.training_data)


def test_minibatch_without_block_kernels_calls_forward_blocks_with_two_arguments():
    graph, model = _graph(), _model()
    tr = CpuTrainer(verbose=False)
    _, losses, _, _ = tr.train_minibatch(model, graph, T.bce_loss, torch.sigmoid, 25, (3, 3), block_kernels=False)
    assert len(losses) == EPOCHS and [int(b.numel()) for b in tr.last_batches] == [25]
    with pytest.raises(TypeError):          # the stub is what it claims to be
        model.forward_blocks(tr.last_batches[0], torch.sigmoid, False)


def test_minibatch_without_a_batch_has_a_nan_loss():
    graph, model = _graph(), _model()
    graph.training_data.x_train, graph.training_data.y_train = graph.training_data.x_train[:0], graph.training_data.y_train[:0]
    tr = CpuTrainer(verbose=False)
    _, losses, _, _ = tr.train_minibatch(model, graph, T.bce_loss, torch.sigmoid, 8, (3, 3))
    assert len(losses) == EPOCHS and all(np.isnan(v) for v in losses) and tr.last_batches == []


def test_minibatch_leaves_the_global_rng_alone():
    graph, model = _graph(), _model()
    torch.manual_seed(99)
    state = torch.get_rng_state()
    CpuTrainer(verbose=False).train_minibatch(model, graph, T.bce_loss, torch.sigmoid, 8, (3, 3), sum_graph=False, seed=SEED)
    assert torch.equal(torch.get_rng_state(), state)


# ---- train_link_prediction ---------------------------------------------------------------------------------------------------
def _triples(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, N, (n,), generator=g), torch.randint(0, NREL, (n,), generator=g),
                        torch.randint(0, N, (n,), generator=g)], dim=1)


def _lp_by_hand(model, decoder, batches_of_epoch, num_negatives, reg):
    opt = torch.optim.Adam(list(model.parameters()) + list(decoder.parameters()), lr=LR, weight_decay=WD)
    losses = []
    for batches in batches_of_epoch:
        step_losses = []
        for batch in batches:
            s, r, o = batch[:, 0], batch[:, 1], batch[:, 2]
            opt.zero_grad()
            z = model.embedding.weight
            sn, rn, on = s.repeat(num_negatives), r.repeat(num_negatives), ((o + 1) % N).repeat(num_negatives)
            scores = decoder(z, torch.cat([s, sn]), torch.cat([r, rn]), torch.cat([o, on]))
            labels = torch.cat([torch.ones(s.shape[0]), torch.zeros(sn.shape[0])])
            loss = nn.functional.binary_cross_entropy_with_logits(scores, labels) + reg * (z.pow(2).mean() + decoder.rel.pow(2).mean())
            loss.backward()
            opt.step()
            step_losses.append(loss.detach())
        losses.append(float(torch.stack(step_losses).mean().item()))
    return losses


def test_link_prediction_without_batch_size(capsys, draws):
    graph, model, decoder, pos = _graph(), _model(), StubDecoder(), _triples(30, 1)
    losses_h = _lp_by_hand(copy.deepcopy(model), copy.deepcopy(decoder), [[pos]] * EPOCHS, 2, 0.01)
    draws.randperms = 0
    tr = CpuTrainer(verbose=True)
    capsys.readouterr()
    losses, mrrs = tr.train_link_prediction(model, decoder, graph.training_data, pos, num_negatives=2, seed=SEED)
    assert draws.randperms == 0
    assert capsys.readouterr().out == "".join(f"Epoch: {e}, Loss: {losses[e]:.4f}\n" for e in (0, 10))
    assert len(tr.negatives) == EPOCHS                              # one step per epoch
    for epoch, (s, r, o, num_nodes, num_negatives, seed) in enumerate(tr.negatives):
        assert torch.equal(s, pos[:, 0]) and torch.equal(r, pos[:, 1]) and torch.equal(o, pos[:, 2])
        assert (num_nodes, num_negatives, seed) == (N, 2, step_seed(SEED, epoch, 0))
    assert model.events == [("full", True, True)] * EPOCHS
    assert decoder.checks == EPOCHS and mrrs == [] and tr.ranks == []
    assert losses == losses_h and tr.last_train_mode == "eager"


def test_link_prediction_with_batches_and_validation(capsys, draws):
    graph, model, decoder, pos, held = _graph(), _model(), StubDecoder(), _triples(30, 1), _triples(6, 2)
    cuts = _cuts(30, 8)
    losses_h = _lp_by_hand(copy.deepcopy(model), copy.deepcopy(decoder), [[pos[rows] for rows in epoch] for epoch in cuts], 1, 0.01)
    draws.generators = draws.randperms = 0
    tr = CpuTrainer(verbose=True)
    capsys.readouterr()
    losses, mrrs = tr.train_link_prediction(model, decoder, graph.training_data, pos, held, batch_size=8, seed=SEED)
    assert draws.generators == 1 and draws.randperms == EPOCHS
    assert len(tr.negatives) == 4 * EPOCHS
    for epoch in range(EPOCHS):
        for b in range(4):
            s, r, o, num_nodes, num_negatives, seed = tr.negatives[4 * epoch + b]
            assert torch.equal(torch.stack([s, r, o], dim=1), pos[cuts[epoch][b]])
            assert (num_nodes, num_negatives, seed) == (N, 1, step_seed(SEED, epoch, b))
    # after every epoch: one eval forward without autograd, then the object side and the subject side through ONE filter
    assert model.events == ([("full", True, True)] * 4 + [("full", False, False)]) * EPOCHS
    assert [c[0] for c in tr.ranks] == ["object", "subject"] * EPOCHS
    assert all(c[1] is tr.ranks[0][1] for c in tr.ranks) and tr.ranks[0][1].num_nodes == N and tr.ranks[0][1].num_relations == NREL
    assert all(torch.equal(torch.stack(c[2:], dim=1), held) for c in tr.ranks)
    assert decoder.checks == EPOCHS and losses == losses_h
    # the stub's counts: greater = i + call number, equal = 1; ties at their mean rank
    expected = []
    for epoch in range(EPOCHS):
        greater = torch.cat([torch.arange(6) + 2 * epoch + 1, torch.arange(6) + 2 * epoch + 2]).double()
        expected.append(float((1.0 / (1.0 + greater + 0.5)).mean()))
    assert len(mrrs) == EPOCHS and mrrs == pytest.approx(expected, abs=1e-15)
    assert capsys.readouterr().out == "".join(f"Epoch: {e}, Loss: {losses[e]:.4f}, filtered MRR: {mrrs[e]:.4f}\n" for e in (0, 10))
