"""Full-batch training loop (and ``Trainer.train_minibatch``, its neighbour-sampled form) with the reference's ``Trainer`` API
(/root/reference/model/modelTrainer.py:15-116) and the loss / activation / metric helpers of
/root/reference/model/evaluation.py, re-provided so the HIP layer can be dropped into the same
experiment flow.  SURVEY.md 8f-2: the step either side of the hot path.

Differences from the reference, all on the host side of the path:
* ``evaluate`` keeps predictions on the device and makes ONE host copy of the few labelled rows, then
  computes accuracy / F1 with numpy (the reference builds a CPU ``torch.zeros`` and hands device tensors
  to sklearn, which breaks on a GPU: evaluation.py:20,29);
* validation forwards run under ``torch.no_grad()`` by default (the reference's eval forward builds an
  autograd graph it never uses: modelTrainer.py:53-55); pass ``eval_no_grad=False`` for the exact behaviour;
* the per-epoch ``.item()`` host sync of the loss is kept (modelTrainer.py:68) because the returned loss
  list is part of the API.
The loop contract itself is the reference's: per epoch on the original graph 1 eval forward + 1 train
forward + 1 backward through the two RGCN layers, Adam(lr, weight_decay), one optimizer step per epoch.
"""
from __future__ import annotations

from collections import defaultdict
from typing import Callable, Dict, List, Tuple, Union

import numpy as np
import torch
from torch import Tensor, nn

from .layers import Emb_Layers


# ---- model/evaluation.py equivalents -------------------------------------------------------------
def do_nothing(x: Tensor) -> Tensor:
    return x


def ce_loss(pred: Tensor, targets: Tensor) -> Tensor:
    return nn.functional.cross_entropy(pred, targets.argmax(-1))


def bce_loss(pred: Tensor, targets: Tensor) -> Tensor:
    return nn.functional.binary_cross_entropy(pred, targets)


def get_losst(dataset: str, sumModel: bool = False) -> Tuple[Callable, Callable]:
    """BCE + sigmoid for summary models and AIFB (multi-label), CE(argmax) + identity otherwise
    (reference evaluation.py:44-48)."""
    if sumModel or dataset == "AIFB":
        return bce_loss, torch.sigmoid
    return ce_loss, do_nothing


def _f1(y_true: np.ndarray, y_pred: np.ndarray, average: str) -> float:
    """F1 over the label columns of multilabel-indicator arrays with zero_division=0, 'weighted' by
    support or 'macro' (what sklearn.f1_score computes for the reference's call)."""
    tp = np.logical_and(y_true == 1, y_pred == 1).sum(0).astype(np.float64)
    fp = np.logical_and(y_true == 0, y_pred == 1).sum(0).astype(np.float64)
    fn = np.logical_and(y_true == 1, y_pred == 0).sum(0).astype(np.float64)
    denom = 2 * tp + fp + fn
    f1 = np.where(denom > 0, 2 * tp / np.maximum(denom, 1), 0.0)
    if average == "macro":
        return float(f1.mean()) if f1.size else 0.0
    support = (y_true == 1).sum(0).astype(np.float64)
    return float((f1 * support).sum() / support.sum()) if support.sum() > 0 else 0.0


def _metrics(pred: Tensor, activation: Callable, x: Tensor, y: Tensor, report: bool = False) -> Tuple[float, float, float]:
    """accuracy / weighted F1 / macro F1 of the predictions ``pred`` (all nodes, on the device) on rows ``x`` against ``y``:
    hard labels on the device, ONE host copy of the labelled rows, numpy metrics."""
    rows = pred.detach()[x.to(pred.device)]
    if activation is not torch.sigmoid:
        hard = torch.zeros_like(rows).scatter_(1, rows.argmax(1, keepdim=True), 1.0)
    else:
        hard = torch.round(rows)
    y_pred = hard.to("cpu").numpy().astype(np.int64)
    y_true = np.asarray(y.detach().to("cpu").numpy()).astype(np.int64)
    acc = float((y_pred == y_true).all(axis=1).mean()) if len(y_true) else 0.0
    f1_w, f1_m = _f1(y_true, y_pred, "weighted"), _f1(y_true, y_pred, "macro")
    if report:
        print(f"test rows {len(y_true)}: accuracy {acc:.4f}  f1 weighted {f1_w:.4f}  f1 macro {f1_m:.4f}")
    return acc, f1_w, f1_m


def evaluate(model: nn.Module, activation: Callable, training_data, x: Tensor, y: Tensor,
             report: bool = False, no_grad: bool = True) -> Tuple[float, float, float]:
    """accuracy (exact-match over label rows), weighted F1, macro F1 on rows ``x`` against ``y``."""
    ctx = torch.no_grad() if no_grad else torch.enable_grad()
    with ctx:
        pred = model(training_data, activation)
    return _metrics(pred, activation, x, y, report)


# ---- model/modelTrainer.py equivalent ---------------------------------------------------------------
class _CaptureFailed(RuntimeError):
    pass


def _check_number(name: str, value, types, low: int, words: str) -> None:
    if isinstance(value, bool) or not isinstance(value, types) or not value >= low:
        raise ValueError(f"{name} must be {words} >= {low} (got {value!r})")


def _step_seed(seed: int, epoch: int, b: int) -> int:
    """the sampler / negatives seed of batch ``b`` of ``epoch``: runs repeat, steps differ"""
    return (seed * 0x9E3779B97F4A7C15 + epoch * 0xD1B54A32D192ED03 + b * 0x2545F4914F6CDD1D) % (2 ** 63)


def _cut_batches(n: int, batch_size: int, perm_gen: torch.Generator, device) -> List[Tensor]:
    """one permutation of ``range(n)`` from ``perm_gen``, on ``device``, cut into consecutive batches (the last may be short)"""
    perm = torch.randperm(n, generator=perm_gen).to(device)
    return [perm[start:start + batch_size] for start in range(0, n, batch_size)]


def _data_to(data, device, **overrides):
    """a new bag of ``data``'s type with every tensor attribute on ``device``; ``overrides`` replace attributes by name"""
    out = type(data)()
    for k, v in data.__dict__.items():
        v = overrides.get(k, v)
        setattr(out, k, v.to(device) if torch.is_tensor(v) else v)
    return out


class Trainer:
    """``Trainer(data, hidden_l, epochs, emb_dim, lr, weight_d)`` with ``train_summaries``,
    ``train_original``, ``train`` and ``transfer_weights`` as in the reference.  ``data`` is any object
    with the reference ``Dataset`` attributes used here: ``sumGraphs``, ``orgGraph`` (each with
    ``relations``, ``num_nodes``, ``training_data``, ``embedding``) and ``num_classes``."""

    device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")

    # graphs up to this many edges train from replayed hipGraphs when ``hipgraph="auto"``: there the epoch is bound by
    # the host submitting its ~60 launches, not by the GPU (AIFB-shaped layer: 0.47 ms eager, 0.20 ms replayed)
    HIPGRAPH_AUTO_MAX_EDGES = 2_000_000

    def __init__(self, data, hidden_l: int, epochs: int, emb_dim: int, lr: float, weight_d: float,
                 eval_no_grad: bool = True, verbose: bool = True, hipgraph="auto", sparse_embedding: bool = False):
        self.data = data
        self.hidden_l, self.epochs, self.emb_dim, self.lr, self.weight_d = hidden_l, epochs, emb_dim, lr, weight_d
        self.sumModel: nn.Module = None
        self.eval_no_grad = eval_no_grad
        self.verbose = verbose
        # True / False / "auto": capture the epoch (eval forward; zero_grad + forward + loss + backward + Adam step) into
        # two hipGraphs and replay them -- the layer path never synchronises or allocates through the library, so it is
        # capturable as it is.  ``last_train_mode`` records what the last ``train`` call did ("hipgraph" / "eager").
        self.hipgraph = hipgraph
        self.last_train_mode = None
        self.last_batches = []      # train_minibatch: the batches (node ids) of the last epoch
        # train_minibatch: True makes a step touch only the embedding rows it gathered (sparse_optim.RowAdam on the table, DESIGN.md
        # 16); rows a step did not gather then do not move.  An option of the trainer: train_minibatch keeps its signature.
        if not isinstance(sparse_embedding, bool):
            raise ValueError(f"sparse_embedding must be a bool (got {sparse_embedding!r})")
        self.sparse_embedding = sparse_embedding

    def transfer_weights(self, orgModel: nn.Module, grad: bool) -> None:
        s = self.sumModel
        orgModel.override_params(s.rgcn1.weight.clone(), s.rgcn1.bias.clone(), s.rgcn1.root.clone(),
                                 s.rgcn2.weight.clone(), s.rgcn2.bias.clone(), s.rgcn2.root.clone(), grad)
        if self.verbose:
            print("weight transfer done")

    def _device_data(self, graph):
        """``graph.training_data`` on the training device.  Only the EDGE tensors are cached on the graph (keyed on the
        identity and version of the host tensors): the layer's graph plans are cached on the identity of the device edge
        tensors, so a fresh copy per call (what ``Data.to`` returns) would rebuild them for every ``train`` and for the final
        test evaluation.  Everything else -- labels, split indices, whatever a caller assigned since the last call
        (graphs/dataset.py:30-35,53-54) -- is moved afresh on every call, as the reference's ``.to(device)`` does
        (model/modelTrainer.py:43)."""
        data = graph.training_data
        key = (self.device, id(data.edge_index), data.edge_index._version, id(data.edge_type), data.edge_type._version)
        cached = getattr(graph, "_device_edges", None)
        if cached is None or cached[0] != key:
            cached = (key, data.edge_index.to(self.device), data.edge_type.to(self.device), data.edge_index, data.edge_type)
            try:
                graph._device_edges = cached
            except AttributeError:
                pass
        return _data_to(data, self.device, edge_index=cached[1], edge_type=cached[2])

    def _want_hipgraph(self, training_data, model: nn.Module = None) -> bool:
        if self.device.type != "cuda" or not self.eval_no_grad:
            return False
        # edge-partitioned layers issue asynchronous RCCL collectives and wait on their handles: not captured
        if model is not None and any(getattr(m, "dist", None) is not None for m in model.modules()):
            return False
        if self.hipgraph == "auto":
            return int(training_data.edge_type.shape[0]) <= self.HIPGRAPH_AUTO_MAX_EDGES
        return bool(self.hipgraph)

    def train(self, model: nn.Module, graph, loss_f: Callable, activation: Callable,
              sum_graph: bool = True) -> Tuple[List[float], List[float], List[float], List[float]]:
        model = model.to(self.device)
        training_data = self._device_data(graph)
        targets = training_data.y_train.to(torch.float32)
        if self._want_hipgraph(training_data, model):
            try:
                out = self._train_hipgraph(model, training_data, targets, loss_f, activation, sum_graph)
                self.last_train_mode = "hipgraph"
                return out
            except _CaptureFailed as err:       # nothing was trained yet: the state was restored before the capture
                if self.hipgraph is True:
                    raise
                if self.verbose:
                    print(f"hipGraph capture not possible ({err}); training eagerly")
        self.last_train_mode = "eager"
        optimizer = torch.optim.Adam(model.parameters(), lr=self.lr, weight_decay=self.weight_d)

        def train_epoch(epoch):
            model.train()
            optimizer.zero_grad()
            output = loss_f(model(training_data, activation)[training_data.x_train], targets)
            output.backward()
            optimizer.step()
            return output

        return self._run_epochs(sum_graph, lambda: self._validate(model, activation, training_data), train_epoch)

    def _validate(self, model: nn.Module, activation: Callable, training_data) -> Tuple[float, float, float]:
        """the eager validation: eval mode, one full-graph forward, the metrics of the validation rows"""
        model.eval()
        return evaluate(model, activation, training_data, training_data.x_val, training_data.y_val, no_grad=self.eval_no_grad)

    def _run_epochs(self, sum_graph: bool, validate: Callable, train_epoch: Callable, after_epoch: Callable = None):
        """THE epoch loop of every training path, with both prints.  Per epoch: unless ``sum_graph``, ``validate() -> (accuracy,
        weighted F1, macro F1)``; ``train_epoch(epoch) -> loss``, all of the epoch's training, its 0-d loss read back ONCE here;
        ``after_epoch() -> str`` where a path has work after its epoch: what it returns ends the loss line."""
        accuracies, losses, f1_ws, f1_ms = [], [], [], []
        for epoch in range(self.epochs):
            if not sum_graph:
                acc, f1_w, f1_m = validate()
                if self.verbose:
                    print(f"Accuracy on validation set = {acc}")
                accuracies.append(acc)
                f1_ws.append(f1_w)
                f1_ms.append(f1_m)
            loss_value = train_epoch(epoch).item()
            losses.append(loss_value)
            suffix = after_epoch() if after_epoch is not None else ""
            if self.verbose and epoch % 10 == 0:
                print(f"Epoch: {epoch}, Loss: {loss_value:.4f}{suffix}")
        return accuracies, losses, f1_ws, f1_ms

    def _sampler(self, graph, training_data, model: nn.Module):
        """the graph's ``NeighborSampler`` on the device edges, cached on the graph beside ``_device_edges`` (same key: the
        in-edge index is built once per graph and device)"""
        from .sampling import NeighborSampler
        key = getattr(graph, "_device_edges", (None,))[0]
        cached = getattr(graph, "_sampler", None)
        if cached is None or key is None or cached[0] != key:
            num_nodes = getattr(graph, "num_nodes", None)
            if num_nodes is None:      # the rows of the model's embedding ([S, N, emb] in the attention model)
                emb = model.embedding
                num_nodes = emb.num_embeddings if isinstance(emb, nn.Embedding) else emb.shape[-2]
            cached = (key, NeighborSampler(training_data.edge_index, training_data.edge_type, int(num_nodes),
                                           int(model.rgcn1.num_relations)))
            try:
                graph._sampler = cached
            except AttributeError:
                pass
        return cached[1]

    def train_minibatch(self, model: nn.Module, graph, loss_f: Callable, activation: Callable, batch_size: int,
                        fanouts, sum_graph: bool = True, seed: int = 0,
                        block_kernels: bool = False) -> Tuple[List[float], List[float], List[float], List[float]]:
        """``train`` with neighbour sampling: per epoch the full-batch validation forward exactly as ``train`` does it (when
        ``not sum_graph``), then a seeded permutation of ``x_train`` cut into batches of ``batch_size`` (the last may be short)
        and ONE optimizer step per batch on the blocks ``NeighborSampler.sample(batch, fanouts, step seed)`` returns, through
        ``model.forward_blocks``.  An entry of ``fanouts`` is an int or a list / tuple of ``model.rgcn1.num_relations`` ints, one fan-out
        per relation.  The step seed is a fixed odd-multiplier combination of ``seed``, the epoch and the batch index
        (mod 2^63; the sampler mixes it): runs repeat, steps differ.  The epoch's
        loss is the mean over its batches.  Eager only -- block shapes change every step, nothing is captured.  Returns the four
        lists of ``train``; ``self.last_batches`` holds the last epoch's batches (tensors of node ids).  ``block_kernels`` goes to
        ``model.forward_blocks``: True runs both layers straight from their blocks (no graph plans).
        With ``self.sparse_embedding`` (``Trainer(..., sparse_embedding=True)``; off by default) and a trainable embedding: a step touches only the embedding
        rows it gathered.  ``torch.optim.Adam`` runs over every parameter but the table, ``sparse_optim.RowAdam`` (same ``lr`` and
        ``weight_d``) over the table's rows ``blocks[0].src_nodes``, on the gradient of ``model.embedding_rows``; no table-sized
        gradient exists.  THE SEMANTICS DIFFER from the dense optimizer: a row that a step did not gather does not move in that
        step -- no momentum carry-over and no weight decay for it -- and every row's bias correction counts the row's own steps.
        ``RowAdam.check()`` (ids out of range) runs once per epoch, beside the loss read-back.  With a frozen embedding the flag
        changes nothing."""
        from .sampling import check_fanouts, check_sample_seed
        if not isinstance(block_kernels, bool):
            raise ValueError(f"block_kernels must be a bool (got {block_kernels!r})")
        if not isinstance(self.sparse_embedding, bool):        # an attribute: it may have been assigned since the constructor
            raise ValueError(f"Trainer.sparse_embedding must be a bool (got {self.sparse_embedding!r})")
        _check_number("batch_size", batch_size, int, 1, "an int")
        fanouts = check_fanouts(fanouts)
        if len(fanouts) != 2:
            raise ValueError(f"the models have two RGCN layers: fanouts takes 2 entries, got {len(fanouts)}")
        if any(isinstance(k, list) for k in fanouts):      # one fan-out per relation: the model knows how many
            if model is None:
                raise ValueError("per-relation fan-outs need the model: their length is the number of relations of its layers")
            fanouts = check_fanouts(fanouts, int(model.rgcn1.num_relations))
        seed = check_sample_seed(seed)
        model = model.to(self.device)
        training_data = self._device_data(graph)
        sampler = self._sampler(graph, training_data, model)
        targets = training_data.y_train.to(torch.float32)
        x_train = training_data.x_train.to(self.device)
        self.last_train_mode, self.last_batches = "eager", []
        row_adam = None
        table = model.embedding_table() if self.sparse_embedding else None
        if table is not None and table.requires_grad:
            from .sparse_optim import RowAdam
            row_adam = RowAdam(table, lr=self.lr, weight_decay=self.weight_d)
            optimizer = torch.optim.Adam([p for p in model.parameters() if p is not table], lr=self.lr, weight_decay=self.weight_d)
        else:
            optimizer = torch.optim.Adam(model.parameters(), lr=self.lr, weight_decay=self.weight_d)
        perm_gen = torch.Generator().manual_seed(seed)
        block_args = (block_kernels,) if block_kernels else ()       # a model with the two-argument ``forward_blocks`` keeps working

        def train_epoch(epoch):
            model.train()
            batch_losses, batches = [], []
            for b, rows in enumerate(_cut_batches(int(x_train.shape[0]), batch_size, perm_gen, self.device)):
                batch = x_train[rows]
                blocks = sampler.sample(batch, fanouts, _step_seed(seed, epoch, b))
                optimizer.zero_grad()
                if row_adam is not None:
                    emb_rows = model.embedding_rows(blocks[0].src_nodes)
                    out = model.forward_blocks_from_rows(blocks, activation, emb_rows, block_kernels)
                else:
                    out = model.forward_blocks(blocks, activation, *block_args)
                output = loss_f(out, targets[rows])
                output.backward()
                optimizer.step()
                if row_adam is not None:
                    row_adam.step(blocks[0].src_nodes, emb_rows.grad, assume_unique=True)
                batch_losses.append(output.detach())
                batches.append(batch)
            self.last_batches = batches
            if row_adam is not None:
                row_adam.check()
            return torch.stack(batch_losses).mean() if batch_losses else torch.tensor(float("nan"))

        return self._run_epochs(sum_graph, lambda: self._validate(model, activation, training_data), train_epoch)

    # ---- link prediction (linkpred.py) --------------------------------------------------------------------
    def _lp_negatives(self, s: Tensor, r: Tensor, o: Tensor, num_nodes: int, num_negatives: int, step_seed: int):
        """the negatives of one step (a hook: a CPU twin replays recorded ones)"""
        from .linkpred import corrupt
        return corrupt(s, r, o, num_nodes, num_negatives, step_seed)

    def _lp_ranks(self, z: Tensor, decoder: nn.Module, s: Tensor, r: Tensor, o: Tensor, side: str, filt):
        """(greater, equal) of one side (a hook, as above)"""
        from .linkpred import ranks
        return ranks(z, decoder, s, r, o, side, filt)

    def train_link_prediction(self, model: nn.Module, decoder: nn.Module, training_data, train_triples: Tensor,
                              valid_triples: Tensor = None, num_negatives: int = 1, batch_size: int = None, reg: float = 0.01,
                              seed: int = 0) -> Tuple[List[float], List[float]]:
        """Link prediction as PyG's ``rgcn_link_pred.py`` trains it.  ``training_data``: the encoder's graph (``edge_index`` /
        ``edge_type``, usually ``with_inverse_edges`` of the training triples); ``train_triples`` / ``valid_triples``: int64 [P, 3]
        rows (s, r, o).  Per step: a full-graph encode ``z = model(training_data, do_nothing)`` (the edge tensors are moved to the
        device once, so the plan cache serves every step), a batch of positives (all of them, in order, when ``batch_size`` is
        None; else a seeded permutation cut into batches) plus ``num_negatives`` ``corrupt`` negatives each, the loss
        ``BCEWithLogits(scores, labels) + reg (mean z^2 + mean rel^2)`` and one Adam step (``lr``, ``weight_d``) over model and
        decoder.  The step seed combines ``seed``, epoch and batch as ``train_minibatch`` does.  Eager only.  Returns
        ``(losses, mrrs)``: the mean step loss per epoch, and with ``valid_triples`` the filtered MRR (both sides, ties at their
        mean rank, filtered by train + valid triples) after every epoch, else an empty list.  ``decoder.check()`` (ids out of range)
        runs once per epoch, beside the loss read-back."""
        from .linkpred import FilterIndex, metrics
        from .sampling import check_sample_seed
        for name, t in (("train_triples", train_triples), ("valid_triples", valid_triples)):
            if t is None and name == "valid_triples":
                continue
            if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.int64:
                raise ValueError(f"{name} must be an int64 [P, 3] tensor of (s, r, o) rows")
        if train_triples.shape[0] == 0:
            raise ValueError("train_triples is empty")
        _check_number("num_negatives", num_negatives, int, 1, "an int")
        if batch_size is not None:
            _check_number("batch_size", batch_size, int, 1, "None or an int")
        _check_number("reg", reg, (int, float), 0, "a number")
        seed = check_sample_seed(seed)
        dev = self.device
        model, decoder = model.to(dev), decoder.to(dev)
        data = _data_to(training_data, dev)
        pos = train_triples.to(dev)
        valid = valid_triples.to(dev) if valid_triples is not None else None
        self.last_train_mode = "eager"
        optimizer = torch.optim.Adam(list(model.parameters()) + list(decoder.parameters()), lr=self.lr, weight_decay=self.weight_d)
        perm_gen = torch.Generator().manual_seed(seed)
        filt, mrrs = None, []

        def train_epoch(epoch):
            model.train()
            batches = [pos] if batch_size is None else [pos[rows] for rows in _cut_batches(int(pos.shape[0]), batch_size, perm_gen, dev)]
            step_losses = []
            for b, batch in enumerate(batches):
                s, r, o = (batch[:, c].contiguous() for c in range(3))
                optimizer.zero_grad()
                z = model(data, do_nothing)
                sn, rn, on = self._lp_negatives(s, r, o, int(z.shape[0]), num_negatives, _step_seed(seed, epoch, b))
                scores = decoder(z, torch.cat([s, sn]), torch.cat([r, rn]), torch.cat([o, on]))
                labels = torch.cat([torch.ones(s.shape[0], device=dev), torch.zeros(sn.shape[0], device=dev)])
                output = nn.functional.binary_cross_entropy_with_logits(scores, labels)
                output = output + reg * (z.pow(2).mean() + decoder.rel.pow(2).mean())
                output.backward()
                optimizer.step()
                step_losses.append(output.detach())
            return torch.stack(step_losses).mean()

        def after_epoch():
            nonlocal filt
            if hasattr(decoder, "check"):
                decoder.check()
            if valid is None:
                return ""
            model.eval()
            with torch.no_grad():
                z = model(data, do_nothing)
            if filt is None:
                filt = FilterIndex(torch.cat([pos, valid]), int(z.shape[0]), int(decoder.rel.shape[0]))
            vs, vr, vo = (valid[:, c].contiguous() for c in range(3))
            counts = [self._lp_ranks(z, decoder, vs, vr, vo, side, filt) for side in ("object", "subject")]
            mrrs.append(metrics(torch.cat([c[0] for c in counts]), torch.cat([c[1] for c in counts]))["mrr"])
            return f", filtered MRR: {mrrs[-1]:.4f}"

        _, losses, _, _ = self._run_epochs(True, None, train_epoch, after_epoch)       # nothing before the epoch: the ranking follows it
        return losses, mrrs

    def _train_hipgraph(self, model, training_data, targets, loss_f, activation, sum_graph):
        """The same epoch loop with its GPU work replayed from two hipGraphs: ``g_eval`` (validation forward in eval mode,
        no autograd) and ``g_train`` (zero_grad + forward + loss + backward + Adam step, ``capturable=True``: the step
        count lives on the device).  Capture needs the lazy state in place first -- graph plans, Adam moments, allocator
        pools -- so ONE eager epoch runs on a side stream before the capture and is then UNDONE (parameters restored,
        Adam state zeroed in place): the captured loop starts from exactly the state an eager ``train`` starts from.
        Per epoch the host does two replays, one host copy of the validation rows and the ``.item()`` of the loss
        (both part of the reference's API: modelTrainer.py:55,68)."""
        dev = self.device
        params = list(model.parameters())
        # the warm-up epoch also advances what is not a parameter: module buffers and the device's RNG stream (the attention
        # model's dropout) -- both are put back, so that the captured loop starts where an eager ``train`` starts.  (Inside
        # the replayed graphs the dropout masks come from torch's graph-safe Philox offsets: same distribution as the eager
        # loop's, not the same stream -- loss curves of Emb_ATT_Layers with dropout agree statistically, not bit for bit.)
        moved = params + list(model.buffers())
        saved = [t.detach().clone() for t in moved]
        rng_state = torch.cuda.get_rng_state(dev)
        optimizer = torch.optim.Adam(params, lr=self.lr, weight_decay=self.weight_d, capturable=True)
        idx_train = training_data.x_train.to(dev)

        def train_step():
            optimizer.zero_grad(set_to_none=True)
            out = model(training_data, activation)
            loss = loss_f(out[idx_train], targets)
            loss.backward()
            optimizer.step()
            return loss

        def eval_forward():
            with torch.no_grad():
                return model(training_data, activation)

        def restore():
            with torch.no_grad():
                for t, t0 in zip(moved, saved):
                    t.copy_(t0)

        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        try:
            with torch.cuda.stream(side):
                if not sum_graph:
                    model.eval()
                    eval_forward()
                model.train()
                train_step()
                # undo the warm-up epoch: parameters back, Adam moments and step count zeroed IN PLACE (their tensors are
                # what the captured optimizer step reads and writes)
                restore()
                for st in optimizer.state.values():
                    for v in st.values():
                        if torch.is_tensor(v):
                            v.zero_()
                torch.cuda.set_rng_state(rng_state, dev)
                optimizer.zero_grad(set_to_none=True)
                g_eval = g_train = pred = loss = None
                if not sum_graph:
                    model.eval()
                    g_eval = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g_eval, stream=side):
                        pred = eval_forward()
                model.train()
                g_train = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g_train, stream=side):
                    loss = train_step()
        except RuntimeError as err:
            torch.cuda.synchronize(dev)
            restore()
            for q in params:
                q.grad = None
            raise _CaptureFailed(str(err).splitlines()[0] if str(err) else type(err).__name__) from err
        torch.cuda.current_stream(dev).wait_stream(side)

        def validate():
            g_eval.replay()
            return _metrics(pred, activation, training_data.x_val, training_data.y_val)

        def train_epoch(epoch):
            g_train.replay()
            return loss

        out = self._run_epochs(sum_graph, validate, train_epoch)
        model.train()
        # the gradients live in the graph's private pool: hand the caller ordinary tensors
        for q in params:
            if q.grad is not None:
                q.grad = q.grad.detach().clone()
        return out

    def train_summaries(self, configs: Dict[str, Union[bool, str, int, float]]) -> None:
        loss_f, activation = get_losst(configs["dataset"], sumModel=True)
        first = self.data.sumGraphs[0]
        self.sumModel = Emb_Layers(2 * len(first.relations.keys()) + 1, self.hidden_l, self.data.num_classes,
                                   first.num_nodes, self.emb_dim, len(self.data.sumGraphs))
        for sumGraph in self.data.sumGraphs:
            self.sumModel.reset_embedding(sumGraph.num_nodes, self.emb_dim)
            self.train(self.sumModel, sumGraph, loss_f, activation, sum_graph=True)
            sumGraph.embedding = self.sumModel.embedding.weight.clone()

    def train_original(self, org_layers, embedding_trick: Callable, configs: Dict[str, Union[bool, str, int, float]],
                       exp: str):
        acc, loss, f1_w, f1_m = defaultdict(list), defaultdict(list), defaultdict(list), defaultdict(list)
        org = self.data.orgGraph
        orgModel = org_layers(2 * len(org.relations.keys()) + 1, self.hidden_l, self.data.num_classes, org.num_nodes,
                              self.emb_dim, configs["num_sums"])
        if exp != "baseline" and configs["e_trans"]:
            embedding = embedding_trick(org, self.data.sumGraphs, self.emb_dim)
            orgModel.load_embedding(embedding, freeze=configs["e_freeze"])
        if exp != "baseline" and configs["w_trans"]:
            self.transfer_weights(orgModel, configs["w_grad"])
        loss_f, activation = get_losst(configs["dataset"], sumModel=False)
        acc["accuracy"], loss["loss"], f1_w["f1 weighted"], f1_m["f1 macro"] = self.train(
            orgModel, org, loss_f, activation, sum_graph=False)
        td = self._device_data(org)
        # (as in the reference the model is still in train mode here: modelTrainer.py:57,113 -- only the attention model,
        # whose dropout stays active, can tell)
        test_acc, test_f1_w, test_f1_m = evaluate(orgModel, activation, td, td.x_test, td.y_test, report=self.verbose)
        return acc, loss, f1_w, f1_m, test_acc, test_f1_w, test_f1_m, orgModel
