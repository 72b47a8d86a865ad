"""``RowAdam``: Adam on the rows of an embedding table that a mini-batch step gathered (csrc/rgcn_emb_rows.hip).

``torch.optim.Adam`` streams the whole table on every step -- it reads ``p, g, m, v`` and writes ``p, m, v`` -- whatever the
step touched.  ``RowAdam.step(nodes, grad_rows)`` reads and writes the listed rows only: per row it is torch's dense Adam (L2
weight decay, no amsgrad) with the row's OWN step count, so a row listed on every step evolves as under the dense optimizer.
Rows a step did not list do not move: no momentum carry-over and no weight decay for them (the lazy semantics of
``torch.optim.SparseAdam`` / DGL's ``SparseAdam``, with per-row bias correction)."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib


class RowAdam:
    """``table``: a CUDA fp32 tensor or ``nn.Parameter``, ``[N, E]`` or ``[S, N, E]`` with a contiguous last dimension; it is
    updated in place.  State: ``exp_avg`` / ``exp_avg_sq`` (zeros with the table's shape and strides), ``row_step`` (int32
    ``[N]``, shared by the S planes) and ``bad_ids`` (int32 ``[1]``: listed ids outside ``[0, N)``, which update nothing)."""

    def __init__(self, table: Tensor, lr: float, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0) -> None:
        if not torch.is_tensor(table):
            raise TypeError(f"RowAdam takes a tensor or nn.Parameter (got {type(table).__name__})")
        if table.device.type != "cuda":
            raise RuntimeError("RowAdam runs only on an MI355X (ROCm 'cuda' device); there is no CPU fallback")
        if table.dtype != torch.float32 or table.dim() not in (2, 3) or (table.shape[-1] > 1 and table.stride(-1) != 1):
            raise ValueError(f"RowAdam: the table must be fp32 [N, E] or [S, N, E] with a contiguous last dimension "
                             f"(got {table.dtype} {tuple(table.shape)}, strides {table.stride()})")
        beta1, beta2 = betas
        if not lr >= 0.0 or not 0.0 <= beta1 < 1.0 or not 0.0 <= beta2 < 1.0 or not eps > 0.0 or not weight_decay >= 0.0:
            raise ValueError(f"RowAdam: lr >= 0, betas in [0, 1), eps > 0, weight_decay >= 0 "
                             f"(got {lr}, {betas}, {eps}, {weight_decay})")
        self.table = table
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(beta1), float(beta2)), float(eps), float(weight_decay)
        data = table.detach()
        self.exp_avg = torch.empty_strided(data.shape, data.stride(), dtype=torch.float32, device=data.device).zero_()
        self.exp_avg_sq = torch.empty_strided(data.shape, data.stride(), dtype=torch.float32, device=data.device).zero_()
        self.row_step = torch.zeros(data.shape[-2], dtype=torch.int32, device=data.device)
        self.bad_ids = torch.zeros(1, dtype=torch.int32, device=data.device)
        self._workspace: Optional[Tensor] = None      # grow-only scratch of the sort (steps without assume_unique)

    def step(self, nodes: Tensor, grad_rows: Tensor, assume_unique: bool = False) -> None:
        """One asynchronous call on the current stream: the rows ``nodes`` (int64 ``[n]``) take an Adam step on ``grad_rows``
        (``[n, E]``, or ``[S, n, E]``: one gradient row per position of ``nodes``).  An id listed several times takes ONE step
        on the sum of its rows, added in position order.  ``assume_unique=True`` skips the sort that finds them: the caller
        guarantees distinct ids (``blocks[0].src_nodes`` of a sampler are).  Nothing is read back; ``check()`` does that."""
        if nodes.device.type != "cuda" or grad_rows.device.type != "cuda":
            raise RuntimeError("RowAdam runs only on an MI355X (ROCm 'cuda' device); there is no CPU fallback")
        if nodes.dtype != torch.int64:
            nodes = nodes.long()
        nodes = nodes.contiguous()
        grad_rows = grad_rows.detach()
        # the kernel takes any row and plane stride that keeps rows apart; a last dimension that is not contiguous, and rows or
        # planes that overlap (an expanded view has stride 0), are copied
        e = grad_rows.shape[-1]
        if (e > 1 and grad_rows.stride(-1) != 1) or any(grad_rows.stride(d) < e for d in range(grad_rows.dim() - 1)):
            grad_rows = grad_rows.contiguous()
        n = int(nodes.shape[0])
        if not assume_unique and n > 0:
            need = _lib.emb_adam_rows_workspace_bytes(n, int(self.row_step.shape[0]))
            if self._workspace is None or self._workspace.numel() < need:
                self._workspace = torch.empty(need, dtype=torch.uint8, device=self.table.device)
        _lib.emb_adam_rows(self.table.detach(), self.exp_avg, self.exp_avg_sq, self.row_step, nodes, grad_rows, self.lr, *self.betas,
                           self.eps, self.weight_decay, assume_unique, self.bad_ids, None if assume_unique else self._workspace)

    def check(self) -> None:
        """Synchronises: raises when a step since the last check listed an id outside ``[0, N)`` (such ids updated nothing)."""
        bad = int(self.bad_ids.item())
        if bad:
            self.bad_ids.zero_()
            raise IndexError(f"RowAdam.step: {bad} listed node id(s) outside [0, {int(self.row_step.shape[0])})")

    def state_dict(self) -> dict:
        return {"exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(), "row_step": self.row_step.clone(),
                "lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay}

    def load_state_dict(self, state: dict) -> None:
        for name in ("exp_avg", "exp_avg_sq", "row_step"):
            own, given = getattr(self, name), state[name]
            if tuple(given.shape) != tuple(own.shape):
                raise ValueError(f"RowAdam.load_state_dict: {name} is {tuple(given.shape)}, the table needs {tuple(own.shape)}")
            own.copy_(given)
        self.lr, self.eps, self.weight_decay = float(state["lr"]), float(state["eps"]), float(state["weight_decay"])
        self.betas = (float(state["betas"][0]), float(state["betas"][1]))
