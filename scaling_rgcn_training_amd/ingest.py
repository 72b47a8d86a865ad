"""N-Triples ingest on the GPU: the bytes of an ``.nt`` file -> the int64 COO, labelled nodes and multi-hot rows that
``TensorDataset`` takes, and the three term tables (kernels: csrc/rgcn_ingest.hip behind ``rgcn_nt_*``)::

    g = ingest.load_nt(path)                 # path | bytes | uint8 tensor
    g.edge_index, g.edge_type                # int64 [2, E], [E] on the GPU, E = 2 * message-passing triples
    g.num_nodes, g.num_relations             # N, 2 R
    g.labelled_idx, g.labels                 # int64 [L] ascending node ids, int64 [L, C] 0/1 rows
    g.nodes, g.relations, g.classes          # TermTable: id -> name, name -> id
    data = g.dataset()                       # a TensorDataset, ready for add_summary / Trainer

The contract is ``graphs.py``'s (which restates the reference's): lines end at ``\\n`` (one ``\\r`` before it is dropped, the last line
need not end in ``\\n``); a line of at most 2 bytes is skipped; every other line loses its last two bytes -- unconditionally, nothing
checks that they are ``" ."`` -- and splits at its first two spaces into subject, predicate and object (the object keeps further
spaces); ``A``-``Z`` are folded to lower case.  Terms are ordered bytewise, which is Python's ``sorted`` on the lower-cased strings for
valid UTF-8.  Node ids are the ranks among the terms that occur as subject or object (literals, blank nodes and both ends of type
triples included), relation ids the ranks among the predicates other than ``graphs.TYPE_PREDICATES``; one term may hold both.  The
i-th non-type triple in file order is edge ``2i = (s, o, 2 rel)`` and edge ``2i + 1 = (o, s, 2 rel + 1)``; duplicate triples stay
duplicate edges.  Classes are the sorted distinct objects of ``graphs.RDF_TYPE`` triples (``<type>`` triples are left out of the edges
and carry no label), except those of triples whose subject's bytes up to its first ``#`` equal ``graphs.ONTOLOGY_PREFIX``: the
reference's filter, kept literally -- it compares the whole term, so it NEVER fires for a subject written in angle brackets
(``<http://swrc...#x>`` starts with ``<``); it fires only for a bare ``http://swrc.ontoware.org/ontology#x``.  The train / val / test
split belongs to ``TensorDataset``.

Where ``graphs.Graph`` differs (documented, not chased): it lower-cases with Python's Unicode ``str.lower()``, so files with
characters that ``lower()`` changes and ASCII folding does not (``É``, ``Σ`` ...) get other names there; and it splits lines with
``str.splitlines()`` after a universal-newlines read, which also breaks at ``\\v``, ``\\f``, ``\\x1c``-``\\x1e``, ``\\x85``, U+2028, U+2029
and a lone ``\\r``.

There is no CPU path: a CPU ``device`` raises.  A malformed line (fewer than two spaces after the cut) or a NUL byte anywhere in
the file raises ``ValueError`` with the 1-based number of the first such line; both are found on the device."""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .tensor_data import TensorDataset

MAX_BYTES = 0xFFFF0000          # the kernels address the text with 32-bit offsets
ERR_COLLISION = -12             # RGCN_ERR_COLLISION
MAX_TRIES = 3                   # hash attempts after the first: 64 bits, another seed each


def _hash_bits(num_occurrences: int) -> int:
    """Hash bits of the first attempt: whole 8-bit sort passes, a collision chance of about 2^-7 (n^2 / 2^(bits + 1) with
    bits >= 2 log2(n) + 6); fewer bits are fewer sort passes.  A collision costs a retry, never a wrong id."""
    need = 2 * max(int(num_occurrences), 2).bit_length() + 6
    return min(64, -(-need // 8) * 8)


def _fold(b: bytes) -> bytes:
    return b.lower()            # (bytes.lower folds A-Z only)


class TermTable:
    """The names of one id space, sorted bytewise by construction: term ``i`` is the ASCII-folded bytes
    ``text_host[offset[i] : offset[i] + length[i]]``.  No dict of all names is ever built."""

    def __init__(self, text_host: np.ndarray, offset: np.ndarray, length: np.ndarray) -> None:
        self.text = text_host
        self.offset = np.asarray(offset, dtype=np.int64)
        self.length = np.asarray(length, dtype=np.int64)
        if self.offset.shape != self.length.shape or self.offset.ndim != 1:
            raise ValueError("offset and length must be vectors of one size")

    def __len__(self) -> int:
        return int(self.offset.shape[0])

    def _bytes(self, i: int) -> bytes:
        o = int(self.offset[i])
        return _fold(self.text[o:o + int(self.length[i])].tobytes())

    def names(self, ids: Optional[Sequence[int]] = None) -> List[str]:
        """The names of ``ids`` (default: all, in id order), decoded as UTF-8 with ``errors="surrogateescape"``."""
        if ids is None:
            ids = range(len(self))
        elif torch.is_tensor(ids):
            ids = ids.tolist()
        n = len(self)
        out = []
        for i in ids:
            i = int(i)
            if not 0 <= i < n:
                raise IndexError(f"term id {i} outside [0, {n})")
            out.append(self._bytes(i).decode("utf-8", errors="surrogateescape"))
        return out

    def index(self, name: str) -> int:
        """The id of ``name`` (compared as it is: names are lower case), or -1: a binary search over the sorted table."""
        key = name.encode("utf-8", errors="surrogateescape") if isinstance(name, str) else bytes(name)
        lo, hi = 0, len(self)
        while lo < hi:
            mid = (lo + hi) // 2
            if self._bytes(mid) < key:
                lo = mid + 1
            else:
                hi = mid
        return lo if lo < len(self) and self._bytes(lo) == key else -1

    def lookup(self, names: Sequence[str]) -> Tensor:
        """int64 ids of ``names`` (-1 where absent): the hook for aligning another file's vocabulary."""
        return torch.tensor([self.index(n) for n in names], dtype=torch.int64)


class NTGraph:
    """What ``load_nt`` returns: the tensors ``TensorDataset`` takes, on the GPU, and the term tables on the host."""

    def __init__(self, edge_index: Tensor, edge_type: Tensor, num_nodes: int, num_relations: int, labelled_idx: Tensor, labels: Tensor,
                 nodes: TermTable, relations: TermTable, classes: TermTable, name: str = "nt_graph") -> None:
        self.edge_index, self.edge_type = edge_index, edge_type
        self.num_nodes, self.num_relations = num_nodes, num_relations
        self.labelled_idx, self.labels = labelled_idx, labels
        self.nodes, self.relations, self.classes = nodes, relations, classes
        self.name = name

    @property
    def num_classes(self) -> int:
        return int(self.labels.shape[1])

    def dataset(self, split=None, seed: int = 1, name: Optional[str] = None) -> TensorDataset:
        """The ``TensorDataset`` of this graph (which needs at least one class and one edge type)."""
        return TensorDataset(self.edge_index, self.edge_type, self.num_nodes, self.num_relations, self.labelled_idx, self.labels,
                             split=split, seed=seed, name=name or self.name)


def _host_bytes(source) -> tuple:
    """(uint8 numpy array of the file, device tensor or None, name)"""
    if isinstance(source, (str, os.PathLike)):
        return np.fromfile(os.fspath(source), dtype=np.uint8), None, os.path.basename(os.fspath(source))
    if isinstance(source, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytearray(source), dtype=np.uint8), None, "nt_graph"       # (a writable copy: torch wants one)
    if torch.is_tensor(source):
        if source.dtype != torch.uint8 or source.dim() != 1:
            raise ValueError("a tensor source must be a uint8 vector: the bytes of the file")
        t = source.contiguous()
        return t.cpu().numpy(), (t if t.device.type == "cuda" else None), "nt_graph"
    raise ValueError(f"source must be a path, bytes or a uint8 tensor (got {type(source).__name__})")


def _ws(nbytes: int, what: str, dev) -> Tensor:
    if nbytes == 0:
        raise _lib.RgcnLibraryError(f"{what}: bad arguments")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def tokenize(text: Tensor):
    """``rgcn_nt_lines`` + ``rgcn_nt_tokenize`` on the uint8 device vector ``text`` -> ``(occ_off, occ_len, T, max_term_len)``:
    uint32 (as int32 storage) ``[3 T]`` term offsets / lengths, occurrence ``3 t + role``.  Raises ``ValueError`` naming the first
    malformed line or line with a NUL byte."""
    lib, dev, n = _lib.load(), text.device, int(text.shape[0])
    if n > MAX_BYTES:
        raise ValueError(f"{n} bytes: one call ingests at most {MAX_BYTES} (32-bit offsets on the device)")
    with torch.cuda.device(dev):
        stream = _lib._stream(text)
        lines = C.c_int64(0)
        nb = lib.rgcn_nt_lines_workspace_bytes(n)
        ws = _ws(nb, "rgcn_nt_lines_workspace_bytes", dev)
        _lib.check(lib.rgcn_nt_lines(text.data_ptr() if n else None, n, ws.data_ptr(), nb, C.byref(lines), stream), "rgcn_nt_lines")
        nl = int(lines.value)
        occ_off = torch.empty(3 * nl, dtype=torch.int32, device=dev)
        occ_len = torch.empty(3 * nl, dtype=torch.int32, device=dev)
        if nl == 0:
            return occ_off, occ_len, 0, 0
        nb = lib.rgcn_nt_tokenize_workspace_bytes(n, nl)
        ws = _ws(nb, "rgcn_nt_tokenize_workspace_bytes", dev)
        info = (C.c_int64 * 4)()
        st = lib.rgcn_nt_tokenize(text.data_ptr(), n, nl, occ_off.data_ptr(), occ_len.data_ptr(), ws.data_ptr(), nb, info, stream)
        if st == _lib.ERR_GRAPH:
            bad, nul = int(info[1]), int(info[2])
            if nul and (not bad or nul <= bad):
                raise ValueError(f"line {nul}: a NUL byte")
            raise ValueError(f"line {bad}: fewer than two spaces before the final two bytes: not '<s> <p> <o> .'")
        _lib.check(st, "rgcn_nt_tokenize")
    t = int(info[0])
    return occ_off[:3 * t], occ_len[:3 * t], t, int(info[3])


def build(text: Tensor, occ_off: Tensor, occ_len: Tensor, num_triples: int, max_term_len: int, hash_bits: int, seed: int):
    """One ``rgcn_nt_build`` attempt -> ``(status, counts, workspace)``; status 0 or ``ERR_COLLISION`` (anything else raises).
    ``counts``: U, N, R, C, E, L, the device status word, rounds."""
    lib, dev = _lib.load(), text.device
    with torch.cuda.device(dev):
        nb = lib.rgcn_nt_workspace_bytes(num_triples)
        ws = _ws(nb, "rgcn_nt_workspace_bytes", dev)
        counts = (C.c_int64 * 8)()
        st = lib.rgcn_nt_build(text.data_ptr() if text.shape[0] else None, int(text.shape[0]), occ_off.data_ptr() if num_triples else None,
                               occ_len.data_ptr() if num_triples else None, num_triples, max_term_len, int(hash_bits), int(seed),
                               ws.data_ptr(), nb, counts, _lib._stream(text))
    if st != ERR_COLLISION:
        _lib.check(st, "rgcn_nt_build")
    return st, counts, ws


def emit(text: Tensor, num_triples: int, counts, ws: Tensor):
    """``rgcn_nt_emit`` after a ``build`` that answered 0 -> ``(edge_index, edge_type, labelled_idx, labels, tables)``; ``tables``:
    six int64 numpy vectors on the host, (offset, length) of the nodes, relations and classes in id order."""
    lib, dev = _lib.load(), text.device
    _, n, r, c, e, l = (int(v) for v in counts[:6])
    with torch.cuda.device(dev):
        i64 = dict(dtype=torch.int64, device=dev)
        edge_index, edge_type = torch.empty(2, e, **i64), torch.empty(e, **i64)
        labelled_idx, labels = torch.empty(l, **i64), torch.empty(l, c, **i64)
        tabs = [torch.empty(k, dtype=torch.int32, device=dev) for k in (n, n, r, r, c, c)]
        ptr = lambda x: x.data_ptr() if x.numel() else None
        _lib.check(lib.rgcn_nt_emit(num_triples, counts, ptr(edge_index), ptr(edge_type), ptr(labelled_idx), ptr(labels),
                                    *[ptr(x) for x in tabs], ws.data_ptr(), int(ws.shape[0]), _lib._stream(text)), "rgcn_nt_emit")
        # (uint32 on the device; int64 byte offsets from here on)
        tables = [x.cpu().numpy().view(np.uint32).astype(np.int64) for x in tabs]
    return edge_index, edge_type, labelled_idx, labels, tables


def load_nt(source, device="cuda") -> NTGraph:
    """Ingest an N-Triples file -- a path, its ``bytes``, or a uint8 tensor of them -- on ``device`` (a GPU; there is no CPU path).
    One host -> device copy of the bytes, no per-line Python; the term tables keep the host bytes and slice names on demand."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"load_nt runs on the GPU (device={device!r}): no CPU fallback; graphs.Graph is the host loader")
    host, text, name = _host_bytes(source)
    if host.shape[0] > MAX_BYTES:
        raise ValueError(f"{host.shape[0]} bytes: one call ingests at most {MAX_BYTES} (32-bit offsets on the device)")
    if text is None or (dev.index is not None and text.device != dev):
        text = torch.from_numpy(host).to(dev) if host.shape[0] else torch.empty(0, dtype=torch.uint8, device=dev)
    occ_off, occ_len, t, max_len = tokenize(text)
    st, counts, ws = build(text, occ_off, occ_len, t, max_len, _hash_bits(3 * t), 0)
    tries = 0
    while st == ERR_COLLISION:
        tries += 1
        if tries > MAX_TRIES:
            raise RuntimeError(f"rgcn_nt_build: distinct terms shared a 64-bit hash under {MAX_TRIES} seeds")
        del ws
        st, counts, ws = build(text, occ_off, occ_len, t, max_len, 64, tries)
    edge_index, edge_type, labelled_idx, labels, tabs = emit(text, t, counts, ws)
    tables = [TermTable(host, tabs[2 * i], tabs[2 * i + 1]) for i in range(3)]
    return NTGraph(edge_index, edge_type, int(counts[1]), 2 * int(counts[2]), labelled_idx, labels, *tables, name=name)
