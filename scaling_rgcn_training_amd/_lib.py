"""ctypes binding of librgcn_mi355x.so (C ABI: include/rgcn_mi355x.h).

There is deliberately no fallback: if the library is missing or a call fails, an exception is
raised.  The library is built in-tree by ``__graft_entry__.build()`` / ``tools/build_lib.sh``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# RGCN_LIB: an alternative build of the same library (kernel experiments: tools/debug/)
LIB_PATH = os.environ.get("RGCN_LIB") or os.path.join(_HERE, "librgcn_mi355x.so")
ABI_VERSION = 19

XWIDE_MAX_WIDTH = 512  # RGCN_XWIDE_MAX_WIDTH

# enum rgcn_act / RGCN_FLAG_* of include/rgcn_mi355x.h
ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2
ERR_PLAN = -4          # inconsistent plan, or a plan layout the called kernel does not walk
ERR_ADDRESS = -10      # rgcn_bwd_dw_tiles: operands not addressable through a buffer descriptor
ERR_GRAPH, ERR_ARG = -9, -11      # rgcn_sample_*: an id out of range / a scalar outside its domain, a destination listed twice
FLAG_POINTER_GATHER, FLAG_DW_RING, FLAG_DW_DIRECT, FLAG_EXACT_FP32, FLAG_DW_ROOT_ONLY, FLAG_SPLIT_PRODUCERS = 1, 2, 4, 8, 16, 32


class RgcnPlanStruct(C.Structure):
    """struct rgcn_plan of include/rgcn_mi355x.h"""
    _fields_ = [
        ("n_nodes", C.c_int32), ("n_owned", C.c_int32), ("num_relations", C.c_int32),
        ("tile", C.c_int32), ("n_tiles", C.c_int32), ("n_chunks", C.c_int32), ("chunk", C.c_int32), ("n_units", C.c_int32),
        ("layout", C.c_int32), ("chunk_rows", C.c_int32),
        ("tile_ptr", C.c_void_p), ("chunk_rel", C.c_void_p), ("chunk_cnt", C.c_void_p),
        ("chunk_tile", C.c_void_p), ("chunk_flags", C.c_void_p), ("rel_order", C.c_void_p), ("slot_src", C.c_void_p),
        ("slot_w", C.c_void_p), ("slot_row", C.c_void_p), ("slot_acc", C.c_void_p), ("slot_src2", C.c_void_p),
    ]


class RgcnEdgeUnits(C.Structure):
    """struct rgcn_edge_units of include/rgcn_mi355x.h"""
    _fields_ = [("n_nodes", C.c_int32), ("n_units", C.c_int32), ("num_relations", C.c_int32), ("reserved", C.c_int32),
                ("unit_rel", C.c_void_p), ("unit_cnt", C.c_void_p), ("slot_src", C.c_void_p), ("slot_w", C.c_void_p)]


class RgcnGraphStruct(C.Structure):
    """struct rgcn_graph: the int64 COO exactly as the caller holds it (strided views allowed)"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("type", C.c_void_p),
                ("src_stride", C.c_int64), ("dst_stride", C.c_int64), ("type_stride", C.c_int64),
                ("num_edges", C.c_int64), ("num_nodes", C.c_int32), ("num_relations", C.c_int32)]


class RgcnSampleIndex(C.Structure):
    """struct rgcn_sample_index: the in-edge index of a graph (rgcn_sample_index_build)"""
    _fields_ = [("ptr", C.c_void_p), ("src", C.c_void_p), ("type", C.c_void_p),
                ("num_edges", C.c_int64), ("num_nodes", C.c_int32), ("num_relations", C.c_int32)]


class RgcnSampleRelIndex(C.Structure):
    """struct rgcn_sample_rel_index: the (destination, relation) run index of a graph (rgcn_sample_rel_index_build)"""
    _fields_ = [("run_ptr", C.c_void_p), ("run_beg", C.c_void_p), ("run_type", C.c_void_p), ("src", C.c_void_p),
                ("num_edges", C.c_int64), ("num_runs", C.c_int64), ("num_nodes", C.c_int32), ("num_relations", C.c_int32)]


class RgcnMbIndex(C.Structure):
    """struct rgcn_mb_index: the index of one sampled block (rgcn_mb_index_build)"""
    _fields_ = [("tile_ptr", C.c_void_p), ("row_beg", C.c_void_p), ("row_cnt", C.c_void_p), ("row_dst", C.c_void_p),
                ("row_scale", C.c_void_p), ("edge_src", C.c_void_p), ("dst_ptr", C.c_void_p), ("dst_rows", C.c_void_p),
                ("src_ptr", C.c_void_p), ("src_row", C.c_void_p), ("src_scale", C.c_void_p),
                ("num_edges", C.c_int64), ("n_rows", C.c_int64), ("n_src", C.c_int32), ("n_dst", C.c_int32),
                ("num_relations", C.c_int32), ("mean", C.c_int32), ("n_tiles", C.c_int32), ("reserved", C.c_int32)]


class RgcnPlanSizes(C.Structure):
    """struct rgcn_plan_sizes"""
    _fields_ = [("n_tiles", C.c_int32), ("n_chunks", C.c_int32), ("n_units", C.c_int32), ("reserved", C.c_int32),
                ("n_slots", C.c_int64), ("n_edges", C.c_int64), ("opaque", C.c_uint64 * 16)]


def _prototypes() -> dict:
    """name -> (restype, [argtypes]) of every entry point of include/rgcn_mi355x.h, as load() installs them"""
    vp, i32, u32, i64, sz, lng, f32 = C.c_void_p, C.c_int, C.c_uint, C.c_int64, C.c_size_t, C.c_long, C.c_float
    plan, units, graph, sizes, pint = (C.POINTER(RgcnPlanStruct), C.POINTER(RgcnEdgeUnits), C.POINTER(RgcnGraphStruct),
                                       C.POINTER(RgcnPlanSizes), C.POINTER(C.c_int))
    return {
        "rgcn_abi_version": (i32, []),
        "rgcn_status_string": (C.c_char_p, [i32]),
        "rgcn_padded_width": (i32, [i32]),
        "rgcn_packed_weight_floats": (sz, [i32, i32, i32]),
        "rgcn_pack_weights": (i32, [vp, vp, i32, i32, i32, i32, vp, vp]),
        "rgcn_fwd": (i32, [plan, vp, i32, i32, vp, vp, vp, i32, i32, i32, u32, vp]),
        "rgcn_bwd_dx": (i32, [plan, vp, i32, i32, vp, vp, i32, i32, vp, i32, u32, vp]),
        "rgcn_act_backward": (i32, [vp, vp, vp, lng, i32, i32, vp]),
        "rgcn_bwd_dw_workspace_bytes": (sz, [plan, i32, i32]),
        "rgcn_bwd_dw": (i32, [plan, vp, i32, i32, vp, i32, i32, vp, sz, vp, vp, vp, u32, vp]),
        "rgcn_plan_workspace_bytes": (sz, [i64, i32, i32, i32]),
        "rgcn_edge_weights": (i32, [graph, i32, vp, vp, sz, vp]),
        "rgcn_plan_build_begin": (i32, [graph, vp, i32, i32, i32, i32, i32, i32, vp, sz, sizes, vp]),
        "rgcn_plan_build_finish": (i32, [sizes, vp, sz, plan, vp]),
        "rgcn_dw_tiles_geometry": (i32, [pint, pint, pint]),
        "rgcn_dw_tiles_walk": (i32, [plan, vp, vp]),
        "rgcn_bwd_dw_tiles_workspace_bytes": (sz, [i32]),
        "rgcn_bwd_dw_tiles": (i32, [plan, vp, vp, i32, i32, vp, i32, i32, vp, sz, vp, u32, vp]),
        "rgcn_bwd_dw_root_workspace_bytes": (sz, []),
        "rgcn_bwd_dw_root": (i32, [vp, i32, i32, vp, i32, i32, lng, vp, sz, vp, vp, vp]),
        "rgcn_pack_weights_basis": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]),
        "rgcn_pack_weights_block": (i32, [vp, vp, i32, i32, i32, i32, i32, vp, vp]),
        "rgcn_basis_backward": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]),
        "rgcn_block_backward": (i32, [vp, i32, i32, i32, i32, vp, vp]),
        "rgcn_eplan_segments": (i32, [vp, i64, i32, vp, sz, vp, vp, vp]),
        "rgcn_ep_transform": (i32, [units, vp, i32, i32, vp, vp, i32, i32, u32, vp]),
        "rgcn_ep_segment_sum": (i32, [vp, i32, vp, vp, vp, i32, i32, vp, i32, vp, i32, i32, vp, i32, vp]),
        "rgcn_featureless_geometry": (i32, [i32, i32, i32, pint, pint]),
        "rgcn_featureless_fwd": (i32, [plan, vp, i64, vp, vp, i32, vp, vp, vp, i32, i32, vp]),
        "rgcn_featureless_bwd_workspace_bytes": (sz, [plan, i32, i32, i32]),
        "rgcn_featureless_bwd": (i32, [plan, vp, vp, vp, i64, vp, i32, i32, vp, vp, i32, vp, sz, vp, vp, vp, vp, vp]),
        "rgcn_xwide_geometry": (i32, [i32, i32, i32, pint, pint]),
        "rgcn_xwide_fwd": (i32, [plan, vp, i32, i32, vp, vp, vp, i32, i32, i32, vp]),
        "rgcn_xwide_bwd_dx": (i32, [plan, vp, i32, i32, vp, vp, i32, i32, vp, i32, vp]),
        "rgcn_xwide_bwd_dw_workspace_bytes": (sz, [plan, i32, i32]),
        "rgcn_xwide_bwd_dw": (i32, [plan, vp, i32, i32, vp, i32, i32, vp, sz, vp, vp, vp, vp]),
        "rgcn_segment_max": (i32, [vp, vp, i32, vp, vp, vp, i32, i32, vp, vp, i32, vp]),
        "rgcn_segment_max_bwd": (i32, [vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp, i64, i32, vp, i32, vp]),
        "rgcn_rows_transform": (i32, [vp, i32, i32, vp, i32, vp, i32, vp, vp, i32, i32, lng, vp]),
        "rgcn_rows_dw_workspace_bytes": (sz, [i32, i32]),
        "rgcn_rows_dw": (i32, [vp, i32, i32, vp, i32, i32, lng, vp, sz, vp, vp]),
        "rgcn_summary_workspace_bytes": (sz, [i64, i32, i32]),
        "rgcn_summary_round": (i32, [graph, i32, vp, i32, i32, vp, vp, sz, C.POINTER(C.c_int32), vp]),
        "rgcn_summary_quotient": (i32, [graph, vp, i32, i32, vp, vp, vp, vp, vp, sz, C.POINTER(C.c_int64), vp]),
        "rgcn_sample_index_workspace_bytes": (sz, [i64, i32]),
        "rgcn_sample_hop_workspace_bytes": (sz, [i64, i32, i64, i32]),
        "rgcn_sample_index_build": (i32, [graph, vp, vp, vp, vp, sz, vp]),
        "rgcn_sample_hop": (i32, [C.POINTER(RgcnSampleIndex), vp, i64, i32, i64, i32, vp, vp, vp, vp, vp, vp, sz,
                                  C.POINTER(C.c_int64), C.POINTER(C.c_int64), vp]),
        "rgcn_sample_rel_index_workspace_bytes": (sz, [i64, i32]),
        "rgcn_sample_hop_rel_workspace_bytes": (sz, [i64, vp, i32, i64, i64, i32]),
        "rgcn_sample_rel_index_build": (i32, [graph, vp, vp, vp, vp, vp, sz, C.POINTER(C.c_int64), vp]),
        "rgcn_sample_hop_rel": (i32, [C.POINTER(RgcnSampleRelIndex), vp, i64, vp, i64, i32, vp, vp, vp, vp, vp, vp, sz,
                                      C.POINTER(C.c_int64), C.POINTER(C.c_int64), vp]),
        "rgcn_mb_index_bytes": (sz, [i64, i64, i64, i32]),
        "rgcn_mb_index_workspace_bytes": (sz, [i64, i64, i64, i32]),
        "rgcn_mb_index_build": (i32, [vp, i64, vp, i64, vp, i64, i64, i64, i64, i32, i32, vp, sz, vp, sz, C.POINTER(RgcnMbIndex), vp]),
        "rgcn_mb_fwd": (i32, [C.POINTER(RgcnMbIndex), vp, i32, i32, vp, vp, vp, i32, vp, i32, vp, i32, i32, vp]),
        "rgcn_mb_bwd_dx": (i32, [C.POINTER(RgcnMbIndex), vp, i32, i32, vp, vp, i32, vp, i32, i32, vp]),
        "rgcn_mb_bwd_dw_workspace_bytes": (sz, [C.POINTER(RgcnMbIndex), i32, i32]),
        "rgcn_mb_bwd_dw": (i32, [C.POINTER(RgcnMbIndex), vp, i32, i32, vp, i32, i32, vp, vp, vp, sz, vp]),
        "rgcn_emb_adam_rows_workspace_bytes": (sz, [i64, i32]),
        "rgcn_emb_adam_rows": (i32, [vp, vp, vp, vp, i32, i64, i32, i32, i32, vp, i64, vp, i64, i32, f32, f32, f32, f32, f32, i32, vp, vp,
                                     sz, vp]),
        "rgcn_lp_score": (i32, [vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, i64, vp, vp, vp]),
        "rgcn_lp_index_workspace_bytes": (sz, [i64, i32, i32]),
        "rgcn_lp_index_build": (i32, [vp, vp, vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, sz, vp]),
        "rgcn_lp_backward_workspace_bytes": (sz, [i64, i32, i32]),
        "rgcn_lp_backward": (i32, [vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, i32, vp, i32, vp, sz, vp]),
        "rgcn_lp_corrupt": (i32, [vp, vp, vp, i64, i32, i32, i64, vp, vp, vp, vp]),
        "rgcn_lp_rank_workspace_bytes": (sz, [i64, i32, i32]),
        "rgcn_lp_rank": (i32, [vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, i64, vp, vp, i64, vp, vp, vp, sz, vp]),
        "rgcn_tr_block_labels_workspace_bytes": (sz, [i64, i64, i64, i32]),
        "rgcn_tr_block_labels": (i32, [vp, i64, i64, vp, vp, i64, i64, i32, vp, vp, i64, vp, vp, vp, sz, vp]),
        "rgcn_tr_gather": (i32, [vp, vp, vp, vp, i32, i32, i64, vp, i64, i32, i64, vp, i64, i64, vp, vp]),
        "rgcn_nt_lines_workspace_bytes": (sz, [i64]),
        "rgcn_nt_lines": (i32, [vp, i64, vp, sz, C.POINTER(C.c_int64), vp]),
        "rgcn_nt_tokenize_workspace_bytes": (sz, [i64, i64]),
        "rgcn_nt_tokenize": (i32, [vp, i64, i64, vp, vp, vp, sz, C.POINTER(C.c_int64), vp]),
        "rgcn_nt_workspace_bytes": (sz, [i64]),
        "rgcn_nt_build": (i32, [vp, i64, vp, vp, i64, i64, i32, i64, vp, sz, C.POINTER(C.c_int64), vp]),
        "rgcn_nt_emit": (i32, [i64, C.POINTER(C.c_int64), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    }


_PROTOTYPES = _prototypes()
EXPORTS = tuple(_PROTOTYPES)      # (tests/test_abi.py compares it with the header's declarations)


class RgcnLibraryError(RuntimeError):
    pass


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """dlopen the HIP library once; raise loudly when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RgcnLibraryError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the R-GCN layer.")
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.rgcn_abi_version() != ABI_VERSION:
        raise RgcnLibraryError(f"ABI version mismatch: library {lib.rgcn_abi_version()} != binding {ABI_VERSION}")
    _lib = lib
    return lib


def check(status: int, what: str) -> None:
    if status != 0:
        msg = load().rgcn_status_string(status).decode()
        err = RgcnLibraryError(f"{what} failed with status {status}: {msg}")
        err.status = status
        raise err


def buffer_addressable(rows: int, ld: int) -> bool:
    """Can a [rows, ld] fp32 matrix be gathered through a buffer descriptor (csrc/rgcn_kernels_shared.h buffer_bytes: 24-bit
    row index, 32-bit offsets with the one-past-the-end padding row in range)?  The tile-major weight-gradient kernel
    addresses both operands that way only; the other kernels fall back to 64-bit pointers."""
    return rows < (1 << 24) and (rows + 1) * ld * 4 < 0xFFFFFF00


def plan_struct(plan) -> RgcnPlanStruct:
    """Fill the C struct from a plan.TilePlan whose tensors live on the GPU."""
    cached = getattr(plan, "_cstruct", None)       # the plan's tensors never change: build the struct once
    if cached is not None:
        return cached
    if plan.slot_src.device.type != "cuda":
        raise RgcnLibraryError("the graph plan must live on the GPU (plan tensors are on %s)" % plan.slot_src.device)
    plan._cstruct = RgcnPlanStruct(
        plan.n_nodes, plan.n_owned, plan.num_relations, plan.tile, plan.n_tiles, plan.n_chunks, plan.chunk, plan.n_units,
        int(plan.layout), int(plan.chunk_rows or plan.chunk),
        plan.tile_ptr.data_ptr(), plan.chunk_rel.data_ptr(), plan.chunk_cnt.data_ptr(),
        plan.chunk_tile.data_ptr(), plan.chunk_flags.data_ptr(), plan.rel_order.data_ptr(), plan.slot_src.data_ptr(),
        plan.slot_w.data_ptr(), plan.slot_row.data_ptr(), plan.slot_acc.data_ptr(),
        _ptr(plan.slot_src2))
    return plan._cstruct


def _stream(t: torch.Tensor) -> int:
    """the current torch stream OF THE TENSOR'S DEVICE (launches go where the data lives, like every torch op)"""
    return torch.cuda.current_stream(t.device).cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def padded_width(w: int) -> int:
    return load().rgcn_padded_width(int(w))


# ---- thin typed wrappers: device tensors in, device tensors out, current torch stream of the tensors' device ----
def pack_weights(weight: torch.Tensor, root: Optional[torch.Tensor], transpose: bool) -> torch.Tensor:
    lib = load()
    r, din, dout = weight.shape
    n = lib.rgcn_packed_weight_floats(r, din, dout)
    if n == 0:
        raise RgcnLibraryError(f"unsupported layer widths {din}->{dout} (1..128 per side)")
    packed = torch.empty(n, dtype=torch.float32, device=weight.device)
    with torch.cuda.device(weight.device):
        check(lib.rgcn_pack_weights(weight.data_ptr(), _ptr(root), r, din, dout, int(transpose),
                                    packed.data_ptr(), _stream(weight)), "rgcn_pack_weights")
    return packed


def pack_weights_decomposed(weight: torch.Tensor, comp: Optional[torch.Tensor], root: Optional[torch.Tensor], num_relations: int,
                            din: int, dout: int, transpose: bool) -> torch.Tensor:
    """The pack of a layer's weights whatever their parametrisation (PyG RGCNConv): dense ``weight [R, in, out]``, basis
    decomposition (``weight [B, in, out]`` + ``comp [R, B]``) or block-diagonal (``weight [R, nb, in/nb, out/nb]``).  The
    decompositions are composed inside the packer: no [R, in, out] tensor exists."""
    if comp is None and weight.dim() == 3:
        return pack_weights(weight, root, transpose)
    lib = load()
    n = lib.rgcn_packed_weight_floats(num_relations, din, dout)
    if n == 0:
        raise RgcnLibraryError(f"unsupported layer widths {din}->{dout} (1..128 per side)")
    packed = torch.empty(n, dtype=torch.float32, device=weight.device)
    with torch.cuda.device(weight.device):
        if comp is not None:
            check(lib.rgcn_pack_weights_basis(weight.data_ptr(), comp.data_ptr(), _ptr(root), num_relations, weight.shape[0], din, dout,
                                              int(transpose), packed.data_ptr(), _stream(weight)), "rgcn_pack_weights_basis")
        else:
            check(lib.rgcn_pack_weights_block(weight.data_ptr(), _ptr(root), num_relations, weight.shape[1], din, dout,
                                              int(transpose), packed.data_ptr(), _stream(weight)), "rgcn_pack_weights_block")
    return packed


def decomposed_weight_grads(d_w: torch.Tensor, weight: torch.Tensor, comp: Optional[torch.Tensor], need_weight: bool, need_comp: bool):
    """(d_weight, d_comp) of the layer's own parameters from the dense ``d_w [R, in, out]`` scratch the weight-gradient kernels
    wrote (rgcn_basis_backward / rgcn_block_backward)."""
    lib = load()
    r, din, dout = d_w.shape
    with torch.cuda.device(d_w.device):
        if comp is not None:
            dv = torch.empty_like(weight) if need_weight else None
            dc = torch.empty_like(comp) if need_comp else None
            if need_weight or need_comp:
                check(lib.rgcn_basis_backward(d_w.data_ptr(), weight.data_ptr(), comp.data_ptr(), r, weight.shape[0], din, dout,
                                              _ptr(dv), _ptr(dc), _stream(d_w)), "rgcn_basis_backward")
            return dv, dc
        db = None
        if need_weight:
            db = torch.empty_like(weight)
            check(lib.rgcn_block_backward(d_w.data_ptr(), r, weight.shape[1], din, dout, db.data_ptr(), _stream(d_w)), "rgcn_block_backward")
        return db, None


def fwd(ps: RgcnPlanStruct, x: torch.Tensor, din: int, packed: torch.Tensor,
        bias: Optional[torch.Tensor], out: torch.Tensor, dout: int, act: int = ACT_NONE, flags: int = 0) -> None:
    with torch.cuda.device(x.device):
        check(load().rgcn_fwd(C.byref(ps), x.data_ptr(), x.stride(0), din, packed.data_ptr(), _ptr(bias),
                              out.data_ptr(), out.stride(0), dout, int(act), int(flags), _stream(x)), "rgcn_fwd")


def bwd_dx(ps_t: RgcnPlanStruct, g: torch.Tensor, dout: int, packed_t: torch.Tensor,
           dx: torch.Tensor, din: int, relu_of: Optional[torch.Tensor] = None, flags: int = 0) -> None:
    with torch.cuda.device(g.device):
        check(load().rgcn_bwd_dx(C.byref(ps_t), g.data_ptr(), g.stride(0), dout, packed_t.data_ptr(),
                                 dx.data_ptr(), dx.stride(0), din, _ptr(relu_of),
                                 0 if relu_of is None else relu_of.stride(0), int(flags), _stream(g)), "rgcn_bwd_dx")


def act_backward(a: torch.Tensor, da: torch.Tensor, act: int) -> torch.Tensor:
    """dz = da * act'(a), a = act(z) (both [rows, ld] with the same 16-byte-aligned stride)"""
    assert a.stride(0) == da.stride(0) and a.stride(1) == 1 and da.stride(1) == 1 and a.stride(0) % 4 == 0
    dz = torch.empty_strided(da.shape, da.stride(), dtype=torch.float32, device=da.device)
    with torch.cuda.device(a.device):
        check(load().rgcn_act_backward(a.data_ptr(), da.data_ptr(), dz.data_ptr(), a.shape[0], a.stride(0), int(act),
                                       _stream(a)), "rgcn_act_backward")
    return dz


def bwd_dw(ps: RgcnPlanStruct, x: torch.Tensor, din: int, g: torch.Tensor, dout: int,
           d_weight: Optional[torch.Tensor], d_root: Optional[torch.Tensor],
           d_bias: Optional[torch.Tensor], flags: int = 0) -> None:
    lib = load()
    nbytes = lib.rgcn_bwd_dw_workspace_bytes(C.byref(ps), din, dout)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        check(lib.rgcn_bwd_dw(C.byref(ps), x.data_ptr(), x.stride(0), din, g.data_ptr(), g.stride(0), dout,
                              ws.data_ptr(), nbytes, _ptr(d_weight), _ptr(d_root), _ptr(d_bias), int(flags), _stream(x)),
              "rgcn_bwd_dw")


# ---- graph plan, built on the device (rgcn_plan.hip) --------------------------------------------------------------
def graph_struct(edge_index: torch.Tensor, edge_type: torch.Tensor, n_nodes: int, num_relations: int):
    """(struct rgcn_graph, tensors it points into).  int64 device tensors are passed as they are -- strided views such
    as the rows of the reference's transposed [E, 3] edge tensor included; other integer dtypes are converted."""
    src, dst = edge_index[0], edge_index[1]
    if src.dtype != torch.int64:
        src, dst = src.long(), dst.long()
    typ = edge_type if edge_type.dtype == torch.int64 else edge_type.long()
    if src.device.type != "cuda" or typ.device != src.device:
        raise RgcnLibraryError("the graph must live on the GPU")
    e = int(typ.shape[0])
    g = RgcnGraphStruct(src.data_ptr() if e else None, dst.data_ptr() if e else None, typ.data_ptr() if e else None,
                        src.stride(0) if e else 1, dst.stride(0) if e else 1, typ.stride(0) if e else 1,
                        e, int(n_nodes), int(num_relations))
    return g, (src, dst, typ)


def plan_workspace(num_edges: int, n_owned: int, num_relations: int, tile: int, device) -> torch.Tensor:
    n = load().rgcn_plan_workspace_bytes(int(num_edges), int(n_owned), int(num_relations), int(tile))
    if n == 0:
        raise RgcnLibraryError("rgcn_plan_workspace_bytes: bad arguments")
    return torch.empty(n, dtype=torch.uint8, device=device)


def edge_weights(graph: RgcnGraphStruct, aggr: str, ws: torch.Tensor) -> torch.Tensor:
    """w_e of rgcn_edge_weights: 1 / max(1, c[dst_e, rel_e]) for "mean", 1 for "sum" / "add" and for "max" (an edge's
    multiplicity: its weight in the tie count of a max)"""
    if aggr not in ("mean", "sum", "add", "max"):
        raise ValueError(f"unsupported aggr {aggr!r}")
    w = torch.empty(max(int(graph.num_edges), 1), dtype=torch.float32, device=ws.device)
    with torch.cuda.device(ws.device):
        check(load().rgcn_edge_weights(C.byref(graph), int(aggr != "mean"), w.data_ptr(), ws.data_ptr(), ws.numel(),
                                       _stream(ws)), "rgcn_edge_weights")
    return w[:int(graph.num_edges)]


def plan_build(graph: RgcnGraphStruct, w: torch.Tensor, transposed: bool, node_begin: int, node_end: int, tile: int,
               chunk: int, ws: torch.Tensor, split=False):
    """-> (RgcnPlanStruct, dict of the ten device arrays, n_edges placed).  split: plan layout -- 0 (False) rows of a (tile, relation) group dealt
    over its row tiles; 1 (True) the team placement of experiment builds; 2 relation-major units of the
    edge-parallel path (one pseudo tile); 3 layout 0 with the rows of a (destination, relation) run compacted onto one head slot
    (compact_runs_kernel: only rgcn_tile3p_kernel walks it, every weight-gradient entry point refuses it)"""
    lib, dev = load(), ws.device
    sizes = RgcnPlanSizes()
    with torch.cuda.device(dev):
        check(lib.rgcn_plan_build_begin(C.byref(graph), w.data_ptr() if graph.num_edges else None, int(transposed),
                                        int(node_begin), int(node_end), int(tile), int(chunk), int(split), ws.data_ptr(),
                                        ws.numel(), C.byref(sizes), _stream(ws)), "rgcn_plan_build_begin")
        i32 = dict(dtype=torch.int32, device=dev)
        arr = {
            "tile_ptr": torch.empty(sizes.n_tiles + 1, **i32), "chunk_rel": torch.empty(sizes.n_chunks, **i32),
            "chunk_cnt": torch.empty(sizes.n_chunks, **i32), "chunk_tile": torch.empty(sizes.n_chunks, **i32),
            "chunk_flags": torch.empty(sizes.n_chunks, **i32), "rel_order": torch.empty(sizes.n_units, **i32),
            "slot_src": torch.empty(sizes.n_slots, **i32), "slot_w": torch.empty(sizes.n_slots, dtype=torch.float32, device=dev),
            "slot_row": torch.empty(sizes.n_slots, **i32), "slot_acc": torch.empty(sizes.n_slots, **i32),
        }
        if int(split) == 5:      # second rows of the pairs (the tile-major weight-gradient plan)
            arr["slot_src2"] = torch.empty(max(sizes.n_chunks * 8, 1), **i32)
        ps = RgcnPlanStruct()
        for k, t in arr.items():
            setattr(ps, k, t.data_ptr())
        check(lib.rgcn_plan_build_finish(C.byref(sizes), ws.data_ptr(), ws.numel(), C.byref(ps), _stream(ws)),
              "rgcn_plan_build_finish")
    return ps, arr, int(sizes.n_edges)


def dw_tiles_geometry():
    """(tile, walkers, max relations) of the tile-major weight-gradient kernel"""
    t, w, r = C.c_int(), C.c_int(), C.c_int()
    check(load().rgcn_dw_tiles_geometry(C.byref(t), C.byref(w), C.byref(r)), "rgcn_dw_tiles_geometry")
    return t.value, w.value, r.value


def dw_tiles_walk(ps: RgcnPlanStruct, device) -> torch.Tensor:
    """walk_ptr of rgcn_bwd_dw_tiles for a plan of the tile-major geometry: int32 [num_relations, walkers + 1]"""
    walkers = dw_tiles_geometry()[1]
    out = torch.empty(int(ps.num_relations), walkers + 1, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        check(load().rgcn_dw_tiles_walk(C.byref(ps), out.data_ptr(), _stream(out)), "rgcn_dw_tiles_walk")
    return out


def bwd_dw_tiles(ps: RgcnPlanStruct, walk_ptr: torch.Tensor, x: torch.Tensor, din: int, g: torch.Tensor, dout: int,
                 d_weight: torch.Tensor, flags: int = 0) -> None:
    lib = load()
    nbytes = lib.rgcn_bwd_dw_tiles_workspace_bytes(int(ps.num_relations))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        check(lib.rgcn_bwd_dw_tiles(C.byref(ps), walk_ptr.data_ptr(), x.data_ptr(), x.stride(0), din, g.data_ptr(), g.stride(0),
                                    dout, ws.data_ptr(), nbytes, d_weight.data_ptr(), int(flags), _stream(x)), "rgcn_bwd_dw_tiles")


def bwd_dw_root(x: torch.Tensor, din: int, g: torch.Tensor, dout: int, d_root: Optional[torch.Tensor],
                d_bias: Optional[torch.Tensor]) -> None:
    """d_root = x^T g, d_bias = column sums of g (rgcn_bwd_dw_root): rows of x and g pair up one to one."""
    lib = load()
    if x.shape[0] != g.shape[0]:
        raise RgcnLibraryError("rgcn_bwd_dw_root: x and g must have the same number of rows")
    with torch.cuda.device(x.device):
        ws = torch.empty(lib.rgcn_bwd_dw_root_workspace_bytes(), dtype=torch.uint8, device=x.device)
        check(lib.rgcn_bwd_dw_root(x.data_ptr(), x.stride(0), din, g.data_ptr(), g.stride(0), dout, x.shape[0],
                                   ws.data_ptr(), ws.numel(), _ptr(d_root), _ptr(d_bias), _stream(x)), "rgcn_bwd_dw_root")


# ---- graph summaries (rgcn_summary.hip; summaries.py validates and drives them) -------------------------------------------
SUMMARY_DIRECTIONS = {"out": 0, "in": 1, "in_out": 2}      # enum rgcn_summary_direction
SUMMARY_MAX_KEYS = 0xFFFF0000                              # edges (twice that for "in_out") one call sorts
SUMMARY_MAX_RELATIONS = 65536


def summary_workspace(num_edges: int, num_nodes: int, direction: int, device) -> torch.Tensor:
    n = load().rgcn_summary_workspace_bytes(int(num_edges), int(num_nodes), int(direction))
    if n == 0:
        raise RgcnLibraryError("rgcn_summary_workspace_bytes: bad arguments")
    return torch.empty(n, dtype=torch.uint8, device=device)


def summary_round(graph: RgcnGraphStruct, direction: int, block_in: torch.Tensor, num_blocks_in: int, block_out: torch.Tensor,
                  ws: torch.Tensor, route: int = 0) -> int:
    """one refinement round (rgcn_summary_round): int32 ``block_in`` -> ``block_out``, returns the number of blocks"""
    nb = C.c_int32(-1)
    with torch.cuda.device(ws.device):
        check(load().rgcn_summary_round(C.byref(graph), int(direction), block_in.data_ptr(), int(num_blocks_in), int(route),
                                        block_out.data_ptr(), ws.data_ptr(), ws.numel(), C.byref(nb), _stream(ws)),
              "rgcn_summary_round")
    return int(nb.value)


def summary_quotient(graph: RgcnGraphStruct, block: torch.Tensor, num_blocks: int, ws: torch.Tensor, route: int = 0):
    """(edge_index_s int64 [2, E_s], edge_type_s [E_s], multiplicity [E_s]) of rgcn_summary_quotient"""
    e = int(graph.num_edges)
    out = torch.empty(4, max(e, 1), dtype=torch.int64, device=ws.device)      # rows: src, dst, type, multiplicity
    ne = C.c_int64(-1)
    with torch.cuda.device(ws.device):
        check(load().rgcn_summary_quotient(C.byref(graph), block.data_ptr(), int(num_blocks), int(route), out[0].data_ptr(),
                                           out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), ws.data_ptr(), ws.numel(),
                                           C.byref(ne), _stream(ws)), "rgcn_summary_quotient")
    out = out[:, :int(ne.value)]
    return out[:2].clone(), out[2].clone(), out[3].clone()


# ---- neighbour sampling (rgcn_sample.hip; sampling.py validates and drives them) -------------------------------------------
SAMPLE_MAX_EDGES = 0xFFFF0000
SAMPLE_MAX_RELATIONS = 65536
SAMPLE_MAX_FANOUT = 256


def sample_index_build(graph: RgcnGraphStruct, device):
    """(struct rgcn_sample_index, (ptr uint32-as-int32 [N + 1], src int32 [E], type int32 [E])) of rgcn_sample_index_build"""
    lib = load()
    e, n = int(graph.num_edges), int(graph.num_nodes)
    nbytes = lib.rgcn_sample_index_workspace_bytes(e, n)
    if nbytes == 0:
        raise RgcnLibraryError("rgcn_sample_index_workspace_bytes: bad arguments")
    with torch.cuda.device(device):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        ptr = torch.empty(n + 1, dtype=torch.int32, device=device)      # (uint32 on the device: edge counts pass 2^31)
        src = torch.empty(max(e, 1), dtype=torch.int32, device=device)
        typ = torch.empty(max(e, 1), dtype=torch.int32, device=device)
        check(lib.rgcn_sample_index_build(C.byref(graph), ptr.data_ptr(), src.data_ptr(), typ.data_ptr(), ws.data_ptr(), nbytes,
                                          _stream(ws)), "rgcn_sample_index_build")
    ix = RgcnSampleIndex(ptr.data_ptr(), src.data_ptr(), typ.data_ptr(), e, n, int(graph.num_relations))
    return ix, (ptr, src, typ)


def sample_hop_cap(num_dst: int, fanout: int, num_edges: int) -> int:
    """the most edges a block of ``num_dst`` destinations can hold (`cap` of include/rgcn_mi355x.h)"""
    return num_edges if fanout < 0 else min(num_edges, num_dst * fanout)


def _sample_hop(name: str, ix, dst_nodes: torch.Tensor, cap: int, nbytes: int, node_map: torch.Tensor, call):
    """what both hops do around their C call; ``call(dst, nd, map, e_src, e_dst, e_type, nodes, ws, nbytes, ne, ns, stream)``"""
    dev, nd, n = dst_nodes.device, int(dst_nodes.shape[0]), int(ix.num_nodes)
    if nbytes == 0:
        raise RgcnLibraryError(f"{name}_workspace_bytes: bad arguments")
    ne, ns = C.c_int64(-1), C.c_int64(-1)
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        edges = torch.empty(3, max(cap, 1), dtype=torch.int64, device=dev)      # rows: src, dst, type
        nodes = torch.empty(max(nd + min(cap, n), 1), dtype=torch.int64, device=dev)
        check(call(dst_nodes.data_ptr() if nd else None, nd, node_map.data_ptr(), edges[0].data_ptr(), edges[1].data_ptr(),
                   edges[2].data_ptr(), nodes.data_ptr(), ws.data_ptr(), nbytes, C.byref(ne), C.byref(ns), _stream(ws)), name)
    eb, nsrc = int(ne.value), int(ns.value)
    if eb == cap:      # (no copy where the worst case was met)
        return edges[:2, :eb], edges[2, :eb], nodes[:nsrc].clone()
    return edges[:2, :eb].clone(), edges[2, :eb].clone(), nodes[:nsrc].clone()


def sample_hop(ix: RgcnSampleIndex, dst_nodes: torch.Tensor, fanout: int, seed: int, hop: int, node_map: torch.Tensor):
    """one hop (rgcn_sample_hop) -> (edge_index [2, E_b], edge_type [E_b], src_nodes [n_src]), int64 on the device of
    ``dst_nodes`` (contiguous int64); ``node_map``: the sampler's persistent int32 [N] map, all -1 between calls"""
    lib, nd, e, k = load(), int(dst_nodes.shape[0]), int(ix.num_edges), int(fanout)
    nbytes = lib.rgcn_sample_hop_workspace_bytes(nd, k, e, int(ix.num_nodes))
    return _sample_hop("rgcn_sample_hop", ix, dst_nodes, sample_hop_cap(nd, k, e), nbytes, node_map,
                       lambda dst, n_dst, *rest: lib.rgcn_sample_hop(C.byref(ix), dst, n_dst, k, int(seed), int(hop), *rest))


def sample_rel_index_build(graph: RgcnGraphStruct, device):
    """(struct rgcn_sample_rel_index, (run_ptr uint32-as-int32 [N + 1], run_beg [num_runs + 1], run_type int32 [num_runs],
    src int32 [E])) of rgcn_sample_rel_index_build"""
    lib = load()
    e, n = int(graph.num_edges), int(graph.num_nodes)
    nbytes = lib.rgcn_sample_rel_index_workspace_bytes(e, n)
    if nbytes == 0:
        raise RgcnLibraryError("rgcn_sample_rel_index_workspace_bytes: bad arguments")
    nr = C.c_int64(-1)
    with torch.cuda.device(device):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        run_ptr = torch.empty(n + 1, dtype=torch.int32, device=device)
        run_beg = torch.empty(e + 1, dtype=torch.int32, device=device)      # (sized for the worst case: every edge its own run)
        run_type = torch.empty(max(e, 1), dtype=torch.int32, device=device)
        src = torch.empty(max(e, 1), dtype=torch.int32, device=device)
        check(lib.rgcn_sample_rel_index_build(C.byref(graph), run_ptr.data_ptr(), run_beg.data_ptr(), run_type.data_ptr(),
                                              src.data_ptr(), ws.data_ptr(), nbytes, C.byref(nr), _stream(ws)),
              "rgcn_sample_rel_index_build")
    runs = int(nr.value)
    if runs < e:      # (keep what was written, not the worst case)
        run_beg, run_type = run_beg[:runs + 1].clone(), run_type[:max(runs, 1)].clone()
    ix = RgcnSampleRelIndex(run_ptr.data_ptr(), run_beg.data_ptr(), run_type.data_ptr(), src.data_ptr(), e, runs, n,
                            int(graph.num_relations))
    return ix, (run_ptr, run_beg, run_type, src)


def sample_hop_rel_cap(num_dst: int, fanouts, num_edges: int) -> int:
    """`cap` of a per-relation hop: E if an entry is -1, else min(E, num_dst * sum of the positive entries)"""
    if any(k < 0 for k in fanouts):
        return num_edges
    return min(num_edges, num_dst * sum(fanouts))


def sample_hop_rel(ix: RgcnSampleRelIndex, dst_nodes: torch.Tensor, fanouts, seed: int, hop: int, node_map: torch.Tensor):
    """one hop with a fan-out per relation (rgcn_sample_hop_rel); ``fanouts``: ``num_relations`` ints, validated by the caller;
    returns what ``sample_hop`` returns"""
    lib, nd, e, r = load(), int(dst_nodes.shape[0]), int(ix.num_edges), int(ix.num_relations)
    fan = (C.c_int32 * r)(*[int(k) for k in fanouts])
    nbytes = lib.rgcn_sample_hop_rel_workspace_bytes(nd, fan, r, e, int(ix.num_runs), int(ix.num_nodes))
    return _sample_hop("rgcn_sample_hop_rel", ix, dst_nodes, sample_hop_rel_cap(nd, fan, e), nbytes, node_map,
                       lambda dst, n_dst, *rest: lib.rgcn_sample_hop_rel(C.byref(ix), dst, n_dst, fan, int(seed), int(hop), *rest))


# ---- mini-batch layers straight from a sampled block (rgcn_minibatch.hip; sampling.block_index / conv._BlockFn drive them) ------
_MB_ARRAYS = (("tile_ptr", torch.int32), ("row_beg", torch.int32), ("row_cnt", torch.int32), ("row_dst", torch.int32),
              ("row_scale", torch.float32), ("edge_src", torch.int32), ("dst_ptr", torch.int32), ("dst_rows", torch.int32),
              ("src_ptr", torch.int32), ("src_row", torch.int32), ("src_scale", torch.float32))


class MbIndex:
    """The index of one block as rgcn_mb_index_build made it.  It owns its arena; ``struct`` is what the layer calls take; the
    attributes named in ``_MB_ARRAYS`` are views of the arena's valid parts (uint32 arrays read as int32: positions and slots of
    the blocks a test or a step handles stay far below 2^31)."""

    def __init__(self, struct: RgcnMbIndex, arena: torch.Tensor):
        self.struct, self.arena = struct, arena
        self.num_edges, self.n_src, self.n_dst = int(struct.num_edges), int(struct.n_src), int(struct.n_dst)
        self.num_relations, self.mean = int(struct.num_relations), bool(struct.mean)
        self.n_rows, self.n_tiles = int(struct.n_rows), int(struct.n_tiles)
        self.n_slots = 16 * self.n_tiles
        m = self.num_edges + self.n_dst
        sizes = {"tile_ptr": self.num_relations + 2, "row_beg": self.n_slots, "row_cnt": self.n_slots, "row_dst": self.n_slots,
                 "row_scale": self.n_slots, "edge_src": m, "dst_ptr": self.n_dst + 1, "dst_rows": self.n_rows,
                 "src_ptr": self.n_src + 1, "src_row": m, "src_scale": m}
        base = arena.data_ptr()
        for name, dtype in _MB_ARRAYS:
            off = (getattr(struct, name) or base) - base
            setattr(self, name, arena[off:off + 4 * sizes[name]].view(dtype))


def mb_index_build(edge_index: torch.Tensor, edge_type: torch.Tensor, n_src: int, n_dst: int, num_relations: int,
                   mean: bool = True) -> MbIndex:
    """rgcn_mb_index_build on the int64 device tensors of a block (strided rows allowed): one host synchronisation"""
    lib, dev = load(), edge_index.device
    src, dst = edge_index[0], edge_index[1]
    if src.dtype != torch.int64:
        src, dst = src.long(), dst.long()
    typ = edge_type if edge_type.dtype == torch.int64 else edge_type.long()
    e = int(typ.shape[0])
    args = (e, int(n_src), int(n_dst), int(num_relations))
    nbytes, wbytes = lib.rgcn_mb_index_bytes(*args), lib.rgcn_mb_index_workspace_bytes(*args)
    st = RgcnMbIndex()
    with torch.cuda.device(dev):
        arena = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        ws = torch.empty(max(wbytes, 1), dtype=torch.uint8, device=dev)
        check(lib.rgcn_mb_index_build(src.data_ptr() if e else None, src.stride(0) if e else 1, dst.data_ptr() if e else None,
                                      dst.stride(0) if e else 1, typ.data_ptr() if e else None, typ.stride(0) if e else 1, *args,
                                      int(bool(mean)), arena.data_ptr(), nbytes, ws.data_ptr(), wbytes, C.byref(st), _stream(arena)),
              "rgcn_mb_index_build")
    return MbIndex(st, arena)


def mb_fwd(ix: MbIndex, x: torch.Tensor, din: int, packed: torch.Tensor, bias: Optional[torch.Tensor], dout: int):
    """(out [n_dst, round4(dout)], H [slots, round4(din)]) of rgcn_mb_fwd; ``x``: padded rows [n_src, ld]"""
    dev, r4 = x.device, lambda w: (w + 3) // 4 * 4
    with torch.cuda.device(dev):
        h = torch.empty(ix.n_slots, r4(din), dtype=torch.float32, device=dev)
        z = torch.empty(ix.n_slots, r4(dout), dtype=torch.float32, device=dev)
        out = torch.empty(ix.n_dst, r4(dout), dtype=torch.float32, device=dev)
        check(load().rgcn_mb_fwd(C.byref(ix.struct), x.data_ptr(), x.stride(0), din, packed.data_ptr(), _ptr(bias), h.data_ptr(),
                                 h.stride(0), z.data_ptr(), z.stride(0), out.data_ptr(), out.stride(0), dout, _stream(x)), "rgcn_mb_fwd")
    return out, h


def mb_bwd_dx(ix: MbIndex, g: torch.Tensor, dout: int, packed_t: torch.Tensor, din: int) -> torch.Tensor:
    """dX [n_src, round4(din)] of rgcn_mb_bwd_dx; ``g``: padded rows [n_dst, ld]"""
    dev, ld = g.device, (din + 3) // 4 * 4
    with torch.cuda.device(dev):
        dh = torch.empty(ix.n_slots, ld, dtype=torch.float32, device=dev)
        dx = torch.empty(ix.n_src, ld, dtype=torch.float32, device=dev)
        check(load().rgcn_mb_bwd_dx(C.byref(ix.struct), g.data_ptr(), g.stride(0), dout, packed_t.data_ptr(), dh.data_ptr(), ld,
                                    dx.data_ptr(), ld, din, _stream(g)), "rgcn_mb_bwd_dx")
    return dx


def mb_bwd_dw(ix: MbIndex, h: torch.Tensor, din: int, g: torch.Tensor, dout: int, d_weight: Optional[torch.Tensor],
              d_root: Optional[torch.Tensor]) -> None:
    """dense d_W [R, din, dout] and d_root [din, dout] (either None) of rgcn_mb_bwd_dw from the forward's H"""
    lib, dev = load(), g.device
    nbytes = lib.rgcn_mb_bwd_dw_workspace_bytes(C.byref(ix.struct), din, dout)
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        check(lib.rgcn_mb_bwd_dw(C.byref(ix.struct), h.data_ptr(), h.stride(0), din, g.data_ptr(), g.stride(0), dout, _ptr(d_weight),
                                 _ptr(d_root), _ptr(ws), nbytes, _stream(g)), "rgcn_mb_bwd_dw")


# ---- sparse embedding rows (rgcn_emb_rows.hip) --------------------------------------------------------------------------
def emb_adam_rows_workspace_bytes(n_rows: int, num_nodes: int) -> int:
    return int(load().rgcn_emb_adam_rows_workspace_bytes(int(n_rows), int(num_nodes)))


def emb_adam_rows(table: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, row_step: torch.Tensor, nodes: torch.Tensor,
                  grad: torch.Tensor, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float,
                  assume_unique: bool = False, bad_ids: Optional[torch.Tensor] = None,
                  workspace: Optional[torch.Tensor] = None) -> None:
    """rgcn_emb_adam_rows on device tensors: ``table`` [N, E] or [S, N, E] (fp32, last dimension contiguous, updated in place),
    its moments with the table's strides, ``row_step`` int32 [N], ``nodes`` int64 [n], ``grad`` [n, E] or [S, n, E], ``bad_ids``
    int32 [1] or None.  ``workspace``: uint8, at least ``emb_adam_rows_workspace_bytes`` unless ``assume_unique`` (allocated
    here when it is missing).  Asynchronous on the current stream of the table's device."""
    lib, dev = load(), table.device
    if table.dim() not in (2, 3) or grad.dim() != table.dim():
        raise RgcnLibraryError(f"rgcn_emb_adam_rows: table is [N, E] or [S, N, E] and grad has as many dimensions "
                               f"(got {tuple(table.shape)}, {tuple(grad.shape)})")
    for name, t, dtype in (("table", table, torch.float32), ("exp_avg", exp_avg, torch.float32), ("exp_avg_sq", exp_avg_sq, torch.float32),
                           ("grad", grad, torch.float32), ("row_step", row_step, torch.int32), ("nodes", nodes, torch.int64)):
        if t.device != dev or t.dtype != dtype:
            raise RgcnLibraryError(f"rgcn_emb_adam_rows: {name} must be {dtype} on {dev} (got {t.dtype} on {t.device})")
    planes = int(table.shape[0]) if table.dim() == 3 else 1
    n_nodes, width, n = int(table.shape[-2]), int(table.shape[-1]), int(nodes.shape[0])
    for name, t in (("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        if t.shape != table.shape or t.stride() != table.stride():
            raise RgcnLibraryError(f"rgcn_emb_adam_rows: {name} must have the table's shape and strides")
    if (table.stride(-1) != 1 and width > 1) or (grad.stride(-1) != 1 and width > 1):
        raise RgcnLibraryError("rgcn_emb_adam_rows: the last dimension of table and grad must be contiguous")
    if nodes.dim() != 1 or (n > 1 and nodes.stride(0) != 1) or not row_step.is_contiguous() or int(row_step.shape[0]) != n_nodes:
        raise RgcnLibraryError("rgcn_emb_adam_rows: nodes must be a contiguous vector and row_step a contiguous [N]")
    if int(grad.shape[-2]) != n or int(grad.shape[-1]) != width or (planes > 1 and int(grad.shape[0]) != planes):
        raise RgcnLibraryError(f"rgcn_emb_adam_rows: grad {tuple(grad.shape)} does not hold one row of {width} per listed node ({n})")
    if n == 0:      # (nothing to do; an empty tensor has no address to pass)
        return
    nbytes = 0
    with torch.cuda.device(dev):
        if not assume_unique:
            if workspace is None:
                workspace = torch.empty(lib.rgcn_emb_adam_rows_workspace_bytes(n, n_nodes), dtype=torch.uint8, device=dev)
            nbytes = int(workspace.numel())
        check(lib.rgcn_emb_adam_rows(table.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), row_step.data_ptr(), planes,
                                     table.stride(0) if table.dim() == 3 else 0, n_nodes, width, table.stride(-2), nodes.data_ptr(), n,
                                     grad.data_ptr(), grad.stride(0) if grad.dim() == 3 else 0, grad.stride(-2), lr, beta1, beta2, eps,
                                     weight_decay, int(bool(assume_unique)), _ptr(bad_ids),
                                     None if assume_unique else workspace.data_ptr(), nbytes, _stream(table)), "rgcn_emb_adam_rows")


# ---- link prediction (rgcn_linkpred.hip) -----------------------------------------------------------------------------------
LP_BAD_NODE, LP_BAD_REL = 1, 2      # RGCN_LP_BAD_*: bits of the `bad` word
LP_MAX_KEYS = 0xFFFF0000


def _lp_tables(what: str, z: torch.Tensor, rel: torch.Tensor):
    """(num_nodes, num_relations, width) of ``z [N, E]`` / ``rel [R, E]`` after the checks every rgcn_lp_* call shares: fp32 on
    one GPU, last dimension contiguous, row strides multiples of 4, bases 16-byte aligned (linkpred.py pads what is not)"""
    for name, t in (("z", z), ("rel", rel)):
        if not torch.is_tensor(t) or t.dim() != 2 or t.dtype != torch.float32:
            raise RgcnLibraryError(f"{what}: {name} must be a [rows, width] float32 tensor")
        if t.device.type != "cuda":
            raise RgcnLibraryError(f"{what}: {name} lives on {t.device}; there is no CPU fallback for the link-prediction kernels")
        if (t.shape[1] > 1 and t.stride(1) != 1) or t.stride(0) % 4 != 0 or t.stride(0) < t.shape[1] or t.data_ptr() % 16 != 0:
            raise RgcnLibraryError(f"{what}: {name} needs a contiguous last dimension, a row stride that is a multiple of 4 and a "
                                   f"16-byte aligned base (strides {t.stride()})")
    if rel.device != z.device or rel.shape[1] != z.shape[1]:
        raise RgcnLibraryError(f"{what}: z {tuple(z.shape)} on {z.device} and rel {tuple(rel.shape)} on {rel.device} do not go together")
    return int(z.shape[0]), int(rel.shape[0]), int(z.shape[1])


def _lp_ids(what: str, dev, **vecs) -> int:
    """the common length of int64 id vectors on ``dev``"""
    n = None
    for name, t in vecs.items():
        if not torch.is_tensor(t) or t.dim() != 1 or t.dtype != torch.int64 or t.device != dev or (t.numel() > 1 and t.stride(0) != 1):
            raise RgcnLibraryError(f"{what}: {name} must be a contiguous int64 vector on {dev}")
        if n is not None and int(t.shape[0]) != n:
            raise RgcnLibraryError(f"{what}: {', '.join(vecs)} must have one length")
        n = int(t.shape[0])
    return n


def _lp_bad(what: str, bad: Optional[torch.Tensor], dev) -> None:
    if bad is not None and (bad.dtype != torch.int32 or bad.device != dev or bad.numel() != 1):
        raise RgcnLibraryError(f"{what}: bad must be one int32 on {dev}")


def lp_score(z: torch.Tensor, rel: torch.Tensor, s: torch.Tensor, r: torch.Tensor, o: torch.Tensor,
             bad: Optional[torch.Tensor] = None) -> torch.Tensor:
    """rgcn_lp_score: ``score[t] = sum_k z[s_t, k] rel[r_t, k] z[o_t, k]`` -> float32 [T].  Asynchronous."""
    n_nodes, n_rel, width = _lp_tables("rgcn_lp_score", z, rel)
    n = _lp_ids("rgcn_lp_score", z.device, s=s, r=r, o=o)
    _lp_bad("rgcn_lp_score", bad, z.device)
    score = torch.empty(n, dtype=torch.float32, device=z.device)
    if n:
        with torch.cuda.device(z.device):
            check(load().rgcn_lp_score(z.data_ptr(), z.stride(0), rel.data_ptr(), rel.stride(0), width, n_nodes, n_rel, s.data_ptr(),
                                       r.data_ptr(), o.data_ptr(), n, score.data_ptr(), _ptr(bad), _stream(z)), "rgcn_lp_score")
    return score


class LpIndex:
    """the index of one batch of triples (rgcn_lp_index_build): int32 tensors that hold the library's uint32 values"""

    def __init__(self, node_ptr, node_slot, rel_ptr, rel_triple, n_triples: int, num_nodes: int, num_relations: int):
        self.node_ptr, self.node_slot, self.rel_ptr, self.rel_triple = node_ptr, node_slot, rel_ptr, rel_triple
        self.n_triples, self.num_nodes, self.num_relations = n_triples, num_nodes, num_relations


def lp_index_build(s: torch.Tensor, r: torch.Tensor, o: torch.Tensor, num_nodes: int, num_relations: int,
                   bad: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, nodes: bool = True,
                   relations: bool = True) -> LpIndex:
    """rgcn_lp_index_build on device vectors: a function of (s, r, o) alone.  ``nodes`` / ``relations``: the halves to build (dz
    needs the first, drel the second); the other half's tensors are None.  Asynchronous; the workspace is allocated here when it is
    missing."""
    lib, dev = load(), s.device
    n = _lp_ids("rgcn_lp_index_build", dev, s=s, r=r, o=o)
    if dev.type != "cuda":
        raise RgcnLibraryError(f"rgcn_lp_index_build: the triples live on {dev}; there is no CPU fallback for the link-prediction kernels")
    _lp_bad("rgcn_lp_index_build", bad, dev)
    i32 = dict(dtype=torch.int32, device=dev)
    ix = LpIndex(torch.zeros(num_nodes + 1, **i32) if nodes else None, torch.empty(2 * n, **i32) if nodes else None,
                 torch.zeros(num_relations + 1, **i32) if relations else None, torch.empty(n, **i32) if relations else None,
                 n, int(num_nodes), int(num_relations))
    if n and (nodes or relations):
        with torch.cuda.device(dev):
            if workspace is None:
                workspace = torch.empty(lib.rgcn_lp_index_workspace_bytes(n, num_nodes, num_relations), dtype=torch.uint8, device=dev)
            check(lib.rgcn_lp_index_build(s.data_ptr(), r.data_ptr(), o.data_ptr(), n, num_nodes, num_relations, _ptr(ix.node_ptr),
                                          _ptr(ix.node_slot), _ptr(ix.rel_ptr), _ptr(ix.rel_triple), _ptr(bad),
                                          workspace.data_ptr(), int(workspace.numel()), _stream(s)), "rgcn_lp_index_build")
    return ix


def lp_backward(z: torch.Tensor, rel: torch.Tensor, s: torch.Tensor, r: torch.Tensor, o: torch.Tensor, g: torch.Tensor, ix: LpIndex,
                need_z: bool = True, need_rel: bool = True, workspace: Optional[torch.Tensor] = None):
    """rgcn_lp_backward: ``(dz, drel)`` from ``g [T]`` and the index of the same triples; ``None`` for a gradient that is not
    wanted.  The gradients are [rows, E] views of buffers whose rows are padded to a multiple of 4.  Asynchronous."""
    lib, dev = load(), z.device
    n_nodes, n_rel, width = _lp_tables("rgcn_lp_backward", z, rel)
    n = _lp_ids("rgcn_lp_backward", dev, s=s, r=r, o=o)
    if g.dtype != torch.float32 or g.device != dev or g.dim() != 1 or int(g.shape[0]) != n or (n > 1 and g.stride(0) != 1):
        raise RgcnLibraryError(f"rgcn_lp_backward: g must be a contiguous float32 [{n}] on {dev}")
    if (ix.n_triples, ix.num_nodes, ix.num_relations) != (n, n_nodes, n_rel):
        raise RgcnLibraryError("rgcn_lp_backward: the index was built for other sizes")
    ld = (width + 3) // 4 * 4
    make = torch.empty if n else torch.zeros       # (no triples: nothing is launched, the gradients are zero)
    dz = make(n_nodes, ld, dtype=torch.float32, device=dev) if need_z else None
    drel = make(n_rel, ld, dtype=torch.float32, device=dev) if need_rel else None
    if n and (need_z or need_rel):
        with torch.cuda.device(dev):
            nbytes = 0
            if need_rel:
                if workspace is None:
                    workspace = torch.empty(lib.rgcn_lp_backward_workspace_bytes(n, n_rel, width), dtype=torch.uint8, device=dev)
                nbytes = int(workspace.numel())
            check(lib.rgcn_lp_backward(z.data_ptr(), z.stride(0), rel.data_ptr(), rel.stride(0), width, n_nodes, n_rel, s.data_ptr(),
                                       r.data_ptr(), o.data_ptr(), n, g.data_ptr(), _ptr(ix.node_ptr), _ptr(ix.node_slot),
                                       _ptr(ix.rel_ptr), _ptr(ix.rel_triple), _ptr(dz), ld, _ptr(drel), ld,
                                       workspace.data_ptr() if need_rel else None, nbytes, _stream(z)), "rgcn_lp_backward")
    return (None if dz is None else dz[:, :width]), (None if drel is None else drel[:, :width])


def lp_corrupt(s: torch.Tensor, r: torch.Tensor, o: torch.Tensor, num_nodes: int, num_negatives: int, seed: int):
    """rgcn_lp_corrupt: ``(s', r', o')``, each int64 [T * num_negatives]; position ``i * num_negatives + j`` is negative j of
    triple i.  Asynchronous."""
    dev = s.device
    n = _lp_ids("rgcn_lp_corrupt", dev, s=s, r=r, o=o)
    if dev.type != "cuda":
        raise RgcnLibraryError(f"rgcn_lp_corrupt: the triples live on {dev}; there is no CPU fallback for the link-prediction kernels")
    out = [torch.empty(n * num_negatives, dtype=torch.int64, device=dev) for _ in range(3)]
    with torch.cuda.device(dev):
        check(load().rgcn_lp_corrupt(s.data_ptr(), r.data_ptr(), o.data_ptr(), n, num_nodes, num_negatives, seed, out[0].data_ptr(),
                                     out[1].data_ptr(), out[2].data_ptr(), _stream(s)), "rgcn_lp_corrupt")
    return tuple(out)


def lp_rank(z: torch.Tensor, rel: torch.Tensor, anchor: torch.Tensor, r: torch.Tensor, target: torch.Tensor,
            filter_ptr: Optional[torch.Tensor] = None, filter_idx: Optional[torch.Tensor] = None,
            workspace: Optional[torch.Tensor] = None):
    """rgcn_lp_rank: ``(greater, equal)`` int64 [Q] of the queries (anchor, r, target) over the candidates that are neither the
    target nor in the query's filter list (CSR ``filter_ptr [Q + 1]`` / ``filter_idx``, int64; None: raw ranks).  Asynchronous."""
    lib, dev = load(), z.device
    n_nodes, n_rel, width = _lp_tables("rgcn_lp_rank", z, rel)
    n = _lp_ids("rgcn_lp_rank", dev, anchor=anchor, r=r, target=target)
    flen = 0
    if filter_ptr is not None:
        _lp_ids("rgcn_lp_rank", dev, filter_ptr=filter_ptr)
        _lp_ids("rgcn_lp_rank", dev, filter_idx=filter_idx)
        if int(filter_ptr.shape[0]) != n + 1:
            raise RgcnLibraryError(f"rgcn_lp_rank: filter_ptr holds {int(filter_ptr.shape[0])} entries for {n} queries")
        flen = int(filter_idx.shape[0])
    greater = torch.empty(n, dtype=torch.int64, device=dev)
    equal = torch.empty(n, dtype=torch.int64, device=dev)
    if n:
        with torch.cuda.device(dev):
            if workspace is None:
                workspace = torch.empty(lib.rgcn_lp_rank_workspace_bytes(n, n_nodes, width), dtype=torch.uint8, device=dev)
            check(lib.rgcn_lp_rank(z.data_ptr(), z.stride(0), rel.data_ptr(), rel.stride(0), width, n_nodes, n_rel, anchor.data_ptr(),
                                   r.data_ptr(), target.data_ptr(), n, _ptr(filter_ptr), _ptr(filter_idx) if flen else None, flen,
                                   greater.data_ptr(), equal.data_ptr(), workspace.data_ptr(), int(workspace.numel()), _stream(z)),
                  "rgcn_lp_rank")
    return greater, equal


# ---- summaries -> original graph (rgcn_transfer.hip; transfer.py validates and drives them) ---------------------------------
TR_BAD_BLOCK, TR_BAD_NODE, TR_BAD_MAP = 1, 2, 4      # RGCN_TR_BAD_*: bits of the `bad` word
TR_MAX_TABLES = 16
TR_MODES = {"stack": 0, "concat": 1, "sum": 2}       # RGCN_TR_STACK / _CONCAT / _SUM


def tr_block_labels(block: torch.Tensor, num_blocks: int, train_idx: torch.Tensor, y: torch.Tensor, bad: Optional[torch.Tensor] = None):
    """rgcn_tr_block_labels on contiguous int64 device tensors ``block [N]``, ``train_idx [L]``, ``y [L, C]`` ->
    ``(size int32 [B], y_sum float32 [B, C], nonzero int32 [B])``.  Asynchronous on the current stream of ``block``'s device."""
    lib, dev = load(), block.device
    n, l, c = int(block.shape[0]), int(train_idx.shape[0]), int(y.shape[1])
    nbytes = lib.rgcn_tr_block_labels_workspace_bytes(n, int(num_blocks), l, c)
    if nbytes == 0:
        raise RgcnLibraryError("rgcn_tr_block_labels_workspace_bytes: bad arguments")
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        size = torch.empty(num_blocks, dtype=torch.int32, device=dev)
        nonzero = torch.empty(num_blocks, dtype=torch.int32, device=dev)
        y_sum = torch.empty(num_blocks, c, dtype=torch.float32, device=dev)
        check(lib.rgcn_tr_block_labels(block.data_ptr() if n else None, n, int(num_blocks), train_idx.data_ptr() if l else None,
                                       y.data_ptr() if l else None, c, l, c, size.data_ptr(), y_sum.data_ptr(), c, nonzero.data_ptr(),
                                       _ptr(bad), ws.data_ptr(), nbytes, _stream(block)), "rgcn_tr_block_labels")
    return size, y_sum, nonzero


def tr_gather(tables, maps, num_nodes: int, width: int, nodes: Optional[torch.Tensor], mode: int, seed: int, out: torch.Tensor,
              bad: Optional[torch.Tensor] = None) -> None:
    """rgcn_tr_gather into ``out`` (contiguous: [S, M, E], [M, S E] or [M, E] by ``mode``); ``tables``: fp32 [B_s, E] device
    tensors with a contiguous last dimension (any row stride), ``maps``: contiguous int64 [N], ``nodes``: contiguous int64 [M] or
    None.  Asynchronous on the current stream of ``out``'s device."""
    s = len(tables)
    m = int(num_nodes) if nodes is None else int(nodes.shape[0])
    if m == 0:      # (nothing to write; an empty tensor has no address to pass)
        return
    tabs = (C.c_void_p * s)(*[t.data_ptr() if t.shape[0] else None for t in tables])
    lds = (C.c_int32 * s)(*[int(t.stride(0)) if t.shape[0] > 1 else int(width) for t in tables])
    rows = (C.c_int64 * s)(*[int(t.shape[0]) for t in tables])
    mps = (C.c_void_p * s)(*[mp.data_ptr() for mp in maps])
    with torch.cuda.device(out.device):
        check(load().rgcn_tr_gather(tabs, lds, rows, mps, s, int(width), int(num_nodes), _ptr(nodes), m, int(mode), int(seed),
                                    out.data_ptr(), int(out.stride(-2)), int(out.stride(0)) if out.dim() == 3 else 0, _ptr(bad),
                                    _stream(out)), "rgcn_tr_gather")


# ---- bipartite layers: the root term (rgcn_rows.hip) ------------------------------------------------------------------
def rows_transform(x: torch.Tensor, din: int, w: torch.Tensor, dout: int, transpose: bool = False,
                   add: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                   y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = add + x @ W + bias over the rows of x (rgcn_rows_transform): W = ``w [din, dout]``, or with ``transpose`` the
    transpose of ``w [dout, din]``.  ``add`` may be ``y`` itself; without ``y`` a padded [rows, dout rounded up to 4] buffer
    is allocated.  Returns y."""
    rows = int(x.shape[0])
    if y is None:
        y = torch.empty(rows, (dout + 3) // 4 * 4, dtype=torch.float32, device=x.device)
    if y.shape[0] != rows or (add is not None and add.shape[0] != rows):
        raise RgcnLibraryError("rgcn_rows_transform: x, add and y must have the same number of rows")
    if rows == 0:       # (nothing to write; an empty tensor has no address to pass)
        return y
    with torch.cuda.device(x.device):
        check(load().rgcn_rows_transform(x.data_ptr(), x.stride(0), din, w.data_ptr(), int(transpose), _ptr(add),
                                         0 if add is None else add.stride(0), _ptr(bias), y.data_ptr(), y.stride(0), dout, rows,
                                         _stream(x)), "rgcn_rows_transform")
    return y


def rows_dw(x: torch.Tensor, din: int, g: torch.Tensor, dout: int) -> torch.Tensor:
    """d_w [din, dout] = x^T g (rgcn_rows_dw): rows of x and g pair up one to one; no rows: zeros."""
    lib = load()
    if x.shape[0] != g.shape[0]:
        raise RgcnLibraryError("rgcn_rows_dw: x and g must have the same number of rows")
    d_w = torch.empty(din, dout, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        ws = torch.empty(lib.rgcn_rows_dw_workspace_bytes(din, dout), dtype=torch.uint8, device=x.device)
        check(lib.rgcn_rows_dw(x.data_ptr(), x.stride(0), din, g.data_ptr(), g.stride(0), dout, int(x.shape[0]), ws.data_ptr(),
                               ws.numel(), d_w.data_ptr(), _stream(x)), "rgcn_rows_dw")
    return d_w


# ---- edge-parallel path (eplan.EdgePlan) ----------------------------------------------------------------------------
def _units_struct(owner, attr: str, units, n_gathered: int, slot_src: torch.Tensor, num_relations: int) -> RgcnEdgeUnits:
    """The struct rgcn_edge_units of ``units`` (an eplan.EdgePlan or HeavyPart: unit_rel, unit_cnt, slot_w) gathering the rows
    ``slot_src`` of a matrix of ``n_gathered`` rows, built once and kept on ``owner`` under ``attr`` (the plan's tensors never
    change)."""
    cached = getattr(owner, attr, None)
    if cached is None:
        if slot_src.device.type != "cuda":
            raise RgcnLibraryError("the edge plan must live on the GPU (plan tensors are on %s)" % slot_src.device)
        cached = RgcnEdgeUnits(n_gathered, units.n_units, num_relations, 0, units.unit_rel.data_ptr(), units.unit_cnt.data_ptr(),
                               slot_src.data_ptr(), units.slot_w.data_ptr())
        setattr(owner, attr, cached)
    return cached


def edge_units_struct(ep) -> RgcnEdgeUnits:
    """the light units of an eplan.EdgePlan: they gather rows of the layer's input"""
    return _units_struct(ep, "_cunits", ep, ep.n_nodes, ep.slot_src, ep.num_relations)


def ep_segment_sum(src: torch.Tensor, ptr: torch.Tensor, idx, w, n_out: int, width: int, out: torch.Tensor, bias=None,
                   act: int = ACT_NONE, mask=None, final: bool = False) -> None:
    with torch.cuda.device(src.device):
        check(load().rgcn_ep_segment_sum(src.data_ptr(), src.stride(0), ptr.data_ptr(), _ptr(idx), _ptr(w), n_out, width,
                                         _ptr(bias), int(act), _ptr(mask), mask.stride(0) if mask is not None else 0, int(final),
                                         out.data_ptr(), out.stride(0), _stream(src)), "rgcn_ep_segment_sum")


def _sum_levels(levels, src: torch.Tensor, width: int, ld: int, out: Optional[torch.Tensor] = None, bias=None, act: int = ACT_NONE,
                mask=None, final: bool = False) -> torch.Tensor:
    """``src`` through one rgcn_ep_segment_sum per entry of ``levels`` -- (seg_ptr, seg_idx, seg_w, n_out), or (seg_ptr, seg_idx,
    n_out) unweighted -- each level reading the one before it.  Intermediate levels go to fresh [max(n_out, 1), ld] buffers; the
    last level goes to ``out`` where the caller gives one, and it alone takes bias, activation, mask and the ``final`` flag.
    Returns what the last level wrote (``src`` itself without a level)."""
    cur = src
    for li, lv in enumerate(levels):
        ptr, idx, w, n_out = lv if len(lv) == 4 else (lv[0], lv[1], None, lv[2])
        last = li == len(levels) - 1
        dst = out if last and out is not None else torch.empty(max(n_out, 1), ld, dtype=torch.float32, device=src.device)
        if last:
            ep_segment_sum(cur, ptr, idx, w, n_out, width, dst, bias, act, mask, final)
        else:
            ep_segment_sum(cur, ptr, idx, w, n_out, width, dst)
        cur = dst
    return cur


def ep_aggregate_heavy(ep, x: torch.Tensor, din: int) -> Optional[torch.Tensor]:
    """H[seg] = sum_e w_e x[src_e] over the rows of every heavy (destination, relation) segment of the plan (eplan.HeavyPart):
    rgcn_ep_segment_sum over x itself, weighted, in levels.  None when the plan has no heavy part."""
    h = ep.heavy
    if h is None:
        return None
    if h.shared is not None:
        raise RgcnLibraryError("this plan's heavy segments are shared across ranks: H comes from ep_aggregate_shared + all-reduce")
    return _sum_levels(h.levels, x, din, x.stride(0))


def ep_aggregate_shared(shared, x: torch.Tensor, din: int) -> torch.Tensor:
    """this rank's share of H[seg] = sum_e w_e x[src_e] over the heavy segments of the whole graph (eplan.SharedHeavy): zeros but
    for the segments its rows belong to; the all-reduce over the ranks (conv.py) completes it"""
    hmat = torch.zeros(max(shared.n_seg, 1), x.stride(0), dtype=torch.float32, device=x.device)
    if shared.levels:      # (the last level's n_out segments start at seg_lo)
        _sum_levels(shared.levels, x, din, x.stride(0), out=hmat[shared.seg_lo:shared.seg_lo + shared.levels[-1][3]])
    return hmat


def ep_layer(ep, x: torch.Tensor, din: int, packed: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, dout: int,
             act: int = ACT_NONE, mask: Optional[torch.Tensor] = None, flags: int = 0, hmat: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """out[:n_owned] = act(bias + sum over the plan's rows of w * (x[src] @ W_rel)) * (mask > 0): the heavy segments' rows
    summed first (ep_aggregate_heavy), rgcn_ep_transform over the units (and over the heavy part's pseudo rows, gathered from
    H), then one rgcn_ep_segment_sum per level of the plan.  ``out``: [n_owned, ld] with ld a multiple of 4.  Returns H (the
    weight gradients of the heavy part need it) or None."""
    lib = load()
    ldz = out.stride(0)
    st = _stream(x)
    h = ep.heavy
    if hmat is None:      # (given: the all-reduced H of the heavy segments shared across ranks)
        hmat = ep_aggregate_heavy(ep, x, din)
    with torch.cuda.device(x.device):
        n_light = ep.n_units * 64
        z = torch.empty(max(n_light + (h.n_units * 64 if h is not None else 0), 1), ldz, dtype=torch.float32, device=x.device)
        check(lib.rgcn_ep_transform(C.byref(edge_units_struct(ep)), x.data_ptr(), x.stride(0), din, packed.data_ptr(),
                                    z.data_ptr(), ldz, dout, int(flags), st), "rgcn_ep_transform")
        if h is not None:
            hu = _units_struct(h, "_cunits", h, h.n_seg, h.slot_src, ep.num_relations)      # (the pseudo rows gather rows of H)
            check(lib.rgcn_ep_transform(C.byref(hu), hmat.data_ptr(), hmat.stride(0), din, packed.data_ptr(),
                                        z[n_light:].data_ptr(), ldz, dout, int(flags), st), "rgcn_ep_transform (heavy part)")
    _sum_levels(ep.levels, z, dout, ldz, out, bias, act, mask, final=True)
    return hmat


def eplan_segments(slot_row: torch.Tensor, n_owned: int):
    """(seg_ptr int32 [n_owned + 1], seg_idx int32 [real slots]) of a relation-major plan's slots (rgcn_eplan_segments)"""
    lib = load()
    n_slots = int(slot_row.numel())
    dev = slot_row.device
    seg_ptr = torch.empty(n_owned + 1, dtype=torch.int32, device=dev)
    seg_idx = torch.empty(max(n_slots, 1), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws = torch.empty(lib.rgcn_plan_workspace_bytes(n_slots, 0, 1, 16), dtype=torch.uint8, device=dev)
        check(lib.rgcn_eplan_segments(slot_row.data_ptr(), n_slots, int(n_owned), ws.data_ptr(), ws.numel(), seg_ptr.data_ptr(),
                                      seg_idx.data_ptr(), _stream(slot_row)), "rgcn_eplan_segments")
    return seg_ptr, seg_idx


# ---- max aggregation (eplan.MaxPlan, csrc/rgcn_segmax.hip) -----------------------------------------------------------
def segment_max(src: torch.Tensor, src_t: Optional[torch.Tensor], ptr: torch.Tensor, idx, w, n_out: int, width: int,
                out: torch.Tensor, out_t: Optional[torch.Tensor]) -> None:
    """one level of rgcn_segment_max: (src, src_t) and (out, out_t) share their strides"""
    with torch.cuda.device(src.device):
        check(load().rgcn_segment_max(src.data_ptr(), _ptr(src_t), src.stride(0), ptr.data_ptr(), _ptr(idx), _ptr(w), int(n_out),
                                      int(width), out.data_ptr(), _ptr(out_t), out.stride(0), _stream(src)), "rgcn_segment_max")


def _max_plan_on(mp, device) -> None:
    """a max plan's arrays must live on the device of the operands: the kernels read them as device pointers"""
    h = mp.ep.heavy
    ts = [mp.ep.slot_src] + ([] if h is None else [h.slot_src] + [lv[0] for lv in h.levels]) + [lv[0] for lv in mp.bwd_levels]
    if any(t.device != device for t in ts):
        raise RgcnLibraryError(f"the max plan must live on {device} (plan tensors are on {ts[0].device})")


def max_aggregate(mp, x: torch.Tensor, din: int, with_t: bool):
    """(H, T) of a max plan's segments: rgcn_segment_max over x, level by level (T: None unless ``with_t``).  (None, None)
    without an edge."""
    _max_plan_on(mp, x.device)
    h = mp.ep.heavy
    if h is None:
        return None, None
    cur, cur_t = x, None
    for ptr, idx, w, n_out in h.levels:
        dst = torch.empty(max(n_out, 1), x.stride(0), dtype=torch.float32, device=x.device)
        dst_t = torch.empty_like(dst) if with_t else None
        segment_max(cur, cur_t, ptr, idx, w, n_out, din, dst, dst_t)
        cur, cur_t = dst, dst_t
    return cur, cur_t


def max_layer_dx(mp, x: torch.Tensor, hmat: Optional[torch.Tensor], tmat: Optional[torch.Tensor], g: torch.Tensor, dout: int,
                 packed_t: torch.Tensor, dx: torch.Tensor, din: int, mask: Optional[torch.Tensor] = None, flags: int = 0) -> None:
    """dX of a max layer into ``dx`` [n, ld]: dH per pseudo slot (rgcn_ep_transform over g with W^T), C per segment row
    (rgcn_segment_max_bwd), the root rows g root^T (rgcn_ep_transform over the light units), then rgcn_ep_segment_sum by source
    in the levels of ``mp.bwd_levels`` with the ReLU mask of the layer input"""
    lib = load()
    _max_plan_on(mp, g.device)
    ep, h = mp.ep, mp.ep.heavy
    ldx = dx.stride(0)
    st = _stream(g)
    y = torch.empty(max(mp.n_hrows + ep.n_units * 64, 1), ldx, dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device):
        if h is not None:
            units = _units_struct(mp, "_bwd_cunits", h, ep.n_nodes, mp.bwd_slot_src, ep.num_relations)      # (they gather g[destination])
            dh = torch.empty(max(h.n_units * 64, 1), ldx, dtype=torch.float32, device=g.device)
            check(lib.rgcn_ep_transform(C.byref(units), g.data_ptr(), g.stride(0), dout, packed_t.data_ptr(), dh.data_ptr(), ldx, din,
                                        int(flags), st), "rgcn_ep_transform (max dH)")
            check(lib.rgcn_segment_max_bwd(x.data_ptr(), x.stride(0), hmat.data_ptr(), tmat.data_ptr(), hmat.stride(0), dh.data_ptr(), ldx,
                                           mp.row_src.data_ptr(), mp.row_seg.data_ptr(), mp.seg_dh.data_ptr(), _ptr(mp.row_w),
                                           mp.n_hrows, din, y.data_ptr(), ldx, st), "rgcn_segment_max_bwd")
        check(lib.rgcn_ep_transform(C.byref(edge_units_struct(ep)), g.data_ptr(), g.stride(0), dout, packed_t.data_ptr(),
                                    y[mp.n_hrows:].data_ptr(), ldx, din, int(flags), st), "rgcn_ep_transform (max root rows)")
    _sum_levels(mp.bwd_levels, y, din, ldx, dx, mask=mask, final=True)


# ---- featureless layers (csrc/rgcn_featureless.hip) -----------------------------------------------------------------
def featureless_geometry(n_nodes: int, dout: int, num_bases: int):
    """(tile, chunk) of the featureless plans (rgcn_featureless_geometry)"""
    tile, chunk = C.c_int(), C.c_int()
    check(load().rgcn_featureless_geometry(int(n_nodes), int(dout), int(num_bases), C.byref(tile), C.byref(chunk)),
          "rgcn_featureless_geometry")
    return tile.value, chunk.value


def featureless_fwd(ps: RgcnPlanStruct, x_index: Optional[torch.Tensor], in_rows: int, weight: torch.Tensor,
                    comp: Optional[torch.Tensor], root: Optional[torch.Tensor], bias: Optional[torch.Tensor], out: torch.Tensor,
                    dout: int) -> None:
    nb = 0 if comp is None else int(comp.shape[1])
    with torch.cuda.device(weight.device):
        check(load().rgcn_featureless_fwd(C.byref(ps), _ptr(x_index), int(in_rows), weight.data_ptr(), _ptr(comp), nb, _ptr(root),
                                          _ptr(bias), out.data_ptr(), out.stride(0), int(dout), _stream(weight)), "rgcn_featureless_fwd")


def featureless_bwd(ps_t: RgcnPlanStruct, x_index: Optional[torch.Tensor], inv: Optional[tuple], in_rows: int, g: torch.Tensor,
                    dout: int, weight: torch.Tensor, comp: Optional[torch.Tensor], d_weight, d_comp, d_root, d_bias) -> None:
    """gradients of rgcn_featureless_fwd on the transposed plan; ``inv`` = (inv_ptr, inv_idx) of an integer x"""
    lib = load()
    nb = 0 if comp is None else int(comp.shape[1])
    nbytes = lib.rgcn_featureless_bwd_workspace_bytes(C.byref(ps_t), int(dout), nb, int(x_index is not None))
    if nbytes == 0:
        raise RgcnLibraryError("rgcn_featureless_bwd_workspace_bytes refused the plan")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=g.device)
    ip, ii = inv if inv is not None else (None, None)
    with torch.cuda.device(g.device):
        check(lib.rgcn_featureless_bwd(C.byref(ps_t), _ptr(x_index), _ptr(ip), _ptr(ii), int(in_rows), g.data_ptr(), g.stride(0),
                                       int(dout), weight.data_ptr(), _ptr(comp), nb, ws.data_ptr(), nbytes, _ptr(d_weight),
                                       _ptr(d_comp), _ptr(d_root), _ptr(d_bias), _stream(g)), "rgcn_featureless_bwd")


# ---- layers wider than 128 (csrc/rgcn_xwide.hip) --------------------------------------------------------------------
def xwide_geometry(n_nodes: int, din: int, dout: int):
    """(tile, chunk) of the forward and transposed plans of a wide layer (rgcn_xwide_geometry)"""
    tile, chunk = C.c_int(), C.c_int()
    check(load().rgcn_xwide_geometry(int(n_nodes), int(din), int(dout), C.byref(tile), C.byref(chunk)), "rgcn_xwide_geometry")
    return tile.value, chunk.value


def xwide_fwd(ps: RgcnPlanStruct, x: torch.Tensor, din: int, weight: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor,
              dout: int, act: int = ACT_NONE) -> None:
    """``weight``: the row-major operand [R' + 1, din, dout] (root last)"""
    with torch.cuda.device(x.device):
        check(load().rgcn_xwide_fwd(C.byref(ps), x.data_ptr(), x.stride(0), int(din), weight.data_ptr(), _ptr(bias), out.data_ptr(),
                                    out.stride(0), int(dout), int(act), _stream(x)), "rgcn_xwide_fwd")


def xwide_bwd_dx(ps_t: RgcnPlanStruct, g: torch.Tensor, dout: int, weight_t: torch.Tensor, dx: torch.Tensor, din: int,
                 relu_of: Optional[torch.Tensor] = None) -> None:
    """``weight_t``: the row-major operand [R' + 1, dout, din] (blocks W_r^T, root last)"""
    with torch.cuda.device(g.device):
        check(load().rgcn_xwide_bwd_dx(C.byref(ps_t), g.data_ptr(), g.stride(0), int(dout), weight_t.data_ptr(), dx.data_ptr(),
                                       dx.stride(0), int(din), _ptr(relu_of), 0 if relu_of is None else relu_of.stride(0), _stream(g)),
              "rgcn_xwide_bwd_dx")


def xwide_bwd_dw(ps: RgcnPlanStruct, x: torch.Tensor, din: int, g: torch.Tensor, dout: int, d_weight: Optional[torch.Tensor],
                 d_root: Optional[torch.Tensor], d_bias: Optional[torch.Tensor]) -> None:
    lib = load()
    nbytes = lib.rgcn_xwide_bwd_dw_workspace_bytes(C.byref(ps), int(din), int(dout))
    if nbytes == 0:
        raise RgcnLibraryError("rgcn_xwide_bwd_dw_workspace_bytes refused the plan")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        check(lib.rgcn_xwide_bwd_dw(C.byref(ps), x.data_ptr(), x.stride(0), int(din), g.data_ptr(), g.stride(0), int(dout),
                                    ws.data_ptr(), nbytes, _ptr(d_weight), _ptr(d_root), _ptr(d_bias), _stream(x)), "rgcn_xwide_bwd_dw")
