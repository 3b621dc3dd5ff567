"""Op-level drop-ins over the C ABI (SURVEY.md §8b "op-level boundary"): the third-party functional calls the
reference's layers sit on, with the same argument meaning, for hosts that keep the reference's Python modules and
swap only these ops.  Everything runs on the HIP device; CPU tensors raise (no fallback).

=====================================================  ==========================================================
reference call                                          here
=====================================================  ==========================================================
``torch_geometric.nn.knn_graph(x, k, batch, flow)``     :func:`knn_graph`         (uni_transformer_edge.py:353)
``scatter_softmax(...); scatter_sum(alpha * v, ...)``   :func:`scatter_attention` (uni_transformer_edge.py:63-68,158-164)
the same with ``v.unsqueeze(-1) * rel_x`` and ``mean``  :func:`scatter_attention_pos` (uni_transformer_edge.py:199-211)
``BondUpdateLayer.triplets(edge_index, num_nodes)``     :func:`triplets`          (uni_transformer_edge.py:103-123)
``torch_sparse.SparseTensor`` as that method uses it    :class:`SparseTensor`     (uni_transformer_edge.py:108-122)
=====================================================  ==========================================================
"""
from __future__ import annotations

from typing import Optional

import torch

from . import hip_lib
from .batch_layout import N_MAX

# ------------------------------------------------------------------------------------------------------------------
# The compiled torch extension (csrc/torch_ext.cpp -> lib/decompdiff_torch_ext.so: TORCH_LIBRARY(decompdiff_hip, ...),
# HIP-key kernels that launch the same C-ABI entry points on torch's current stream).  When it is present the ops below
# go through the dispatcher (torch.ops.decompdiff_hip.*); otherwise -- extension not built, or another library build
# selected with DD_HIP_LIB (the extension is linked against the default one) -- through the ctypes binding of the same
# entry points.  DD_TORCH_EXT=0 forces ctypes.  Either way the arithmetic is the HIP library's: no CPU path.
# ------------------------------------------------------------------------------------------------------------------
import os as _os

_EXT_PATH = _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "lib", "decompdiff_torch_ext.so")
_ext_state = {"tried": False, "ops": None}


def torch_ext():
    """torch.ops.decompdiff_hip (compiled extension) or None."""
    if not _ext_state["tried"]:
        _ext_state["tried"] = True
        if _os.environ.get("DD_TORCH_EXT", "1") != "0" and not _os.environ.get("DD_HIP_LIB") and _os.path.exists(_EXT_PATH):
            try:
                torch.ops.load_library(_EXT_PATH)
                if int(torch.ops.decompdiff_hip.abi_version()) == hip_lib.ABI_VERSION:
                    _ext_state["ops"] = torch.ops.decompdiff_hip
            except (OSError, RuntimeError):                  # toolchain skew: the ctypes binding serves the same entry points
                _ext_state["ops"] = None
    return _ext_state["ops"]


def knn_graph(x: torch.Tensor, k: int, batch: Optional[torch.Tensor] = None, loop: bool = False,
              flow: str = "source_to_target") -> torch.Tensor:
    """``edge_index [2,E]`` (row 0 = neighbour / source, row 1 = centre / target), grouped by centre in ascending
    order, neighbours by ascending distance, self loops excluded, candidates restricted to the same ``batch`` id — the
    order torch_cluster returns.  ``batch`` must be sorted (torch_cluster requires that too); the samples may have any
    sizes and ids may be missing -- a PyG ``Batch`` of different complexes (``dd_knn_csr``); equal counts of at most 2048
    atoms take the dense kernel (``dd_knn``), with the same result.  A sample with fewer than ``k`` other atoms
    contributes all of them.  ``loop=True`` makes the centre a candidate of its own list;
    ``flow='target_to_source'`` swaps the two rows, as torch_geometric does."""
    if flow not in ("source_to_target", "target_to_source"):
        raise ValueError(f"knn_graph: flow '{flow}'")
    hip_lib.require_gpu(x, "x")
    if x.dim() != 2 or x.size(1) != 3:
        raise ValueError("knn_graph: x must be [n,3]")
    n, k, dev = x.size(0), int(k), x.device
    swap = (lambda e: e.flip(0)) if flow == "target_to_source" else (lambda e: e)
    if n == 0 or k <= 0:
        return torch.empty(2, 0, dtype=torch.long, device=dev)
    dense = not loop
    if batch is None:
        B, N = 1, n
    else:
        if batch.dim() != 1 or batch.numel() != n:
            raise ValueError("knn_graph: batch must have one entry per row of x")
        B = int(batch.max().item()) + 1
        N = n // B
        dense = dense and n % B == 0 and torch.equal(batch, torch.arange(B, device=dev).repeat_interleave(N))
    xc = x.detach().to(torch.float32).contiguous()
    if not dense or N > N_MAX:
        return swap(_knn_graph_csr(xc, k, batch, B, loop))
    kk = min(k, N - 1)
    if kk <= 0:
        return torch.empty(2, 0, dtype=torch.long, device=dev)
    ext = torch_ext()
    if ext is not None:
        nbr = ext.knn(xc.view(B, N, 3), kk)
    else:
        nbr = torch.empty(B, N, kk, dtype=torch.int32, device=x.device)
        hip_lib.check(hip_lib.load().dd_knn(hip_lib.ptr(xc), B, N, kk, hip_lib.ptr(nbr), hip_lib.stream_ptr(x.device)), "dd_knn")
    base = (torch.arange(B, device=x.device) * N).view(B, 1, 1)
    src = (nbr.long() + base).reshape(-1)
    dst = torch.arange(n, device=x.device).repeat_interleave(kk)
    return swap(torch.stack([src, dst], 0))


def _knn_graph_csr(xc: torch.Tensor, k: int, batch: Optional[torch.Tensor], B: int, loop: bool) -> torch.Tensor:
    """``edge_index`` of a flat batch with any count per sample (dd_knn_csr): sample offsets and the edge prefix sums are
    made here (one device -> host copy for E and the largest sample), the kernel writes global int64 rows."""
    n, dev = xc.size(0), xc.device
    if batch is None:
        counts = torch.tensor([n], device=dev)
    else:
        if batch.numel() > 1 and bool((batch[1:] < batch[:-1]).any().item()):
            raise NotImplementedError("knn_graph: batch must be sorted (non-decreasing), as torch_cluster requires")
        counts = torch.bincount(batch, minlength=B)
    if k > 64:
        raise NotImplementedError("knn_graph: k <= 64 (DD_KNN_MAX)")
    kb = (counts - (0 if loop else 1)).clamp(min=0, max=k)
    ptr = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    ptr[1:] = counts.cumsum(0)
    out_off = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    out_off[1:] = (counts * kb).cumsum(0)
    E, n_max = torch.stack([out_off[-1], counts.max()]).tolist()
    ext = torch_ext()
    if ext is not None:
        return ext.knn_csr(xc, ptr, out_off, E, n_max, k, bool(loop))
    edge_index = torch.empty(2, E, dtype=torch.int64, device=dev)
    hip_lib.check(hip_lib.load().dd_knn_csr(hip_lib.ptr(xc), hip_lib.ptr(ptr), B, n, n_max, k, int(bool(loop)), hip_lib.ptr(out_off), E,
                                            hip_lib.ptr(edge_index), hip_lib.stream_ptr(dev)), "dd_knn_csr")
    return edge_index


def _seg_ptr(index: torch.Tensor, dim_size: int) -> torch.Tensor:
    if index.numel() > 1 and bool((index[1:] < index[:-1]).any().item()):
        raise NotImplementedError(_UNSORTED)
    ptr = torch.zeros(dim_size + 1, dtype=torch.int32, device=index.device)
    ptr[1:] = torch.bincount(index, minlength=dim_size).cumsum(0)
    return ptr


_UNSORTED = ("scatter_attention: edges must be grouped by destination (sorted index), as knn_graph, "
             "the dst-major bond list and the SparseTensor triplets are")


def _attn_seg(index, dim_size: int, E: int) -> torch.Tensor:
    """Segment pointer of an index vector, or of a SegmentPlan (no device -> host round trip: usable in a captured step)."""
    if isinstance(index, SegmentPlan):
        if index.perm is not None:
            raise NotImplementedError(_UNSORTED)
        if int(dim_size) != index.n or index.E != E:
            raise ValueError("SegmentPlan does not match k / dim_size")
        return index.ptr
    if index.dim() != 1 or index.numel() != E:
        raise ValueError("scatter_attention: index must have one entry per row of k")
    return _seg_ptr(index, dim_size)


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).reshape(t.size(0), -1).contiguous()


def _ew32(e_w: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if e_w is None else e_w.detach().to(torch.float32).reshape(-1).contiguous()


def _needs_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _grad_like(g: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """A gradient computed on the fp32 contiguous copy of t, in t's own shape and dtype."""
    return g.view(t.shape).to(t.dtype)


def _per_edge(q: torch.Tensor, E: int, dim_size: int) -> bool:
    return q.size(0) == E and q.size(0) != dim_size


def _member_mask(member_mask, k: torch.Tensor, what: str) -> Optional[torch.Tensor]:
    """The mask as the kernels read it: one byte per member (uint8; a bool tensor is viewed, not copied), non-zero = real."""
    if member_mask is None:
        return None
    if not torch.is_tensor(member_mask) or member_mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{what}: member_mask must be a bool or uint8 tensor")
    if member_mask.dim() != 1 or member_mask.numel() != k.size(0):
        raise ValueError(f"{what}: member_mask must be [E], one entry per row of k")
    if member_mask.device != k.device:
        raise ValueError(f"{what}: member_mask must be on the device of k ({k.device}, got {member_mask.device})")
    m = member_mask.detach().contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def _attention_node(q, k, v, e_w, seg: torch.Tensor, dim_size: int, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    per_edge = _per_edge(q, k.size(0), dim_size)
    ew = _ew32(e_w)
    # converted copies are bound to locals that outlive the launch: a temporary freed before the kernel is enqueued
    # would hand its block to the next same-size allocation (k and v would alias)
    qf, kf, vf = _f32(q), _f32(k), _f32(v)
    ext = torch_ext()
    if ext is not None:
        return ext.attn_aggregate_node(qf, bool(per_edge), kf, vf, ew, seg, mask)
    out = torch.empty(dim_size, 128, device=k.device)
    hip_lib.check(hip_lib.load().dd_attn_aggregate_node_masked(                     # (mask None = NULL: all members are real)
        hip_lib.ptr(qf), int(per_edge), hip_lib.ptr(kf), hip_lib.ptr(vf), hip_lib.ptr(ew), hip_lib.ptr(seg), dim_size,
        hip_lib.ptr(mask), hip_lib.ptr(out), hip_lib.stream_ptr(k.device)), "dd_attn_aggregate_node_masked")
    return out


def _attention_pos(q, k, v, rel_x, e_w, seg: torch.Tensor, dim_size: int, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    ew = _ew32(e_w)
    qf, kf, vf, rf = _f32(q), _f32(k), _f32(v), _f32(rel_x)                          # (alive past the launch, see above)
    ext = torch_ext()
    if ext is not None:
        return ext.attn_aggregate_pos(qf, kf, vf, ew, rf, seg, mask)
    out = torch.empty(dim_size, 3, device=k.device)
    hip_lib.check(hip_lib.load().dd_attn_aggregate_pos_masked(
        hip_lib.ptr(qf), hip_lib.ptr(kf), hip_lib.ptr(vf), hip_lib.ptr(ew), hip_lib.ptr(rf), hip_lib.ptr(seg), dim_size,
        hip_lib.ptr(mask), hip_lib.ptr(out), hip_lib.stream_ptr(k.device)), "dd_attn_aggregate_pos_masked")
    return out


def _attention_node_bwd(q, k, v, e_w, seg: torch.Tensor, dim_size: int, out, g, mask: Optional[torch.Tensor] = None):
    """(dq, dk, dv, d_ew or None) of `_attention_node`, each in its input's shape and dtype (dd_attn_aggregate_node_bwd_masked;
    mask None = NULL: all members are real)."""
    E, dev = k.size(0), k.device
    per_edge = _per_edge(q, E, dim_size)
    qf, kf, vf, ew, of, gf = _f32(q), _f32(k), _f32(v), _ew32(e_w), _f32(out), _f32(g)
    if qf.shape != ((E if per_edge else dim_size), 128) or kf.shape != (E, 128) or vf.shape != (E, 128) or \
            of.shape != (dim_size, 128) or gf.shape != (dim_size, 128) or (ew is not None and ew.numel() != E) or seg.numel() != dim_size + 1:
        raise ValueError("scatter_attention backward: shapes of q / k / v / e_w / out / grad disagree")
    dq, dk, dv = torch.empty_like(qf), torch.empty_like(kf), torch.empty_like(vf)
    d_ew = None if ew is None else torch.empty_like(ew)
    hip_lib.check(hip_lib.load().dd_attn_aggregate_node_bwd_masked(
        hip_lib.ptr(qf), int(per_edge), hip_lib.ptr(kf), hip_lib.ptr(vf), hip_lib.ptr(ew), hip_lib.ptr(seg), dim_size,
        hip_lib.ptr(mask), hip_lib.ptr(of), hip_lib.ptr(gf), hip_lib.ptr(dq), hip_lib.ptr(dk), hip_lib.ptr(dv), hip_lib.ptr(d_ew),
        hip_lib.stream_ptr(dev)), "dd_attn_aggregate_node_bwd_masked")
    return _grad_like(dq, q), _grad_like(dk, k), _grad_like(dv, v), (None if d_ew is None else _grad_like(d_ew, e_w))


def _attention_pos_bwd(q, k, v, rel_x, e_w, seg: torch.Tensor, dim_size: int, g, mask: Optional[torch.Tensor] = None):
    """(dq, dk, dv16, d_rel, d_ew or None) of `_attention_pos` (dd_attn_aggregate_pos_bwd_masked)."""
    E, dev = k.size(0), k.device
    qf, kf, vf, rf, ew, gf = _f32(q), _f32(k), _f32(v), _f32(rel_x), _ew32(e_w), _f32(g)
    if qf.shape != (dim_size, 128) or kf.shape != (E, 128) or vf.shape != (E, 16) or rf.shape != (E, 3) or gf.shape != (dim_size, 3) or \
            (ew is not None and ew.numel() != E) or seg.numel() != dim_size + 1:
        raise ValueError("scatter_attention_pos backward: shapes of q / k / v / rel_x / e_w / grad disagree")
    dq, dk, dv, dr = torch.empty_like(qf), torch.empty_like(kf), torch.empty_like(vf), torch.empty_like(rf)
    d_ew = None if ew is None else torch.empty_like(ew)
    hip_lib.check(hip_lib.load().dd_attn_aggregate_pos_bwd_masked(
        hip_lib.ptr(qf), hip_lib.ptr(kf), hip_lib.ptr(vf), hip_lib.ptr(ew), hip_lib.ptr(rf), hip_lib.ptr(seg), dim_size,
        hip_lib.ptr(mask), hip_lib.ptr(gf), hip_lib.ptr(dq), hip_lib.ptr(dk), hip_lib.ptr(dv), hip_lib.ptr(d_ew), hip_lib.ptr(dr),
        hip_lib.stream_ptr(dev)), "dd_attn_aggregate_pos_bwd_masked")
    return _grad_like(dq, q), _grad_like(dk, k), _grad_like(dv, v), _grad_like(dr, rel_x), (None if d_ew is None else _grad_like(d_ew, e_w))


def _only_needed(ctx, grads):
    return tuple(g if g is not None and need else None for g, need in zip(grads, ctx.needs_input_grad))


class _ScatterAttention(torch.autograd.Function):
    """scatter_attention with the HIP backward; the forward is the no-grad code path (same kernel, same result)."""

    @staticmethod
    def forward(ctx, q, k, v, e_w, seg, dim_size, mask):
        out = _attention_node(q, k, v, e_w, seg, dim_size, mask)
        ctx.save_for_backward(q, k, v, e_w, seg, out, mask)
        ctx.dim_size = dim_size
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        q, k, v, e_w, seg, out, mask = ctx.saved_tensors
        dq, dk, dv, d_ew = _attention_node_bwd(q, k, v, e_w, seg, ctx.dim_size, out, g, mask)
        return _only_needed(ctx, (dq, dk, dv, d_ew, None, None, None))     # (the mask is not differentiable)


class _ScatterAttentionPos(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, rel_x, e_w, seg, dim_size, mask):
        ctx.save_for_backward(q, k, v, rel_x, e_w, seg, mask)
        ctx.dim_size = dim_size
        return _attention_pos(q, k, v, rel_x, e_w, seg, dim_size, mask)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        q, k, v, rel_x, e_w, seg, mask = ctx.saved_tensors
        dq, dk, dv, dr, d_ew = _attention_pos_bwd(q, k, v, rel_x, e_w, seg, ctx.dim_size, g, mask)
        return _only_needed(ctx, (dq, dk, dv, dr, d_ew, None, None, None))


def scatter_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, index, dim_size: int,
                      e_w: Optional[torch.Tensor] = None, member_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``scatter_sum(scatter_softmax((q_e * k / sqrt(8)).sum(-1), index)[..., None] * (v * e_w), index, dim_size)``
    flattened to ``[dim_size,128]`` (16 heads x 8).  ``q`` is ``[dim_size,128]`` (gathered as ``q[index]`` by the
    reference's node / coordinate layers) or per edge ``[E,128]`` (bond layer: rows of a segment are identical).
    ``index``: the sorted destination vector, or its :class:`SegmentPlan` (no device -> host round trip per call).
    Differentiable w.r.t. ``q``, ``k``, ``v`` and ``e_w`` (dd_attn_aggregate_node_bwd; no double backward).
    ``member_mask`` (``[E]`` bool or uint8 on the device of ``k``; padded batches): True / non-zero members are real, the
    others do not exist -- the softmax runs over the real members of a segment only, a segment without one gives a zero row,
    and whatever the masked rows of ``k``, ``v``, ``e_w`` (and of a per-edge ``q``) hold, NaN included, reaches no result;
    their gradients are exactly zero (dd_attn_aggregate_node_masked / _bwd_masked).  Not differentiable itself."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        hip_lib.require_gpu(t, name)
    dim_size = int(dim_size)
    seg = _attn_seg(index, dim_size, k.size(0))
    mask = _member_mask(member_mask, k, "scatter_attention")                       # (None stays None: the unmasked launch)
    if _needs_grad(q, k, v, e_w):
        return _ScatterAttention.apply(q, k, v, e_w, seg, dim_size, mask)
    return _attention_node(q, k, v, e_w, seg, dim_size, mask)


def scatter_attention_pos(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, rel_x: torch.Tensor, index,
                          dim_size: int, e_w: Optional[torch.Tensor] = None, member_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """PosUpdateLayer's aggregation: ``v`` is ``[E,16]`` (one scalar per head), ``rel_x`` ``[E,3]``; returns
    ``scatter_sum(alpha[..., None] * (v * e_w)[..., None] * rel_x[:, None], index).mean(1)`` — ``[dim_size,3]``.
    ``index`` and ``member_mask`` as for :func:`scatter_attention` (a masked member's ``rel_x`` row is not read into any
    result either); differentiable w.r.t. ``q``, ``k``, ``v``, ``rel_x`` and ``e_w``."""
    for name, t in (("q", q), ("k", k), ("v", v), ("rel_x", rel_x)):
        hip_lib.require_gpu(t, name)
    dim_size = int(dim_size)
    seg = _attn_seg(index, dim_size, k.size(0))
    mask = _member_mask(member_mask, k, "scatter_attention_pos")
    if _needs_grad(q, k, v, rel_x, e_w):
        return _ScatterAttentionPos.apply(q, k, v, rel_x, e_w, seg, dim_size, mask)
    return _attention_pos(q, k, v, rel_x, e_w, seg, dim_size, mask)


def scatter_attention_backward(q, k, v, index, dim_size: int, e_w, out, grad_out, member_mask=None):
    """``(dq, dk, dv, d_ew or None)`` of :func:`scatter_attention` given its result ``out`` and the gradient of it
    (``member_mask``: the forward's; masked members get exact zeros)."""
    return _attention_node_bwd(q, k, v, e_w, _attn_seg(index, int(dim_size), k.size(0)), int(dim_size), out, grad_out,
                               _member_mask(member_mask, k, "scatter_attention_backward"))


def scatter_attention_pos_backward(q, k, v, rel_x, index, dim_size: int, e_w, grad_out, member_mask=None):
    """``(dq, dk, dv, d_rel, d_ew or None)`` of :func:`scatter_attention_pos` given the gradient of its result."""
    return _attention_pos_bwd(q, k, v, rel_x, e_w, _attn_seg(index, int(dim_size), k.size(0)), int(dim_size), grad_out,
                              _member_mask(member_mask, k, "scatter_attention_pos_backward"))


# ------------------------------------------------------------------------------------------------------------------
# Plain torch_scatter drop-ins, same signatures as the wheel the reference imports:
#     from torch_scatter import scatter_softmax, scatter_sum, scatter_mean, scatter_min
# over dim 0 with a 1-D index broadcast along it (every call site of the reference: uni_transformer_edge.py:64,68,160,
# 164,205,209; decompdiff.py:25; guidance_funcs.py:52).  Rows need not be sorted: an unsorted index is stable-sorted
# first (torch_scatter accumulates in an unspecified order; here the order is fixed -> deterministic results).
# ------------------------------------------------------------------------------------------------------------------
_OPS = {"sum": 0, "mean": 1, "min": 2, "max": 3}


def _prep_scatter(src: torch.Tensor, index: torch.Tensor, dim: int, dim_size: Optional[int]):
    hip_lib.require_gpu(src, "src")
    if dim not in (0, -src.dim()):
        raise NotImplementedError("decompdiff_amd scatter ops reduce over dim 0 (every call site of the reference does)")
    if index.dim() != 1:
        if index.shape != src.shape:
            raise ValueError("index must be 1-D or have the shape of src")
        flat = index.reshape(index.size(0), -1)
        if not bool((flat == flat[:, :1]).all().item()):
            raise NotImplementedError("index must be constant along the trailing dims (broadcast of a 1-D index)")
        index = flat[:, 0]
    if index.numel() != src.size(0):
        raise ValueError("index and src disagree along dim 0")
    E = src.size(0)
    n = int(dim_size) if dim_size is not None else (int(index.max().item()) + 1 if E else 0)
    if E and (int(index.min().item()) < 0 or int(index.max().item()) >= n):
        raise IndexError("scatter index out of range")
    perm = None
    if E > 1 and bool((index[1:] < index[:-1]).any().item()):
        index, perm = torch.sort(index, stable=True)
    x = src.detach().to(torch.float32).reshape(E, -1)
    x = (x[perm] if perm is not None else x).contiguous()
    ptr = torch.zeros(n + 1, dtype=torch.int32, device=src.device)
    if E:
        ptr[1:] = torch.bincount(index, minlength=n).cumsum(0)
    return x, ptr, n, perm


class SegmentPlan:
    """The checks and the segment pointer of one (index, dim_size) pair, made ONCE (three device -> host round trips and a
    bincount) for callers that scatter over the same index many times -- a training step uses each of its five index
    vectors 12-36 times (decompdiff_amd/training.py).  Pass it as `index` to scatter_sum / scatter_mean / scatter_softmax."""

    def __init__(self, index: torch.Tensor, dim_size: Optional[int] = None, check: bool = True):
        hip_lib.require_gpu(index, "index")
        if index.dim() != 1:
            raise ValueError("SegmentPlan: 1-D index")
        E = index.numel()
        if not check:
            # No device -> host round trip (usable while a stream is being captured): the caller vouches for 0 <= index < dim_size
            # (e.g. the sources of a kNN graph); the index is sorted unconditionally, the segment pointer comes from a search.
            if dim_size is None:
                raise ValueError("SegmentPlan(check=False) needs dim_size")
            n = int(dim_size)
            self.index, self.perm = torch.sort(index, stable=True)
            self.ptr = torch.searchsorted(self.index, torch.arange(n + 1, device=index.device, dtype=index.dtype)).to(torch.int32)
            self.n, self.E = n, E
            self.inv = torch.empty_like(self.perm)
            self.inv[self.perm] = torch.arange(E, device=index.device)
            return
        n = int(dim_size) if dim_size is not None else (int(index.max().item()) + 1 if E else 0)
        if E and (int(index.min().item()) < 0 or int(index.max().item()) >= n):
            raise IndexError("scatter index out of range")
        self.perm = None
        self.index = index
        if E > 1 and bool((index[1:] < index[:-1]).any().item()):
            self.index, self.perm = torch.sort(index, stable=True)
        self.ptr = torch.zeros(n + 1, dtype=torch.int32, device=index.device)
        if E:
            self.ptr[1:] = torch.bincount(self.index, minlength=n).cumsum(0)
        self.n, self.E = n, E
        self.inv = None
        if self.perm is not None:
            self.inv = torch.empty_like(self.perm)
            self.inv[self.perm] = torch.arange(E, device=index.device)


def _prep(src, index, dim, dim_size):
    """(rows [E,F] fp32 contiguous in segment order, ptr, n, perm) from an index vector or a SegmentPlan."""
    if isinstance(index, SegmentPlan):
        hip_lib.require_gpu(src, "src")
        if src.size(0) != index.E or (dim_size is not None and int(dim_size) != index.n):
            raise ValueError("SegmentPlan does not match src / dim_size")
        x = src.detach().to(torch.float32).reshape(index.E, -1)
        x = (x[index.perm] if index.perm is not None else x).contiguous()
        return x, index.ptr, index.n, index.perm
    return _prep_scatter(src, index, dim, dim_size)


def _segment_reduce(src, index, dim, dim_size, op, out=None):
    x, ptr, n, perm = _prep(src, index, dim, dim_size)
    E, F = x.shape
    ext = torch_ext()
    if ext is not None:
        res, arg = ext.segment_reduce(x, ptr, _OPS[op])
        if op not in ("min", "max"):
            arg = None
    else:
        res = torch.empty(n, F, device=src.device)
        arg = torch.empty(n, F, dtype=torch.int64, device=src.device) if op in ("min", "max") else None
    if ext is None and n and F:
        hip_lib.check(hip_lib.load().dd_segment_reduce(hip_lib.ptr(x) if E else None, hip_lib.ptr(ptr), n, F, _OPS[op], E,
                                                       hip_lib.ptr(res), hip_lib.ptr(arg), hip_lib.stream_ptr(src.device)),
                      "dd_segment_reduce")
    if arg is not None and perm is not None:                # row ids of the caller's (unsorted) order
        valid = arg < E
        arg = torch.where(valid, perm[arg.clamp(max=max(E - 1, 0))], arg)
    shape = (n,) + tuple(src.shape[1:])
    res = res.view(shape).to(src.dtype)
    if out is not None:
        if op in ("sum", "mean"):
            raise NotImplementedError("out= (accumulation into a given tensor) is not used by the reference's call sites")
    return res, (arg.view(shape) if arg is not None else None)


def scatter_sum(src: torch.Tensor, index: torch.Tensor, dim: int = -1, out: Optional[torch.Tensor] = None,
                dim_size: Optional[int] = None) -> torch.Tensor:
    """``torch_scatter.scatter_sum`` (= ``scatter_add``) over dim 0."""
    return _segment_reduce(src, index, dim if src.dim() > 1 or dim != -1 else 0, dim_size, "sum", out)[0]


def scatter_mean(src: torch.Tensor, index: torch.Tensor, dim: int = -1, out: Optional[torch.Tensor] = None,
                 dim_size: Optional[int] = None) -> torch.Tensor:
    """``torch_scatter.scatter_mean`` over dim 0 (sum / max(count, 1))."""
    return _segment_reduce(src, index, dim if src.dim() > 1 or dim != -1 else 0, dim_size, "mean", out)[0]


def scatter_min(src: torch.Tensor, index: torch.Tensor, dim: int = -1, out: Optional[torch.Tensor] = None,
                dim_size: Optional[int] = None):
    """``torch_scatter.scatter_min`` over dim 0 -> ``(values, argmin)``; empty destinations hold 0 / ``src.size(0)``."""
    return _segment_reduce(src, index, dim if src.dim() > 1 or dim != -1 else 0, dim_size, "min", out)


def scatter_max(src: torch.Tensor, index: torch.Tensor, dim: int = -1, out: Optional[torch.Tensor] = None,
                dim_size: Optional[int] = None):
    """``torch_scatter.scatter_max`` over dim 0 -> ``(values, argmax)``."""
    return _segment_reduce(src, index, dim if src.dim() > 1 or dim != -1 else 0, dim_size, "max", out)


def scatter_softmax(src: torch.Tensor, index: torch.Tensor, dim: int = -1, dim_size: Optional[int] = None) -> torch.Tensor:
    """``torch_scatter.composite.scatter_softmax`` over dim 0: per destination and trailing element, softmax over the rows
    scattered to it (max-shifted, no eps: torch_scatter >= 2.1)."""
    x, ptr, n, perm = _prep(src, index, dim if src.dim() > 1 or dim != -1 else 0, dim_size)
    E, F = x.shape
    ext = torch_ext()
    res = ext.segment_softmax(x, ptr) if ext is not None else torch.empty_like(x)
    if ext is None and E and F:
        hip_lib.check(hip_lib.load().dd_segment_softmax(hip_lib.ptr(x), hip_lib.ptr(ptr), n, F, hip_lib.ptr(res),
                                                        hip_lib.stream_ptr(src.device)), "dd_segment_softmax")
    if perm is not None:
        if isinstance(index, SegmentPlan):
            inv = index.inv
        else:
            inv = torch.empty_like(perm)
            inv[perm] = torch.arange(E, device=perm.device)
        res = res[inv]
    return res.view(src.shape).to(src.dtype)


# ------------------------------------------------------------------------------------------------------------------
# torch_sparse at its one call site: the k -> j -> i triplet lists of the ligand bond graph,
# BondUpdateLayer.triplets (uni_transformer_edge.py:103-123), and the SparseTensor that method builds them with.  Both sit on
# one primitive of the library, dd_csr_select_*: a CSR built on the device and rows selected from it, with an optional key
# to leave out per selected row.  ctypes only (the compiled extension has no op for it).
# ------------------------------------------------------------------------------------------------------------------
def _csr_select(node: torch.Tensor, key: torch.Tensor, n_rows: int, n_cols: int, sel: torch.Tensor, skip: Optional[torch.Tensor],
                what: str, with_sel: bool = False):
    """``(out_row, out_key, out_entry[, out_sel, out_skip])`` of include/decompdiff_hip.h: dd_csr_select_count, ONE host read
    (the total and the count of ids out of range, together), dd_csr_select_fill.  All arguments int64, contiguous, on one device."""
    lib, dev = hip_lib.load(), node.device
    E, R = node.numel(), sel.numel()
    nbytes = lib.dd_csr_select_scratch_bytes(E, n_rows, n_cols, R)
    if nbytes == 0:
        raise NotImplementedError(f"{what}: sizes at or above 2**31 (the kernels index with int32)")
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    st = hip_lib.stream_ptr(dev)
    hip_lib.check(lib.dd_csr_select_count(hip_lib.ptr(node), hip_lib.ptr(key), E, n_rows, n_cols, hip_lib.ptr(sel), hip_lib.ptr(skip), R,
                                          hip_lib.ptr(scratch), nbytes, st), "dd_csr_select_count")
    total, bad = scratch[:2].tolist()
    if bad:
        raise IndexError(f"{what}: {bad} ids out of range")
    outs = [torch.empty(total, dtype=torch.int64, device=dev) for _ in range(5 if with_sel else 3)]
    hip_lib.check(lib.dd_csr_select_fill(hip_lib.ptr(sel), hip_lib.ptr(skip), E, n_rows, n_cols, R, hip_lib.ptr(scratch), total,
                                         *[hip_lib.ptr(o) for o in outs], *([] if with_sel else [None, None]), st), "dd_csr_select_fill")
    return outs


def triplets(edge_index: torch.Tensor, num_nodes: int):
    """``BondUpdateLayer.triplets``: ``(i, j, idx_i, idx_j, idx_k, idx_kj, idx_ji)`` of the directed graph whose edge ``e`` is
    ``edge_index[0, e] -> edge_index[1, e]`` (j -> i).  For every edge in edge order, the edges ``k -> j`` into its source with
    ``k`` ascending (equal ``(k, j)`` pairs in edge order) and ``k == i`` dropped: ``idx_kj`` is the id of the edge ``k -> j``,
    ``idx_ji`` is ``e`` -- non-decreasing, so it is accepted as the index of :func:`scatter_attention`.  ``i`` and ``j`` are
    ``edge_index[1]`` and ``edge_index[0]`` themselves.  The edge list need not be sorted and nodes without edges are normal
    (``decomp_fc`` / ``scaffold_fc`` bond lists, ligand rows among protein rows).  Node ids outside ``[0, num_nodes)`` raise
    ``IndexError``.  The length of the lists depends on the data: every call reads it back from the device (one device ->
    host copy), so it cannot run while a stream is being captured."""
    if not torch.is_tensor(edge_index) or edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError("triplets: edge_index must be an int64 tensor [2,E]")
    n = int(num_nodes)
    if n < 0:
        raise ValueError("triplets: num_nodes < 0")
    hip_lib.require_gpu(edge_index, "edge_index")
    j, i = edge_index[0], edge_index[1]
    if edge_index.size(1) == 0 or n == 0:
        if edge_index.size(1):
            raise IndexError("triplets: edges of a graph without nodes")
        return (i, j) + tuple(torch.empty(0, dtype=torch.int64, device=edge_index.device) for _ in range(5))
    row, col = j.contiguous(), i.contiguous()
    idx_ji, idx_k, idx_kj, idx_j, idx_i = _csr_select(col, row, n, n, row, col, "triplets", with_sel=True)
    return i, j, idx_i, idx_j, idx_k, idx_kj, idx_ji


class _SparseStorage:
    def __init__(self, row, col, value):
        self._row, self._col, self._value = row, col, value

    def row(self):
        return self._row

    def col(self):
        return self._col

    def value(self):
        return self._value


class SparseTensor:
    """``torch_sparse.SparseTensor`` as far as ``BondUpdateLayer.triplets`` touches it (uni_transformer_edge.py:108-122), on
    device tensors: the constructor with ``row=``, ``col=``, ``value=``, ``sparse_sizes=`` (entries kept sorted by (row, col),
    stable), ``t[index]`` with an int64 index tensor (new row ``r`` is old row ``index[r]``; repeats and empty rows allowed),
    ``set_value(None)``, ``sum(dim=1)`` of a value-less tensor (entries per row, float), ``storage.row() / col() / value()`` and
    ``sparse_sizes()``.  Anything else raises ``NotImplementedError``.  The constructor and ``t[index]`` each run the
    dd_csr_select kernels and read one pair of counters back from the device."""

    def __init__(self, row: Optional[torch.Tensor] = None, col: Optional[torch.Tensor] = None, value: Optional[torch.Tensor] = None,
                 sparse_sizes=None, **kwargs):
        if kwargs or row is None or col is None or sparse_sizes is None:
            raise NotImplementedError("SparseTensor: construct with row=, col=, value=, sparse_sizes= (" + ", ".join(kwargs) + ")")
        if row.dtype != torch.int64 or col.dtype != torch.int64 or row.dim() != 1 or col.shape != row.shape:
            raise ValueError("SparseTensor: row and col must be int64 vectors of one length")
        hip_lib.require_gpu(row, "row")
        hip_lib.require_gpu(col, "col")
        if value is not None and (value.size(0) != row.numel() or value.device != row.device):
            raise ValueError("SparseTensor: value must have one entry per row / col entry, on their device")
        self._sizes = (int(sparse_sizes[0]), int(sparse_sizes[1]))
        if row.numel() == 0:
            self.storage = _SparseStorage(row, col, value)
            return
        every_row = torch.arange(self._sizes[0], device=row.device)
        srow, scol, perm = _csr_select(row.contiguous(), col.contiguous(), self._sizes[0], self._sizes[1], every_row, None, "SparseTensor")
        self.storage = _SparseStorage(srow, scol, None if value is None else value[perm])

    @classmethod
    def _sorted(cls, row, col, value, sizes):
        t = cls.__new__(cls)
        t.storage, t._sizes = _SparseStorage(row, col, value), sizes
        return t

    def sparse_sizes(self):
        return self._sizes

    def __getitem__(self, index):
        if not torch.is_tensor(index) or index.dtype != torch.int64 or index.dim() != 1:
            raise NotImplementedError("SparseTensor.__getitem__: an int64 index vector selecting rows")
        row, col, value = self.storage.row(), self.storage.col(), self.storage.value()
        hip_lib.require_gpu(index, "index")
        sizes = (index.numel(), self._sizes[1])
        if index.numel() == 0 or self._sizes[0] == 0:
            if index.numel():
                raise IndexError("SparseTensor.__getitem__: rows of a tensor without rows")
            return SparseTensor._sorted(row[:0], col[:0], None if value is None else value[:0], sizes)
        nrow, ncol, entry = _csr_select(row, col, self._sizes[0], self._sizes[1], index.contiguous(), None, "SparseTensor.__getitem__")
        return SparseTensor._sorted(nrow, ncol, None if value is None else value[entry], sizes)

    def set_value(self, value, layout=None):
        if value is not None:
            raise NotImplementedError("SparseTensor.set_value: only set_value(None)")
        return SparseTensor._sorted(self.storage.row(), self.storage.col(), None, self._sizes)

    def sum(self, dim=None):
        if dim != 1 or self.storage.value() is not None:
            raise NotImplementedError("SparseTensor.sum: only sum(dim=1) of a tensor without values")
        return torch.bincount(self.storage.row(), minlength=self._sizes[0]).to(torch.float32)

    def __getattr__(self, name):
        if name.startswith("__") or name in ("storage", "_sizes"):      # (Python's own protocol lookups; a half-built object)
            raise AttributeError(name)
        raise NotImplementedError(f"SparseTensor.{name}: not part of the decompdiff_amd drop-in")
