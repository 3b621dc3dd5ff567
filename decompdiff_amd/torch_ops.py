"""Torch-level registration of the op-level boundary (BASELINE.json north_star: "exposed as torch
extensions"): every drop-in of :mod:`decompdiff_amd.functional` becomes a dispatcher op ``torch.ops.decompdiff_amd.*``
(``torch.library.custom_op``, device type "cuda" = HIP on ROCm), with shape-propagating fake implementations so the ops
trace under ``torch.compile`` / ``make_fx``.  The kernels stay behind the C ABI (ctypes, no torch headers in the library);
there is no CPU implementation — CPU tensors raise.

    import decompdiff_amd.torch_ops                         # registers the ops
    edge_index = torch.ops.decompdiff_amd.knn_graph(x, 32, batch)
    alpha = torch.ops.decompdiff_amd.scatter_softmax(score, dst, 0, n)

:func:`patch_reference_imports` installs module objects named ``torch_scatter`` and ``torch_cluster`` exposing these ops
under the names the reference imports (``from torch_scatter import scatter_softmax, scatter_sum``:
models/encoders/uni_transformer_edge.py:9; ``scatter_mean``: models/decompdiff.py:9; ``scatter_min``:
utils/guidance_funcs.py:9), and -- where the real package is not importable -- a ``torch_sparse`` module holding
:class:`decompdiff_amd.functional.SparseTensor` (``from torch_sparse import SparseTensor``:
models/encoders/uni_transformer_edge.py:13), for hosts that keep the reference's Python layers.
"""
from __future__ import annotations

import importlib
import sys
import types
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import functional as F

_NS = "decompdiff_amd"


@torch.library.custom_op(f"{_NS}::knn_graph", mutates_args=(), device_types="cuda")
def knn_graph(x: Tensor, k: int, batch: Optional[Tensor] = None, loop: bool = False, flow: str = "source_to_target") -> Tensor:
    return F.knn_graph(x, k, batch, loop, flow)


@knn_graph.register_fake
def _(x, k, batch=None, loop=False, flow="source_to_target"):
    ctx = torch.library.get_ctx()
    return x.new_empty((2, ctx.new_dynamic_size()), dtype=torch.long)


# The five triplet lists (idx_i, idx_j, idx_k, idx_kj, idx_ji) of functional.triplets; its first two results are rows of
# edge_index itself, which an op may not return (outputs must not alias inputs).  Integer outputs: no autograd formula.
@torch.library.custom_op(f"{_NS}::triplets", mutates_args=(), device_types="cuda")
def triplets(edge_index: Tensor, num_nodes: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    return F.triplets(edge_index, num_nodes)[2:]


@triplets.register_fake
def _(edge_index, num_nodes):
    n = torch.library.get_ctx().new_dynamic_size()
    return tuple(edge_index.new_empty((n,), dtype=torch.long) for _ in range(5))


@torch.library.custom_op(f"{_NS}::scatter_attention", mutates_args=(), device_types="cuda")
def scatter_attention(q: Tensor, k: Tensor, v: Tensor, index: Tensor, dim_size: int, e_w: Optional[Tensor] = None,
                      member_mask: Optional[Tensor] = None) -> Tensor:
    with torch.no_grad():                                   # (the autograd formula is registered below)
        return F.scatter_attention(q, k, v, index, dim_size, e_w, member_mask)


@scatter_attention.register_fake
def _(q, k, v, index, dim_size, e_w=None, member_mask=None):
    return k.new_empty((dim_size, 128), dtype=torch.float32)


@torch.library.custom_op(f"{_NS}::scatter_attention_pos", mutates_args=(), device_types="cuda")
def scatter_attention_pos(q: Tensor, k: Tensor, v: Tensor, rel_x: Tensor, index: Tensor, dim_size: int,
                          e_w: Optional[Tensor] = None, member_mask: Optional[Tensor] = None) -> Tensor:
    with torch.no_grad():
        return F.scatter_attention_pos(q, k, v, rel_x, index, dim_size, e_w, member_mask)


@scatter_attention_pos.register_fake
def _(q, k, v, rel_x, index, dim_size, e_w=None, member_mask=None):
    return k.new_empty((dim_size, 3), dtype=torch.float32)


# The backward passes of the two attention ops are ops themselves (dd_attn_aggregate_node_bwd / _pos_bwd behind them), so a
# traced backward graph holds them as single nodes.  An absent e_w comes back as an empty tensor (an op cannot return None).
@torch.library.custom_op(f"{_NS}::scatter_attention_backward", mutates_args=(), device_types="cuda")
def scatter_attention_backward(q: Tensor, k: Tensor, v: Tensor, index: Tensor, dim_size: int, e_w: Optional[Tensor], out: Tensor,
                               grad_out: Tensor, member_mask: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    dq, dk, dv, d_ew = F.scatter_attention_backward(q, k, v, index, dim_size, e_w, out, grad_out, member_mask)
    return dq, dk, dv, (d_ew if d_ew is not None else k.new_empty(0))


@scatter_attention_backward.register_fake
def _(q, k, v, index, dim_size, e_w, out, grad_out, member_mask=None):
    return torch.empty_like(q), torch.empty_like(k), torch.empty_like(v), (torch.empty_like(e_w) if e_w is not None else k.new_empty(0))


@torch.library.custom_op(f"{_NS}::scatter_attention_pos_backward", mutates_args=(), device_types="cuda")
def scatter_attention_pos_backward(q: Tensor, k: Tensor, v: Tensor, rel_x: Tensor, index: Tensor, dim_size: int, e_w: Optional[Tensor],
                                   grad_out: Tensor, member_mask: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    dq, dk, dv, dr, d_ew = F.scatter_attention_pos_backward(q, k, v, rel_x, index, dim_size, e_w, grad_out, member_mask)
    return dq, dk, dv, dr, (d_ew if d_ew is not None else k.new_empty(0))


@scatter_attention_pos_backward.register_fake
def _(q, k, v, rel_x, index, dim_size, e_w, grad_out, member_mask=None):
    return (torch.empty_like(q), torch.empty_like(k), torch.empty_like(v), torch.empty_like(rel_x),
            (torch.empty_like(e_w) if e_w is not None else k.new_empty(0)))


def _n_out(index, dim_size):
    return dim_size if dim_size is not None else torch.library.get_ctx().new_dynamic_size()


@torch.library.custom_op(f"{_NS}::scatter_sum", mutates_args=(), device_types="cuda")
def scatter_sum(src: Tensor, index: Tensor, dim: int = -1, dim_size: Optional[int] = None) -> Tensor:
    return F.scatter_sum(src, index, dim, None, dim_size)


@scatter_sum.register_fake
def _(src, index, dim=-1, dim_size=None):
    return src.new_empty((_n_out(index, dim_size),) + tuple(src.shape[1:]))


@torch.library.custom_op(f"{_NS}::scatter_mean", mutates_args=(), device_types="cuda")
def scatter_mean(src: Tensor, index: Tensor, dim: int = -1, dim_size: Optional[int] = None) -> Tensor:
    return F.scatter_mean(src, index, dim, None, dim_size)


@scatter_mean.register_fake
def _(src, index, dim=-1, dim_size=None):
    return src.new_empty((_n_out(index, dim_size),) + tuple(src.shape[1:]))


@torch.library.custom_op(f"{_NS}::scatter_min", mutates_args=(), device_types="cuda")
def scatter_min(src: Tensor, index: Tensor, dim: int = -1, dim_size: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    return F.scatter_min(src, index, dim, None, dim_size)


@scatter_min.register_fake
def _(src, index, dim=-1, dim_size=None):
    shape = (_n_out(index, dim_size),) + tuple(src.shape[1:])
    return src.new_empty(shape), src.new_empty(shape, dtype=torch.long)


@torch.library.custom_op(f"{_NS}::scatter_softmax", mutates_args=(), device_types="cuda")
def scatter_softmax(src: Tensor, index: Tensor, dim: int = -1, dim_size: Optional[int] = None) -> Tensor:
    return F.scatter_softmax(src, index, dim, dim_size)


@scatter_softmax.register_fake
def _(src, index, dim=-1, dim_size=None):
    return torch.empty_like(src)


# ------------------------------------------------------------------------------------------------------------------
# Autograd formulas (the reference differentiates through these ops: drift guidance calls torch.autograd.grad through
# scatter_min, utils/guidance_funcs.py:52-60; training goes through scatter_softmax / scatter_sum / scatter_mean).
# Backward passes reuse the registered ops (so they run on the HIP kernels too); the index is never differentiated.
# ------------------------------------------------------------------------------------------------------------------
def _index_1d(index):
    return index if index.dim() == 1 else index.reshape(index.size(0), -1)[:, 0]


def _setup_sum(ctx, inputs, output):
    src, index, dim, dim_size = inputs
    ctx.save_for_backward(_index_1d(index))


def _bw_sum(ctx, g):
    (index,) = ctx.saved_tensors
    return g.index_select(0, index), None, None, None


scatter_sum.register_autograd(_bw_sum, setup_context=_setup_sum)


def _setup_mean(ctx, inputs, output):
    src, index, dim, dim_size = inputs
    idx = _index_1d(index)
    ctx.save_for_backward(idx, torch.bincount(idx, minlength=output.size(0)).clamp(min=1))


def _bw_mean(ctx, g):
    index, cnt = ctx.saved_tensors
    scale = (1.0 / cnt.to(g.dtype)).view((-1,) + (1,) * (g.dim() - 1))
    return (g * scale).index_select(0, index), None, None, None


scatter_mean.register_autograd(_bw_mean, setup_context=_setup_mean)


def _setup_softmax(ctx, inputs, output):
    src, index, dim, dim_size = inputs
    idx = _index_1d(index)
    ctx.save_for_backward(output, idx)
    ctx.n_seg = int(dim_size) if dim_size is not None else (int(idx.max().item()) + 1 if idx.numel() else 0)


def _bw_softmax(ctx, g):
    y, index = ctx.saved_tensors
    yg = y * g
    tot = torch.ops.decompdiff_amd.scatter_sum(yg.contiguous(), index, 0, ctx.n_seg)
    return yg - y * tot.index_select(0, index), None, None, None


scatter_softmax.register_autograd(_bw_softmax, setup_context=_setup_softmax)


def _setup_attention(ctx, inputs, output):
    q, k, v, index, dim_size, e_w, member_mask = inputs
    ctx.save_for_backward(q, k, v, index, e_w, output, member_mask)
    ctx.dim_size = dim_size


def _bw_attention(ctx, g):
    q, k, v, index, e_w, out, member_mask = ctx.saved_tensors
    dq, dk, dv, d_ew = torch.ops.decompdiff_amd.scatter_attention_backward(q, k, v, index, ctx.dim_size, e_w, out, g.contiguous(),
                                                                           member_mask)
    need = ctx.needs_input_grad
    return (dq if need[0] else None, dk if need[1] else None, dv if need[2] else None, None, None,
            d_ew if e_w is not None and need[5] else None, None)


scatter_attention.register_autograd(_bw_attention, setup_context=_setup_attention)


def _setup_attention_pos(ctx, inputs, output):
    q, k, v, rel_x, index, dim_size, e_w, member_mask = inputs
    ctx.save_for_backward(q, k, v, rel_x, index, e_w, member_mask)
    ctx.dim_size = dim_size


def _bw_attention_pos(ctx, g):
    q, k, v, rel_x, index, e_w, member_mask = ctx.saved_tensors
    dq, dk, dv, dr, d_ew = torch.ops.decompdiff_amd.scatter_attention_pos_backward(q, k, v, rel_x, index, ctx.dim_size, e_w, g.contiguous(),
                                                                                   member_mask)
    need = ctx.needs_input_grad
    return (dq if need[0] else None, dk if need[1] else None, dv if need[2] else None, dr if need[3] else None, None, None,
            d_ew if e_w is not None and need[6] else None, None)


scatter_attention_pos.register_autograd(_bw_attention_pos, setup_context=_setup_attention_pos)


def _setup_min(ctx, inputs, output):
    src, index, dim, dim_size = inputs
    ctx.save_for_backward(output[1])
    ctx.src_shape = tuple(src.shape)


def _bw_min(ctx, g_val, g_arg):
    (arg,) = ctx.saved_tensors
    E = ctx.src_shape[0]
    a = arg.reshape(arg.size(0), -1)
    g = g_val.reshape(arg.size(0), -1)
    valid = a < E                                                        # empty destinations point at row E
    grad = torch.zeros((E + 1, a.size(1)), dtype=g.dtype, device=g.device)
    grad.scatter_add_(0, torch.where(valid, a, torch.full_like(a, E)), g * valid.to(g.dtype))
    return grad[:E].reshape(ctx.src_shape), None, None, None


scatter_min.register_autograd(_bw_min, setup_context=_setup_min)


def patch_reference_imports(force: bool = False) -> None:
    """Make ``import torch_scatter`` / ``from torch_geometric.nn import knn_graph``-style imports of a host that keeps the
    reference's Python resolve to these ops.  Existing real packages are left alone unless ``force``.  ``torch_sparse`` is
    installed (one name, ``SparseTensor``: functional.SparseTensor) when the real package cannot be imported, or with ``force``."""
    ops = torch.ops.decompdiff_amd

    def _with_out(op):
        def f(src, index, dim=-1, out=None, dim_size=None):
            if out is not None:
                raise NotImplementedError("out= is not used by the reference's call sites")
            return op(src, index, dim, dim_size)
        return f
    if force or "torch_scatter" not in sys.modules:
        m = types.ModuleType("torch_scatter")
        m.scatter_sum = m.scatter_add = _with_out(ops.scatter_sum)
        m.scatter_mean = _with_out(ops.scatter_mean)
        m.scatter_min = _with_out(ops.scatter_min)
        m.scatter_softmax = lambda src, index, dim=-1, dim_size=None: ops.scatter_softmax(src, index, dim, dim_size)
        m.__doc__ = "decompdiff_amd drop-ins (HIP, gfx950) for the torch_scatter functions the reference imports"
        sys.modules["torch_scatter"] = m
    if force or "torch_cluster" not in sys.modules:
        c = types.ModuleType("torch_cluster")
        c.knn_graph = lambda x, k, batch=None, loop=False, flow="source_to_target", **kw: ops.knn_graph(x, k, batch, loop, flow)
        sys.modules["torch_cluster"] = c
    if force or not _importable("torch_sparse"):
        t = types.ModuleType("torch_sparse")
        t.SparseTensor = F.SparseTensor
        t.__doc__ = "decompdiff_amd drop-in (HIP, gfx950) for the SparseTensor the reference's BondUpdateLayer.triplets builds"
        sys.modules["torch_sparse"] = t


def _importable(name: str) -> bool:
    if name in sys.modules:
        return True
    try:
        importlib.import_module(name)
    except (ImportError, OSError):                            # absent, or a wheel built against another runtime
        return False
    return True
