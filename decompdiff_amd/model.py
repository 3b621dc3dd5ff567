"""Host-side mirror of the reference's model API for the sampling hot path.

:class:`DecompScorePosNet3D` keeps the constructor, ``forward`` and ``sample_diffusion``
signatures, the attribute surface read by scripts/sample_diffusion_decomp.py
(``num_classes``, ``num_bond_classes``, ``bond_diffusion``, ``num_timesteps``) and the complete
``state_dict`` key layout of /root/reference/models/decompdiff.py:75-703, so a reference
checkpoint loads with ``strict=True`` and the reference's sampling script can call it unchanged.
All arithmetic of the loop runs in libdecompdiff_hip.so (HIP, gfx950); this file only converts
the PyG-style flat batch into the dense fixed-shape layout, owns device buffers and unpacks
results.  Nothing here computes the network on the CPU — CPU tensors raise.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
import os
import time
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from . import batch_layout as BL, hip_lib, packing, schedules
from .synth import learnable_param_shapes

H = 128


class _Node(nn.Module):
    """Anonymous container used to reproduce the reference's dotted state_dict keys."""


def _attach(root: nn.Module, dotted: str, tensor: torch.Tensor, kind: str):
    parts = dotted.split(".")
    mod = root
    for p in parts[:-1]:
        if p not in mod._modules:
            mod.add_module(p, _Node())
        mod = mod._modules[p]
    if kind == "param":
        mod.register_parameter(parts[-1], nn.Parameter(tensor, requires_grad=True))
    elif kind == "const":                       # to_torch_const(): nn.Parameter(requires_grad=False)
        mod.register_parameter(parts[-1], nn.Parameter(tensor, requires_grad=False))
    else:
        mod.register_buffer(parts[-1], tensor)


BOND_NET_TYPES = ("lin", "pre_att")     # bond head on the last h_bond / on the final distances and atom features

GAUSS_OFFSETS = [0, 1, 1.25, 1.5, 1.75, 2, 2.25, 2.5, 2.75, 3, 3.5, 4, 4.5, 5, 5.5, 6, 7, 8, 9, 10]


def _check_queue(sampler, dev):
    """Measurement build only.  Its tile-queue schedule (dd_debug_set_option(8, 5); EXPERIMENTS.md R3-1) hands data from the
    layer-tail GEMM queue to the attention launches through device counters with bounded polls; a poll that gave up means
    the results are invalid: raise.  The default library's schedule uses graph edges only and never polls, so for it this
    is a no-op (no device -> host copy, no stream synchronisation)."""
    if not hip_lib.is_measurement_build():
        return
    code = ctypes.c_int(0)
    hip_lib.check(hip_lib.load().dd_queue_error(ctypes.byref(sampler), hip_lib.stream_ptr(dev), ctypes.byref(code)), "dd_queue_error")
    if code.value != 0:
        raise RuntimeError(f"decompdiff_hip (measurement build): an in-launch hand-off of the tile-queue schedule timed out "
                           f"(waiter {code.value}); the results are invalid (dd_debug_set_option(8, 4) selects the shipped "
                           "graph-edge schedule)")


def log_sample_categorical(logits: torch.Tensor) -> torch.Tensor:
    """Gumbel-argmax sampling, re-exported because the reference's script imports it from
    models.decompdiff (scripts/sample_diffusion_decomp.py:25; models/transitions.py:78-84).
    Used by the harness for the *initial* types only (outside the hot loop)."""
    uniform = torch.rand_like(logits)
    gumbel = -torch.log(-torch.log(uniform + 1e-30) + 1e-30)
    return (gumbel + logits).argmax(dim=-1)


def sample_keys(seed: int, indices) -> torch.Tensor:
    """Per-sample noise keys for ``sample_diffusion(sample_keys=...)``: one 64-bit key per global sample index, as an int64 CPU
    tensor of the shape of ``indices`` (an int, a sequence of ints or an integer tensor; the key's 64 bits, two's complement).

    The function, exactly (all arithmetic on unsigned 64-bit integers, wrapping modulo 2**64)::

        z   = seed + 0x9E3779B97F4A7C15 * (index + 1)
        z   = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
        z   = (z ^ (z >> 27)) * 0x94D049BB133111EB
        key = z ^ (z >> 31)

    i.e. output number ``index`` (from 0) of a splitmix64 generator whose state starts at ``seed``.  A job that gives its sample
    ``g`` the key ``sample_keys(seed, g)`` gets the same chain for that sample under any batch size, sharding or order."""
    idx = np.asarray(indices.cpu() if torch.is_tensor(indices) else indices)
    if idx.size and (idx.dtype.kind not in "iu" or int(idx.min()) < 0):
        raise ValueError("indices must be non-negative integers")
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) + np.uint64(0x9E3779B97F4A7C15) * (idx.astype(np.uint64) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return torch.from_numpy(np.asarray(z, dtype=np.uint64).astype(np.int64).reshape(idx.shape))


def _as_sample_keys(keys, batch_ligand) -> torch.Tensor:
    """``sample_keys`` of sample_diffusion as an int64 tensor [B] holding the keys' 64 bits: a length-B int64 tensor as it is, a
    sequence of ints in [0, 2**64) wrapped to two's complement; one key per sample of ``batch_ligand``."""
    if torch.is_tensor(keys):
        if keys.dtype != torch.int64 or keys.dim() != 1:
            raise ValueError("sample_keys must be a one-dimensional int64 tensor or a sequence of ints")
        out = keys.detach()
    else:
        vals = [int(k) for k in keys]
        if any(not 0 <= k < 2 ** 64 for k in vals):
            raise ValueError("sample_keys must lie in [0, 2**64)")
        out = torch.tensor([k - 2 ** 64 if k >= 2 ** 63 else k for k in vals], dtype=torch.int64)
    B = int(batch_ligand.max().item()) + 1 if batch_ligand.numel() else 0
    if out.numel() != B:
        raise ValueError(f"sample_keys must hold one key per sample ({B}), got {out.numel()}")
    return out


def _check_ligand_atom_mask(mask, n_ligand):
    """``ligand_atom_mask`` of forward / sample_diffusion (decompdiff.py:217,560).  The reference's script always passes
    None (scripts/sample_diffusion_decomp.py:340).  An all-True boolean mask is equivalent to None in the reference
    (probed: identical results); any mask with a False / 0 entry makes the reference itself fail -- its forward returns
    predictions for the selected atoms only (`final_pos[mask_ligand_atom]`, decompdiff.py:321) and the loop then combines
    them with the full x_t (:611: "The size of tensor a must match the size of tensor b") -- so the same RuntimeError is
    raised here instead of inventing semantics."""
    if mask is None:
        return
    mask = torch.as_tensor(mask)
    if mask.numel() != n_ligand:
        raise ValueError("ligand_atom_mask must have one entry per ligand atom")
    if mask.dtype == torch.bool and bool(mask.all().item()):
        return
    raise RuntimeError("ligand_atom_mask with masked-out (or non-boolean) entries: the reference's sampling loop fails on "
                       "such a mask (size mismatch between the masked predictions and x_t, decompdiff.py:321,611); only "
                       "None or an all-True boolean mask is meaningful")


FIXED_MODES = ("hold", "replace")


def _as_fixed(fixed, n_ligand, fc_index, bond_type, num_classes, num_bond_classes, noise, start_step, prior_centers,
              ligand_decomp_batch, ligand_atom_mask, dev, need_cc=False):
    """``fixed`` of sample_diffusion, validated (ValueError) and moved to the device: dict(mode, init, mask bool [n], pos f32 [n,3],
    v int32 [n], bond int32 [n_bond], cc f32 [n,3] or None -- the prior centre of every atom's arm, replace mode and, with
    ``need_cc`` (resampling: a jump noises around the centres), hold mode)."""
    if not isinstance(fixed, dict):
        raise ValueError("fixed must be None or a dict(mask, pos, v, bond, mode[, init])")
    unknown = set(fixed) - {"mask", "pos", "v", "bond", "mode", "init"}
    if unknown or any(k not in fixed for k in ("mask", "pos", "v", "bond")):
        raise ValueError(f"fixed takes the keys mask, pos, v, bond, mode and init (got {sorted(fixed)})")
    mode = fixed.get("mode", "hold")
    if mode not in FIXED_MODES:
        raise ValueError(f"fixed['mode'] must be one of {FIXED_MODES}, got {mode!r}")
    if ligand_atom_mask is not None:
        m = torch.as_tensor(ligand_atom_mask)
        if not (m.dtype == torch.bool and m.numel() == n_ligand and bool(m.all().item())):
            raise ValueError("fixed excludes a ligand_atom_mask that masks atoms out: the held atoms are given by fixed['mask']")
    mask, pos, v, bond = (torch.as_tensor(fixed[k]) for k in ("mask", "pos", "v", "bond"))
    if mask.dtype != torch.bool:
        raise ValueError(f"fixed['mask'] must be a bool tensor, got {mask.dtype}")
    if fc_index is None or bond_type is None:
        raise NotImplementedError("the uni_o2_bond path needs the fully connected ligand bond graph")
    n_bond = int(bond_type.numel())
    for name, t, shape in (("mask", mask, (n_ligand,)), ("pos", pos, (n_ligand, 3)), ("v", v, (n_ligand,)), ("bond", bond, (n_bond,))):
        if tuple(t.shape) != shape:
            raise ValueError(f"fixed['{name}'] must have shape {shape}, got {tuple(t.shape)}")
    if v.dtype.is_floating_point or bond.dtype.is_floating_point or v.dtype == torch.bool or bond.dtype == torch.bool:
        raise ValueError("fixed['v'] and fixed['bond'] must be integer class ids")
    mask_c, v_c, bond_c = mask.cpu(), v.cpu().long(), bond.cpu().long()
    fc = fc_index.cpu()
    held_b = mask_c[fc[0]] & mask_c[fc[1]]                   # a bond is held iff both its endpoints are
    hv, hb = v_c[mask_c], bond_c[held_b]
    if hv.numel() and (int(hv.min()) < 0 or int(hv.max()) >= num_classes):
        raise ValueError(f"fixed['v'] holds a class outside [0, {num_classes}) at a held atom")
    if hb.numel() and (int(hb.min()) < 0 or int(hb.max()) >= num_bond_classes):
        raise ValueError(f"fixed['bond'] holds a class outside [0, {num_bond_classes}) at a held bond")
    init, cc = None, None
    if mode == "replace":
        need_given = noise is not None or int(start_step) > 0
        init = fixed.get("init", None if need_given else "draw")
        if init not in ("draw", "given"):
            raise ValueError("fixed['init'] must be 'draw' or 'given'" + (
                " ('given' is required with noise= and with start_step > 0: the held rows of init_ligand_* are the state)"
                if init is None else f", got {init!r}"))
        if need_given and init != "given":
            raise ValueError("fixed['init'] = 'draw' needs the device generator and start_step == 0; with noise= or start_step > 0 "
                             "pass init='given' and the held rows' state in init_ligand_*")
    elif "init" in fixed and fixed["init"] not in (None, "draw", "given"):
        raise ValueError(f"fixed['init'] must be 'draw' or 'given', got {fixed['init']!r}")
    if mode == "replace" or need_cc:
        if prior_centers is None or ligand_decomp_batch is None or not torch.is_tensor(prior_centers) or prior_centers.dim() != 2 \
                or prior_centers.shape[1] != 3 or ligand_decomp_batch.numel() != n_ligand \
                or (ligand_decomp_batch.numel() and int(ligand_decomp_batch.max()) >= prior_centers.shape[0]):
            raise ValueError("fixed mode 'replace' (and resample in either mode) needs prior_centers [n_prior,3] and "
                             "ligand_decomp_batch [n_ligand]: the forward process noises around the arm centres")
        cc = prior_centers.detach().to(device=dev, dtype=torch.float32)[ligand_decomp_batch.to(dev)].contiguous()
    # classes at free rows are never read: zero them so that the int32 copies stay in range whatever the caller left there
    v_c = torch.where(mask_c, v_c, torch.zeros_like(v_c))
    bond_c = torch.where(held_b, bond_c, torch.zeros_like(bond_c))
    return dict(mode=mode, init=init, mask=mask_c.to(dev), pos=pos.detach().to(device=dev, dtype=torch.float32).contiguous(),
                v=v_c.to(device=dev, dtype=torch.int32), bond=bond_c.to(device=dev, dtype=torch.int32), cc=cc)


INIT_MODES = ("prior", "noised")


def _as_init(init, batch_ligand, fc_index, ligand_decomp_batch, prior_centers, prior_stds, given, noise, start_step, num_timesteps,
             num_classes, num_bond_classes, dev):
    """``init`` of sample_diffusion, validated (ValueError) and moved to the device: dict(mode, cen f32 [n,3] -- the centre of
    every atom, uncentred --, std f32 [n,3], atom_lp f32 [num_classes] or None, bond_lp f32 [num_bond_classes] or None and,
    mode "noised", pos f32 [n,3], v int32 [n], bond int32 [n_bond]).  ``given``: the caller's init_ligand_pos / _v / _fc_bond_type."""
    if not isinstance(init, dict) or init.get("mode") not in INIT_MODES:
        raise ValueError(f"init must be None or a dict with mode in {INIT_MODES}")
    mode = init["mode"]
    allowed = {"mode", "centers", "stds", "atom_prior", "bond_prior"} | ({"pos", "v", "bond"} if mode == "noised" else set())
    if set(init) - allowed or (mode == "noised" and any(k not in init for k in ("pos", "v", "bond"))):
        raise ValueError(f"init mode {mode!r} takes the keys {sorted(allowed)} (got {sorted(init)})")
    if any(t is not None for t in given):
        raise ValueError("init draws the chain's first state on the device: init_ligand_pos, init_ligand_v and "
                         "init_ligand_fc_bond_type must be None")
    if noise is not None:
        raise ValueError("init excludes noise=: the first state is drawn by the device generator")
    if mode == "prior" and int(start_step) != 0:
        raise ValueError("init mode 'prior' draws the level above the first step: it needs start_step == 0")
    if mode == "noised" and not 0 <= int(start_step) < num_timesteps:
        raise ValueError("init mode 'noised' needs 0 <= start_step < num_timesteps (the level num_timesteps - 1 - start_step)")
    if fc_index is None:
        raise NotImplementedError("the uni_o2_bond path needs the fully connected ligand bond graph")
    n, n_bond = int(batch_ligand.numel()), int(fc_index.shape[1])
    if ligand_decomp_batch is None or ligand_decomp_batch.numel() != n or (n and int(ligand_decomp_batch.min()) < 0):
        raise ValueError("init needs ligand_decomp_batch [n_ligand]: the centre and std of every atom")
    n_prior = int(ligand_decomp_batch.max()) + 1 if n else 0
    per_atom = {}
    for name, t, what in (("centers", init.get("centers"), prior_centers), ("stds", init.get("stds"), prior_stds)):
        t = what if t is None else t
        if t is None:
            raise ValueError(f"init needs {name} (or prior_{name}): the chain's first level is drawn around the arm centres")
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3 or not t.dtype.is_floating_point or t.shape[0] < n_prior:
            raise ValueError(f"init['{name}'] must be a float tensor [n_prior,3] with a row for every entry of ligand_decomp_batch")
        per_atom[name] = t.detach().to(device=dev, dtype=torch.float32)[ligand_decomp_batch.to(dev)].contiguous()
    log_priors = {}
    for name, nc in (("atom_prior", num_classes), ("bond_prior", num_bond_classes)):
        p = init.get(name)
        if p is None:
            log_priors[name] = None
            continue
        p = torch.as_tensor(p)
        if tuple(p.shape) != (nc,) or not p.dtype.is_floating_point:
            raise ValueError(f"init['{name}'] must be a float probability vector of shape ({nc},), got {tuple(p.shape)} {p.dtype}")
        p = p.detach().cpu().double()
        if not bool(torch.isfinite(p).all()) or bool((p < 0).any()) or float(p.sum()) <= 0:
            raise ValueError(f"init['{name}'] must hold finite non-negative probabilities with a positive sum")
        # (as DiscreteTransition: normalised, log of the clamped probabilities)
        log_priors[name] = torch.log((p / p.sum()).clamp(min=1e-30)).to(device=dev, dtype=torch.float32).contiguous()
    out = dict(mode=mode, cen=per_atom["centers"], std=per_atom["stds"], atom_lp=log_priors["atom_prior"],
               bond_lp=log_priors["bond_prior"], pos=None, v=None, bond=None)
    if mode == "noised":
        pos, v, bond = (torch.as_tensor(init[k]) for k in ("pos", "v", "bond"))
        for name, t, shape in (("pos", pos, (n, 3)), ("v", v, (n,)), ("bond", bond, (n_bond,))):
            if tuple(t.shape) != shape:
                raise ValueError(f"init['{name}'] must have shape {shape}, got {tuple(t.shape)}")
        if not pos.dtype.is_floating_point:
            raise ValueError("init['pos'] must be a float tensor")
        if v.dtype.is_floating_point or bond.dtype.is_floating_point or v.dtype == torch.bool or bond.dtype == torch.bool:
            raise ValueError("init['v'] and init['bond'] must be integer class ids")
        v_c, bond_c = v.detach().cpu().long(), bond.detach().cpu().long()
        if v_c.numel() and (int(v_c.min()) < 0 or int(v_c.max()) >= num_classes):
            raise ValueError(f"init['v'] holds a class outside [0, {num_classes})")
        if bond_c.numel() and (int(bond_c.min()) < 0 or int(bond_c.max()) >= num_bond_classes):
            raise ValueError(f"init['bond'] holds a class outside [0, {num_bond_classes})")
        out.update(pos=pos.detach().to(device=dev, dtype=torch.float32).contiguous(), v=v_c.to(device=dev, dtype=torch.int32),
                   bond=bond_c.to(device=dev, dtype=torch.int32))
    return out


def stride_levels(num_timesteps, n):
    """``n`` distinct time levels of a schedule of ``num_timesteps``, evenly spaced from ``num_timesteps - 1`` down to 0 (both
    included) and strictly decreasing: a ``time_levels`` of sample_diffusion.  ``n = num_timesteps``: the full list."""
    T, n = int(num_timesteps), int(n)
    if not 2 <= n <= T:
        raise ValueError(f"stride_levels needs 2 <= n <= num_timesteps, got n = {n}, num_timesteps = {T}")
    return [((T - 1) * (n - 1 - i) + (n - 1) // 2) // (n - 1) for i in range(n)]     # (rounded; steps of >= 1: distinct)


def _as_time_levels(time_levels, num_timesteps):
    """``time_levels`` of sample_diffusion, validated (ValueError): the int64 tensor [S] of the real level of every VIRTUAL level
    0 .. S - 1, i.e. the caller's strictly decreasing list reversed."""
    if torch.is_tensor(time_levels):
        if time_levels.dim() != 1 or time_levels.dtype.is_floating_point or time_levels.dtype.is_complex or time_levels.dtype == torch.bool:
            raise ValueError("time_levels must be a one-dimensional integer tensor, array or sequence of ints")
        vals = time_levels.detach().cpu().tolist()
    elif isinstance(time_levels, np.ndarray):
        if time_levels.ndim != 1 or time_levels.dtype.kind not in "iu":
            raise ValueError("time_levels must be a one-dimensional integer tensor, array or sequence of ints")
        vals = time_levels.tolist()
    else:
        try:
            vals = list(time_levels)
        except TypeError:
            raise ValueError("time_levels must be a one-dimensional integer tensor, array or sequence of ints") from None
        if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in vals):
            raise ValueError("time_levels must hold ints")
        vals = [int(v) for v in vals]
    if len(vals) < 2:
        raise ValueError("time_levels needs at least two levels")
    if any(not 0 <= v <= num_timesteps - 1 for v in vals):
        raise ValueError(f"time_levels must lie in [0, {num_timesteps - 1}]")
    if any(a <= b for a, b in zip(vals, vals[1:])):
        raise ValueError("time_levels must be strictly decreasing (execution order, no level twice)")
    return torch.tensor(vals[::-1], dtype=torch.int64)


def _virtual_window(levels, t_min, t_max):
    """The virtual levels whose real level (``levels`` int64 [S], ascending) lies in the real window [t_min, t_max], as the
    inclusive range (lo, hi) -- contiguous, the list is monotonic -- or None: no level does."""
    lo = int(torch.searchsorted(levels, torch.tensor(int(t_min)), right=False))
    hi = int(torch.searchsorted(levels, torch.tensor(int(t_max)), right=True)) - 1
    return (lo, hi) if lo <= hi else None


def resample_schedule(t_hi, t_lo, j, r):
    """The resampling ("jump-back") schedule of ``sample_diffusion(resample=dict(jump_length=j, n_resample=r))`` over the reverse
    steps t_hi .. t_lo: a list of ``("step", t)`` and ``("jump", l, l + j)`` in execution order.  Jump points are anchored at the
    range's last level: every level l in {t_lo - 1, t_lo - 1 + j, ...} with l + j <= t_hi is left r - 1 times by a jump back
    to l + j.  ``num_steps // j`` jump points, ``num_steps + (r - 1) * j * (num_steps // j)`` steps; r = 1 or j > num_steps: the
    plain chain."""
    budget = {l: r - 1 for l in range(t_lo - 1, t_hi - j + 1, j)}
    ops, t = [], t_hi
    while t >= t_lo:
        ops.append(("step", t))
        l = t - 1
        if budget.get(l, 0) > 0:
            budget[l] -= 1
            ops.append(("jump", l, l + j))
            t = l + j
        else:
            t = l
    return ops


def _as_resample(resample, fixed, noise, num_timesteps, num_steps, start_step):
    """``resample`` of sample_diffusion, validated (ValueError): dict(j, r, runs, t_traj, n_total) -- ``runs``: [(reverse steps,
    followed by a jump)] in execution order; ``t_traj``: the int64 times of the n_total positions."""
    if not isinstance(resample, dict) or set(resample) != {"jump_length", "n_resample"}:
        raise ValueError("resample must be None or a dict(jump_length=j, n_resample=r)")
    j, r = resample["jump_length"], resample["n_resample"]
    if isinstance(j, bool) or isinstance(r, bool) or not isinstance(j, int) or not isinstance(r, int):
        raise ValueError("resample['jump_length'] and resample['n_resample'] must be ints")
    if j < 1 or r < 1:
        raise ValueError("resample needs jump_length >= 1 and n_resample >= 1")
    if fixed is None:
        raise ValueError("resample is valid only together with fixed: it re-harmonises the free atoms with the held ones")
    if noise is not None:
        raise ValueError("resample excludes noise=: a revisited time draws afresh from the device generator")
    if num_timesteps > 65535:
        raise ValueError("resample needs num_timesteps <= 65535 (the epoch shares the Philox time word with t)")
    t_hi = num_timesteps - 1 - int(start_step)
    t_lo = t_hi - int(num_steps) + 1
    if (r - 1) * (int(num_steps) // j) > 65535:
        raise ValueError("resample: more than 65535 jumps in one call")
    runs, times, n = [], [], 0
    for op in resample_schedule(t_hi, t_lo, j, r) if num_steps > 0 else []:
        if op[0] == "step":
            times.append(op[1])
            n += 1
        else:
            runs.append((n, True))
            n = 0
    if n:
        runs.append((n, False))
    return dict(j=j, r=r, runs=runs, t_traj=torch.tensor(times, dtype=torch.int64), n_total=len(times))


RESTRAINT_ANY = hip_lib.RESTRAINT_ANY              # group id "every real ligand atom of the sample" (not an arm id, not -1, not -2)
RESTRAINT_NONE = hip_lib.RESTRAINT_NONE            # ``group2`` of a row without a second endpoint (no arm id, not -1, -2 or -3)
_RESTRAINT_KEYS = {"type", "sample", "point", "min_d", "max_d", "weight", "atom", "group", "scale", "t_min", "t_max",
                   "classes", "classes2", "atom2", "group2", "form", "traj"}
_RESTRAINT_FORMS = {"linear": 0, "harmonic": 1}
_ALL_CLASSES = 0xFFFFFFFF                          # the class mask of an untyped endpoint


def _split_restraints(energy_drift_opt):
    """``energy_drift_opt`` as (the entries of the three built-in terms -- what `_drift_fields` takes --, the ``restraint`` entry or
    None).  The term may be listed once (ValueError)."""
    if energy_drift_opt is None:
        return None, None
    mine = [dr for dr in energy_drift_opt if isinstance(dr, dict) and dr.get("type") == "restraint"]
    if len(mine) > 1:
        raise ValueError("energy_drift_opt lists 'restraint' twice: put every restraint into one entry")
    return [dr for dr in energy_drift_opt if not (isinstance(dr, dict) and dr.get("type") == "restraint")], (mine[0] if mine else None)


def _class_masks(name, v, R, num_classes):
    """``classes`` / ``classes2`` of a restraint entry -- None, a bool tensor [R, num_classes], or R entries of None | class ids --
    as int64 [R] bit masks (bit c = class c; None: every bit), or None where the key is not given."""
    if v is None:
        return None
    if torch.is_tensor(v):
        if v.dtype != torch.bool or tuple(v.shape) != (R, num_classes):
            raise ValueError(f"restraint['{name}'] must be a bool tensor of shape ({R}, {num_classes}) or a list, got {v.dtype} {tuple(v.shape)}")
        rows = [r.nonzero()[:, 0].tolist() for r in v.detach().cpu()]
    else:
        try:
            rows = list(v)
        except TypeError:
            raise ValueError(f"restraint['{name}'] must be None, a bool tensor or a list of {R} class sets") from None
        if len(rows) != R:
            raise ValueError(f"restraint['{name}'] must hold {R} entries, got {len(rows)}")
    masks = []
    for ids in rows:
        if ids is None:
            masks.append(_ALL_CLASSES)
            continue
        try:
            ids = [i for i in (ids.tolist() if torch.is_tensor(ids) else ids)]
        except TypeError:
            raise ValueError(f"restraint['{name}']: a class set is None or an iterable of class ids") from None
        if any(isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < num_classes for i in ids):
            raise ValueError(f"restraint['{name}']: class ids must be ints in [0, {num_classes})")
        if not ids:
            raise ValueError(f"restraint['{name}']: an empty class set matches nothing (use a weight of 0 instead)")
        masks.append(sum(1 << i for i in set(ids)))
    return torch.tensor(masks, dtype=torch.long).reshape(R)


def _as_restraints(entry, batch_ligand, ligand_decomp_index, num_timesteps, num_classes=32):
    """The ``restraint`` entry of energy_drift_opt, validated (ValueError) into host tensors in the CALLER's restraint order:
    dict(R, sample int64 [R], point f32 [R,3], min_d / max_d / weight f32 [R], atom int32 [R] -- the row WITHIN the sample, or -1 --,
    group int32 [R], first int64 [B] -- the first flat ligand row of every sample --, scale, t_min, t_max) and the general form:
    cls / cls2 int64 [R] class masks or None (key not given), pair bool [R], atom2 int32 [R] (row within the sample or -1), group2
    int32 [R] (RESTRAINT_NONE off the pairs), form int32 [R], traj, general -- does the entry use anything the point kernel lacks."""
    if not isinstance(entry, dict) or set(entry) - _RESTRAINT_KEYS or "sample" not in entry or \
            ("point" not in entry and "atom2" not in entry and "group2" not in entry):
        raise ValueError(f"a restraint entry takes the keys {sorted(_RESTRAINT_KEYS)} and needs sample and point")
    bl = batch_ligand.detach().cpu().long()
    n = int(bl.numel())
    B = int(bl.max()) + 1 if n else 0
    counts = torch.bincount(bl, minlength=B) if n else torch.zeros(0, dtype=torch.long)
    first = torch.cumsum(counts, 0) - counts
    if n and not torch.equal(bl, torch.arange(B).repeat_interleave(counts)):
        raise ValueError("restraints need batch_ligand sorted by sample")

    def ints(name, t, shape):
        t = torch.as_tensor(t)
        if t.dtype.is_floating_point or t.dtype == torch.bool or t.dtype.is_complex or tuple(t.shape) != shape:
            raise ValueError(f"restraint['{name}'] must be an integer tensor of shape {shape}, got {t.dtype} {tuple(t.shape)}")
        return t.detach().cpu().long()

    sample = torch.as_tensor(entry["sample"])
    if sample.dim() != 1:
        raise ValueError("restraint['sample'] must be one-dimensional: the sample of every restraint")
    R = int(sample.numel())
    sample = ints("sample", sample, (R,))
    if R and (int(sample.min()) < 0 or int(sample.max()) >= B):
        raise ValueError(f"restraint['sample'] must lie in [0, {B})")
    if not 1 <= int(num_classes) <= 32:
        raise ValueError("restraint class masks hold 32 classes")
    # the second endpoint: a restraint is a pair iff its atom2 >= 0 or its group2 is given
    atom2 = entry.get("atom2")
    atom2 = torch.full((R,), -1, dtype=torch.long) if atom2 is None else ints("atom2", atom2, (R,))
    group2 = entry.get("group2")
    if group2 is not None and not torch.is_tensor(group2):
        try:
            group2 = [RESTRAINT_NONE if g is None else g for g in group2]
        except TypeError:
            raise ValueError(f"restraint['group2'] must be None, an integer tensor of shape ({R},) or a list") from None
    group2 = torch.full((R,), RESTRAINT_NONE, dtype=torch.long) if group2 is None else ints("group2", group2, (R,))
    explicit2 = atom2 >= 0
    pair = explicit2 | (group2 != RESTRAINT_NONE)
    if entry.get("point") is None:
        if not bool(pair.all()):
            raise ValueError("restraint['point'] may be None only when every restraint is a pair (atom2 / group2): a pair without a second endpoint")
        entry = dict(entry, point=torch.zeros(R, 3))
    point = torch.as_tensor(entry["point"])
    if not point.dtype.is_floating_point or tuple(point.shape) != (R, 3):
        raise ValueError(f"restraint['point'] must be a float tensor of shape ({R}, 3), got {point.dtype} {tuple(point.shape)}")
    point = point.detach().cpu().to(torch.float32)
    if not bool(torch.isfinite(point).all()):
        raise ValueError("restraint['point'] must be finite")
    per = {}
    for name, default in (("min_d", None), ("max_d", None), ("weight", 1.0)):
        v = entry.get(name, default)
        if v is None:
            raise ValueError(f"a restraint entry needs {name}")
        v = torch.as_tensor(v)
        if v.dtype == torch.bool or v.dtype.is_complex or tuple(v.shape) not in ((), (R,)):
            raise ValueError(f"restraint['{name}'] must be a number or a tensor of shape ({R},), got {tuple(v.shape)}")
        per[name] = v.detach().cpu().to(torch.float32).expand(R).contiguous()
    if bool(torch.isnan(per["min_d"]).any() | torch.isinf(per["min_d"]).any() | (per["min_d"] < 0).any()):
        raise ValueError("restraint['min_d'] must be finite and >= 0")
    if bool(torch.isnan(per["max_d"]).any() | (per["max_d"] == -math.inf).any() | (per["min_d"] > per["max_d"]).any()):
        raise ValueError("restraint needs min_d <= max_d (max_d may be +inf)")
    if not bool(torch.isfinite(per["weight"]).all()) or bool((per["weight"] < 0).any()):
        raise ValueError("restraint['weight'] must be finite and >= 0")
    atom = entry.get("atom")
    atom = torch.full((R,), -1, dtype=torch.long) if atom is None else ints("atom", atom, (R,))
    explicit = atom >= 0
    if bool((atom < -1).any()) or bool((atom >= n).any()) or not torch.equal(bl[atom[explicit]], sample[explicit]):
        raise ValueError("restraint['atom'] must be -1 (use group) or a flat ligand row of the restraint's own sample")
    group = entry.get("group")
    group = torch.full((R,), RESTRAINT_ANY, dtype=torch.long) if group is None else ints("group", group, (R,))
    grp = group[~explicit]
    if bool(((grp < -1) & (grp != RESTRAINT_ANY)).any()):
        raise ValueError("restraint['group'] must be RESTRAINT_ANY, -1 (scaffold) or an arm id >= 0")
    if ligand_decomp_index is None and bool((grp != RESTRAINT_ANY).any()):
        raise ValueError("a scaffold / arm restraint needs ligand_decomp_index")
    group = torch.where(explicit, torch.full_like(group, RESTRAINT_ANY), group)      # (not read for an explicit atom)
    if bool((atom2 < -1).any()) or bool((atom2 >= n).any()) or not torch.equal(bl[atom2[explicit2]], sample[explicit2]):
        raise ValueError("restraint['atom2'] must be -1 or a flat ligand row of the restraint's own sample")
    if bool((explicit & explicit2 & (atom == atom2)).any()):
        raise ValueError("restraint['atom2'] must differ from restraint['atom']: a pair needs two atoms")
    grp2 = group2[pair & ~explicit2]
    if bool(((grp2 < -1) & (grp2 != RESTRAINT_ANY)).any()):
        raise ValueError("restraint['group2'] must be RESTRAINT_ANY, -1 (scaffold), an arm id >= 0 or RESTRAINT_NONE (no second endpoint)")
    if ligand_decomp_index is None and bool((grp2 != RESTRAINT_ANY).any()):
        raise ValueError("a scaffold / arm group2 needs ligand_decomp_index")
    group2 = torch.where(explicit2, torch.full_like(group2, RESTRAINT_ANY), group2)  # (not read for an explicit atom)
    group2 = torch.where(pair, group2, torch.full_like(group2, RESTRAINT_NONE))
    cls, cls2 = (_class_masks(k, entry.get(k), R, int(num_classes)) for k in ("classes", "classes2"))
    form = entry.get("form", "linear")
    forms = [form] * R if isinstance(form, str) else (list(form) if isinstance(form, (list, tuple)) else None)
    if forms is None or len(forms) != R or any(not isinstance(f, str) or f not in _RESTRAINT_FORMS for f in forms):
        raise ValueError(f"restraint['form'] must be one of {sorted(_RESTRAINT_FORMS)} or a list of {R} of them")
    form = torch.tensor([_RESTRAINT_FORMS[f] for f in forms], dtype=torch.int32).reshape(R)
    traj = entry.get("traj", False)
    if not isinstance(traj, bool):
        raise ValueError("restraint['traj'] must be a bool")
    T = int(num_timesteps)
    t_min, t_max = entry.get("t_min"), entry.get("t_max")
    t_min, t_max = 0 if t_min is None else t_min, T - 1 if t_max is None else t_max
    if any(isinstance(t, bool) or not isinstance(t, int) for t in (t_min, t_max)) or not 0 <= t_min <= t_max <= T - 1:
        raise ValueError(f"restraint needs ints 0 <= t_min <= t_max <= {T - 1}")
    scale = entry.get("scale", False)
    if not isinstance(scale, (bool, int)):
        raise ValueError("restraint['scale'] must be a bool")
    local = torch.where(explicit, atom - first[sample], atom) if R else atom
    local2 = torch.where(explicit2, atom2 - first[sample], atom2) if R else atom2
    general = cls is not None or cls2 is not None or bool(pair.any()) or bool(form.any()) or traj
    return dict(R=R, sample=sample, point=point, min_d=per["min_d"], max_d=per["max_d"], weight=per["weight"],
                atom=local.to(torch.int32), group=group.to(torch.int32), first=first, scale=bool(scale), t_min=int(t_min), t_max=int(t_max),
                cls=cls, cls2=cls2, pair=pair, atom2=local2.to(torch.int32), group2=group2.to(torch.int32), form=form, traj=traj,
                general=general)


def _place_restraints(rs, ids, B, offset):
    """The call's restraints ``rs`` (`_as_restraints`) as ONE chain's share, sorted by the chain's sample slot -- a stable sort: the
    caller's order within a sample -- with the CSR ``ptr`` [B+1] rebuilt.  ``ids``: the call's samples in the chain's order (None:
    all, in order); ``offset`` [B,3]: the chain's offsets, points are centred as the ligand is (the fp32 ``p - offset[slot]``).
    ``order``: the caller's restraint index of every row (the way back).  ``atom`` / ``atom2`` stay the row within the sample: the
    explicit atom of a padded chain sits at padded row ``slot * NL + atom``, that of a group's chain at ``slot * n + atom``.  The
    general form's arrays travel with their restraint; an entry written before it (no ``general`` key) is a point entry."""
    slot_of = torch.arange(B) if ids is None else torch.full((int(rs["first"].numel()),), -1, dtype=torch.long).index_put_(
        (torch.as_tensor(list(ids), dtype=torch.long),), torch.arange(len(ids)))
    slot = slot_of[rs["sample"]] if rs["R"] else torch.zeros(0, dtype=torch.long)
    keep = (slot >= 0).nonzero()[:, 0]
    order = keep[torch.sort(slot[keep], stable=True).indices]
    slot = slot[order]
    ptr = torch.zeros(B + 1, dtype=torch.int32)
    ptr[1:] = torch.cumsum(torch.bincount(slot, minlength=B), 0).to(torch.int32)
    point = rs["point"][order].to(offset.device) - offset.detach().to(torch.float32)[slot.to(offset.device)]
    out = dict(R=int(order.numel()), order=order, slot=slot, ptr=ptr, point=point.contiguous(), min_d=rs["min_d"][order],
               max_d=rs["max_d"][order], weight=rs["weight"][order], atom=rs["atom"][order], group=rs["group"][order],
               first=rs["first"][rs["sample"][order]], scale=rs["scale"], t_min=rs["t_min"], t_max=rs["t_max"],
               general=bool(rs.get("general", False)), traj=bool(rs.get("traj", False)))
    if out["general"]:
        for k in ("pair", "atom2", "group2", "form"):
            out[k] = rs[k][order]
        for k in ("cls", "cls2"):
            out[k] = torch.full((out["R"],), _ALL_CLASSES, dtype=torch.long) if rs[k] is None else rs[k][order]
    return out


@dataclasses.dataclass(frozen=True)
class _Call:
    """What one sample_diffusion call asks for apart from its batch: built once, after validation, and handed to every batch path
    (dense, padded, equal-size groups).  ``drift`` is energy_drift_opt without its ``restraint`` entry; ``sample_keys`` / ``fixed`` /
    ``resample`` / ``chain_init`` / ``restraints`` are what `_as_sample_keys` / `_as_fixed` / `_as_resample` / `_as_init` /
    `_as_restraints` returned, in the CALLER's sample, row and restraint order (`_chain_rows` lays them into a chain)."""
    num_timesteps: int
    num_steps: int
    start_step: int = 0
    center_pos_mode: Optional[str] = "protein"
    drift: Optional[list] = None
    noise: Optional[dict] = None
    seed: int = 0
    keep_traj: bool = True
    use_graph: bool = True
    drift_norm_batch: int = 0
    sample_keys: Optional[torch.Tensor] = None
    fixed: Optional[dict] = None
    resample: Optional[dict] = None
    chain_init: Optional[dict] = None
    restraints: Optional[dict] = None
    schedule: Optional[dict] = None     # a strided call's schedule set (`_schedule_set`; num_timesteps is then its length S)
    levels: Optional[torch.Tensor] = None   # ... and the int64 real level of every virtual level 0 .. S - 1 (ascending)

    def __post_init__(self):
        if self.start_step < 0 or self.num_steps + self.start_step > self.num_timesteps:
            raise ValueError("num_steps (+ start_step) exceeds num_timesteps")

    @property
    def t_start(self):                  # time_seq = reversed(range(T - num_steps, T)), decompdiff.py:575
        return self.num_timesteps - 1 - int(self.start_step)

    @property
    def n_pos(self):                    # trajectory positions: the reverse steps the chain runs
        return self.num_steps if self.resample is None else self.resample["n_total"]

    @property
    def t_traj(self):                   # the int64 time of every position, for the calls that report it: resampled, strided (real levels)
        if self.resample is not None:
            t = self.resample["t_traj"]
        elif self.levels is not None:
            t = torch.arange(self.t_start, self.t_start - int(self.num_steps), -1, dtype=torch.int64)
        else:
            return None
        return t if self.levels is None else self.levels[t]


class _Placement:
    """Where the caller's flat ligand-atom rows and bond rows go in ONE chain's dense [B*NL] / [B*Eb] layout.  Taking: a group's
    chain owns the rows ``rows_l`` / ``rows_b`` (host index tensors) of the call, every other chain owns them all.  Putting: a
    padded batch scatters its rows to ``put_l`` / ``put_b`` (`BatchLayout.padded_rows()`, of ``n_l`` / ``n_b`` dense rows) over a
    fill value; every other chain holds them as they are (a reshape: no copy, no launch).  ``sample``: the chain's sample slot of
    each of its atom rows; ``ids``: the call's samples in the chain's order (None: all); ``n_bonds``: the chain's real bonds."""

    def __init__(self, sample, n_bonds, rows_l=None, rows_b=None, ids=None, put_l=None, put_b=None, n_l=0, n_b=0, dev=None):
        self.sample, self.n_bonds, self.ids = sample, int(n_bonds), ids
        self.rows_l, self.rows_b = rows_l, rows_b
        self.d_l, self.d_b = (None, None) if rows_l is None else (rows_l.to(dev), rows_b.to(dev))     # (the same, on the chain's device)
        self.put_l, self.put_b, self.n_l, self.n_b = put_l, put_b, n_l, n_b

    def take(self, t, bonds=False, dim=0):
        rows, d_rows = (self.rows_b, self.d_b) if bonds else (self.rows_l, self.d_l)
        if rows is None:
            return t
        rows = d_rows if t.device == d_rows.device else rows
        return t[rows] if dim == 0 else t[:, rows]

    def put(self, t, bonds=False, fill=0, dim=0):
        return self._scatter(t, *((self.put_b, self.n_b) if bonds else (self.put_l, self.n_l)), fill, dim)

    @staticmethod
    def _scatter(t, rows, n, fill, dim):
        if rows is None:
            return t
        shape = tuple(t.shape[:dim]) + (n,) + tuple(t.shape[dim + 1:])
        out = torch.full(shape, fill, dtype=t.dtype, device=t.device) if fill else torch.zeros(shape, dtype=t.dtype, device=t.device)
        return out.index_copy_(dim, rows, t)

    def atoms(self, t, fill=0, dim=0):
        return self.put(self.take(t, False, dim), False, fill, dim)

    def bonds(self, t, fill=0, dim=0):
        return self.put(self.take(t, True, dim), True, fill, dim)


def _chain_rows(call, place, offset, prior_stds, ligand_decomp_batch, ligand_decomp_index, num_classes, full_protein=(None, None)):
    """The per-row inputs of ONE chain in its dense layout, as `_make_sampler` consumes them.  From the chain's own batch tensors
    (``prior_stds`` ... ``full_protein`` = (full_protein_pos, full_batch_protein); put only): ``atom_std`` [B*NL,3], ``decomp`` int32
    [B*NL] or None, ``fpp`` [B,NF,3] (only with a clash drift, else None).  From the call record (taken, then put): ``keys`` int64 [B]
    or None; ``noise`` dict(u_v, u_b, eps) or None; ``fx`` -- the fixed atoms, dict(mode, init, mask uint8 [B*NL], v0 int32 [B*NL], b0
    int32 [B*Eb], x0c [B*NL,3] centred, cc [B*NL,3] centred or None) -- or None; ``ci`` -- what dd_chain_init draws the first level
    from, dict(mode, cc [B*NL,3] centred, std [B*NL,3], atom_lp / bond_lp or None and, mode "noised", x0c centred, v0, b0) -- or None;
    ``rs`` -- the chain's share of the distance restraints (`_place_restraints`: sorted by sample slot, points centred) -- or None.
    Centring is the ligand's own: the fp32 subtraction ``x - offset[row's sample]``.  Padding rows of a padded chain: 0; 0.5 in u_v /
    u_b; -2 (neither arm nor scaffold) in decomp; 1e6 in fpp (exp(-|p - y|^2 / sigma) underflows to exactly 0: nothing added to any sum)."""
    dev, B = offset.device, int(offset.shape[0])
    f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32)
    out = dict(atom_std=place.put(f32(prior_stds)[ligand_decomp_batch.to(dev)]).contiguous(), decomp=None, fpp=None, noise=None,
               fx=None, ci=None, rs=None if call.restraints is None else _place_restraints(call.restraints, place.ids, B, offset),
               keys=call.sample_keys if call.sample_keys is None or place.ids is None else call.sample_keys[place.ids])
    if ligand_decomp_index is not None:
        out["decomp"] = place.put(ligand_decomp_index.to(device=dev, dtype=torch.int32), fill=-2).contiguous()
    if call.drift is not None and any(dr["type"] == "clash" for dr in call.drift):
        fpos, fbatch = full_protein
        if fpos is None or fbatch is None:
            raise ValueError("clash drift needs full_protein_pos / full_batch_protein")
        if place.put_l is None:
            nf = fpos.shape[0] // B
            if fpos.shape[0] % B or not torch.equal(fbatch.to(dev), torch.arange(B, device=dev).repeat_interleave(nf)):
                raise NotImplementedError("full_protein_pos must hold the same number of atoms per sample")
            out["fpp"] = f32(fpos).contiguous().view(B, nf, 3)
        else:
            n_f = BL.sample_counts(fbatch, B)
            out["fpp"] = _Placement._scatter(f32(fpos), BL.block_rows(n_f, max(n_f)).to(dev), B * max(n_f), 1.0e6, 0).view(B, max(n_f), 3)
    if call.noise is not None:
        n_l, out["noise"] = int(place.sample.numel()), {}
        for k, bonds, fill, shp in (("u_v", False, 0.5, (call.num_steps, n_l, num_classes)), ("u_b", True, 0.5, (call.num_steps, place.n_bonds, 5)),
                                    ("eps", False, 0, (call.num_steps, n_l, 3))):
            t = place.take(call.noise[k], bonds, 1)
            if tuple(t.shape) != shp:
                raise ValueError(f"noise['{k}'] must have shape {shp}, got {tuple(t.shape)}")
            out["noise"][k] = place.put(f32(t), bonds, fill, 1)
    fixed, ini = call.fixed, call.chain_init
    if fixed is not None or ini is not None:
        off_l = offset[place.sample.to(dev)]
        centred = lambda x: place.put(place.take(x) - off_l).contiguous()
    if fixed is not None:                                  # (padding rows: not held)
        out["fx"] = dict(mode=fixed["mode"], init=fixed["init"], mask=place.put(place.take(fixed["mask"]).to(torch.uint8)),
                         v0=place.atoms(fixed["v"]), b0=place.bonds(fixed["bond"]), x0c=centred(fixed["pos"]),
                         cc=None if fixed["cc"] is None else centred(fixed["cc"]))
    if ini is not None:                                    # (padding rows are never drawn)
        noised = ini["mode"] == "noised"
        out["ci"] = dict(ini, cc=centred(ini["cen"]), std=place.atoms(ini["std"]), x0c=centred(ini["pos"]) if noised else None,
                         v0=place.atoms(ini["v"]) if noised else None, b0=place.bonds(ini["bond"]) if noised else None)
    return out


def _drift_fields(drift, has_decomp):
    """``energy_drift_opt`` as the drift fields of dd_sampler (a term that is not listed: zeros)."""
    f, seen = dict(drift_armsca=0, armsca_min_d=0.0, armsca_max_d=0.0, armsca_scale=0, drift_clash=0, clash_sigma=0.0, clash_gamma=0.0,
                   clash_scale=0, drift_repul=0, repul_max_d=0.0, repul_scale=0), []
    for dr in drift or []:
        if dr["type"] in seen:                             # one buffer per term: a repeated entry would silently replace the first
            raise NotImplementedError(f"energy_drift_opt lists '{dr['type']}' twice")
        seen.append(dr["type"])
        scale = int(bool(dr.get("scale", False)))
        if dr["type"] == "armsca_prox":
            f.update(drift_armsca=1, armsca_min_d=float(dr["min_d"]), armsca_max_d=float(dr["max_d"]), armsca_scale=scale)
        elif dr["type"] == "clash":
            f.update(drift_clash=1, clash_sigma=float(dr["sigma"]), clash_gamma=float(dr["gamma"]), clash_scale=scale)
        elif dr["type"] == "arms_repul":
            # EXTENSION: the reference defines the energy (utils/guidance_funcs.py:81-118) but its
            # sample_diffusion has no branch for it (decompdiff.py:643-675 raises ValueError); wired like armsca_prox
            # (:648-659): gradient at x_t, optional `scale`.  Defaults = the function's own (max_d 1.9, mode 'min').
            mode = dr.get("mode", "min")
            if mode not in ("min", "all"):
                raise ValueError(mode)                     # (guidance_funcs.py:90)
            if not has_decomp:
                raise ValueError("arms_repul drift needs ligand_decomp_index")
            f.update(drift_repul=1 if mode == "min" else 2, repul_max_d=float(dr.get("max_d", 1.9)), repul_scale=scale)
        elif dr["type"] in ("center_prox", "mmff_min"):
            raise NotImplementedError(f"drift '{dr['type']}' is outside the shipped sampling path "
                                      "(center_prox raises in the reference; mmff_min is RDKit/CPU)")
        else:
            raise ValueError(dr["type"])
    return f


class DecompScorePosNet3D(nn.Module):

    def __init__(self, config, protein_atom_feature_dim, ligand_atom_feature_dim, num_classes,
                 prior_atom_types=None, prior_bond_types=None):
        super().__init__()
        self.config = config
        self.model_mean_type = config.model_mean_type
        self.add_prior_node = getattr(config, "add_prior_node", False)
        self.bond_diffusion = getattr(config, "bond_diffusion", False)
        self.bond_net_type = getattr(config, "bond_net_type", "mlp")
        self.x2h_out_fc = bool(getattr(config, "x2h_out_fc", False))
        self.h_node_in_bond_net = bool(getattr(config, "h_node_in_bond_net", False))
        self.sample_time_method = getattr(config, "sample_time_method", "symmetric")
        self.loss_pos_type = getattr(config, "loss_pos_type", "mse")
        self.refine_net_type = config.model_type
        self.hidden_dim = config.hidden_dim
        self.center_pos_mode = config.center_pos_mode
        self.time_emb_dim = config.time_emb_dim
        self.num_classes = num_classes
        self.num_bond_classes = getattr(config, "num_bond_classes", 1)
        self._check_supported(config, protein_atom_feature_dim, ligand_atom_feature_dim, num_classes)

        # ---- schedule tables (same keys as the reference checkpoint)
        for k, v in schedules.position_tables(config).items():
            _attach(self, k, v, "const")
        self.num_timesteps = self.betas.size(0)
        for name, ncls, prior in (("atom_type_trans", num_classes, prior_atom_types),
                                  ("bond_type_trans", self.num_bond_classes, prior_bond_types)):
            tabs = schedules.categorical_tables(config.v_beta_schedule, self.num_timesteps, config.v_beta_s, ncls, prior)
            for k, v in tabs.items():
                _attach(self, f"{name}.{k}", v, "const")
        self.register_buffer("Lt_history", torch.zeros(self.num_timesteps))
        self.register_buffer("Lt_count", torch.zeros(self.num_timesteps))

        # ---- learnable tensors (reference module tree; default init ~ nn.Linear / nn.LayerNorm)
        gen = torch.Generator().manual_seed(0)
        shapes = learnable_param_shapes(config, protein_atom_feature_dim=protein_atom_feature_dim,
                                        ligand_atom_feature_dim=ligand_atom_feature_dim, num_classes=num_classes)
        gen_out = torch.Generator().manual_seed(1)          # (node_output MLPs, x2h_out_fc: drawn apart, behind the others)
        for k, shp in shapes.items():
            if ".node_output." in k and len(shp) == 2:
                t = (torch.rand(shp, generator=gen_out) * 2 - 1) * (1.0 / np.sqrt(shp[1]))
            elif ".node_output." in k and ".net.1." not in k:
                t = (torch.rand(shp, generator=gen_out) * 2 - 1) * 0.05
            elif len(shp) == 2:
                bound = 1.0 / np.sqrt(shp[1])
                t = (torch.rand(shp, generator=gen) * 2 - 1) * bound
            elif k.endswith(".net.1.weight"):
                t = torch.ones(shp)
            elif k.endswith(".net.1.bias"):
                t = torch.zeros(shp)
            else:
                t = (torch.rand(shp, generator=gen) * 2 - 1) * 0.05
            _attach(self, k, t, "param")

        # ---- non-learnable buffers of the reference modules
        off = torch.tensor(GAUSS_OFFSETS, dtype=torch.float32)
        _attach(self, "refine_net.distance_expansion.offset", off.clone(), "buffer")
        for l in range(config.num_layers):
            p = f"refine_net.base_block.{l}"
            _attach(self, f"{p}.distance_expansion.offset", off.clone(), "buffer")
            _attach(self, f"{p}.bond_layer.distance_expansion.offset", off.clone(), "buffer")
            _attach(self, f"{p}.bond_layer.angle_expansion.freq_bands",
                    torch.tensor([1.0, 2.0, 3.0, 1.0, 1.0 / 2.0, 1.0 / 3.0]), "buffer")
        if self.bond_diffusion:
            _attach(self, "distance_expansion.offset", torch.linspace(0.0, 5.0, config.num_r_gaussian), "buffer")

        self._packed = None
        self._packed_key = None

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def _check_supported(config, pdim, ldim, num_classes=8):
        def need(cond, what):
            if not cond:
                raise NotImplementedError(
                    f"decompdiff_amd implements the shipped sampling configuration only ({what}); "
                    "see DESIGN.md 'out of scope'")
        need(config.model_type == "uni_o2_bond", "model_type=uni_o2_bond")
        need(config.hidden_dim == 128 and config.n_heads == 16, "hidden_dim=128, n_heads=16")
        need(config.cutoff_mode == "knn", "cutoff_mode=knn")
        need(getattr(config, "bond_diffusion", False) and getattr(config, "bond_net_type", "mlp") in BOND_NET_TYPES,
             "bond_diffusion with bond_net_type in {lin, pre_att}")
        need(not getattr(config, "add_prior_node", False), "add_prior_node=False")
        need(config.time_emb_dim == 0, "time_emb_dim=0")
        need(config.node_indicator, "node_indicator=True")
        # (every step of a forward -- num_blocks * num_layers of them -- has a work counter of its own in the workspace: 64 slots)
        need(int(config.num_blocks) >= 1 and 1 <= int(config.num_blocks) * int(config.num_layers) <= 64,
             "1 <= num_blocks and num_blocks * num_layers <= 64")
        need(config.edge_feat_dim == 4 and config.num_r_gaussian == 20, "edge_feat_dim=4, num_r_gaussian=20")
        # h_node_in_bond_net (uni_transformer_edge.py:147-152; the encoder's default is False): both widths of the bond layer's
        # first Linears.  sync_twoup: stored by uni_o2_bond and never read in its forward -- accepted, changes nothing.
        need(getattr(config, "h_node_in_bond_net", False) in (False, True), "h_node_in_bond_net in {False, True}")
        need(config.x2h_out_fc in (False, True) and config.norm and config.act_fn == "relu", "x2h_out_fc in {False, True}, norm, relu")
        need(getattr(config, "num_bond_classes", 1) == 5, "num_bond_classes=5")
        # ligand_atom_mode basic / add_aromatic / full: 8 / 13 / 23 atom classes (utils/transforms.py:15-64,138-151;
        # scripts/sample_diffusion_decomp.py:538-540: feature dim = classes + the 2 arm / scaffold indicators)
        need(num_classes in (8, 13, 23), "num_classes in {8, 13, 23} (ligand_atom_mode basic / add_aromatic / full)")
        need(pdim == 29 and ldim == num_classes + 2, "protein feature dim 29, ligand feature dim num_classes + 2")
        need(1 <= config.knn <= 64, "1<=knn<=64")

    # ------------------------------------------------------------------------------------------
    def _device(self):
        return self.betas.device

    def invalidate_pocket_uploads(self):
        """Forget what the cached chains hold of the pocket side (protein coordinates / features / layer-0 rows): the next call of
        every cached shape uploads again.  Needed only after an in-place write that does not bump tensor version counters."""
        for ent in list(DecompScorePosNet3D._chain_cache.values()):
            if isinstance(ent, dict):
                ent["uploaded"] = None

    def invalidate_packed_weights(self):
        """Forget the packed weight arena (and with it the cached chain resources that point into it).  Called by
        load_state_dict / .to() / train(); call it by hand after modifying parameters in place."""
        self._packed = None
        self.__dict__["_param_list"] = None
        self._evict_chain_cache(0)

    def load_state_dict(self, *args, **kwargs):
        r = super().load_state_dict(*args, **kwargs)
        self.invalidate_packed_weights()
        return r

    def _apply(self, fn, *args, **kwargs):
        r = super()._apply(fn, *args, **kwargs)
        self.__dict__["_packed"] = None
        self.__dict__["_param_list"] = None                 # (.to() may replace the parameter tensors)
        return r

    def schedule_tables(self, levels=None):
        """The schedule tables the step tables are composed from, as one dict: the position tables by name, ``atom_type_trans`` /
        ``bond_type_trans`` -> their categorical tables.  ``levels=None``: this module's own buffers.  Otherwise (ascending time
        levels, S of them): the respaced schedule of `schedules.position_tables(config, levels)` / `categorical_tables(...,
        levels=...)`, composed in float64 from the config's schedule -- never from the fp32 buffers, whose small betas cancel --
        with this module's class priors."""
        if levels is None:
            tabs = {k: getattr(self, k).detach() for k in ("alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
                                                           "posterior_mean_c0_coef", "posterior_mean_ct_coef", "posterior_logvar",
                                                           "pos_score_coef")}
            for name in ("atom_type_trans", "bond_type_trans"):
                tabs[name] = {k: v.detach() for k, v in getattr(self, name)._parameters.items()}
            return tabs
        tabs = dict(schedules.position_tables(self.config, levels))
        for name, ncls in (("atom_type_trans", self.num_classes), ("bond_type_trans", self.num_bond_classes)):
            tabs[name] = schedules.categorical_tables(self.config.v_beta_schedule, self.num_timesteps, self.config.v_beta_s, ncls,
                                                      levels=levels)
            tabs[name]["prior_probs"] = getattr(self, name).prior_probs.detach().float().cpu()
        return tabs

    def position_step_table(self, model_mean_type=None, tables=None):
        """The [3][T] fp32 table the step kernels read as ``dd_sampler.tab_pos``: for each t, the coefficients of the network's
        coordinate output and of x_t in the posterior mean, then posterior_logvar.  C0: posterior_mean_c0_coef and
        posterior_mean_ct_coef as they are.  'noise': the eps -> x0 map of the reference (_predict_x0_from_eps,
        decompdiff.py:353-356) folded into them -- with eps = pred - x_t the mean c0 * x0 + ct * x_t is
        (-c0 * sqrt_recipm1) * pred + (ct + c0 * (sqrt_recip + sqrt_recipm1)) * x_t, the two rows composed in float64 from
        this module's schedule tables and rounded once.  ``tables`` (here and in the builders below): the `schedule_tables` dict to
        compose from; default this module's own."""
        mode = self.model_mean_type if model_mean_type is None else model_mean_type
        tb = self.schedule_tables() if tables is None else tables
        c0, ct = tb["posterior_mean_c0_coef"].detach(), tb["posterior_mean_ct_coef"].detach()
        if mode == "noise":
            c0d, ctd = c0.double(), ct.double()
            sr = tb["sqrt_recip_alphas_cumprod"].detach().double()
            srm1 = tb["sqrt_recipm1_alphas_cumprod"].detach().double()
            c0, ct = -c0d * srm1, ctd + c0d * (sr + srm1)
        elif mode != "C0":
            raise ValueError(mode)
        return torch.stack([c0.float(), ct.float(), tb["posterior_logvar"].detach().float()]).contiguous()

    def fixed_step_table(self, tables=None):
        """The [2][T] fp32 table the step kernels read as ``dd_fixed.tab`` (replace mode): sqrt(alphas_cumprod) and
        sqrt(1 - alphas_cumprod) of the forward process (decompdiff.py:436-449), composed in float64 from this module's
        ``alphas_cumprod`` and rounded once."""
        tb = self.schedule_tables() if tables is None else tables
        ac = tb["alphas_cumprod"].detach().double()
        return torch.stack([ac.sqrt(), (1.0 - ac).sqrt()]).float().contiguous()

    def resample_jump_table(self, jump_length, tables=None):
        """The [6][T] fp32 table ``dd_resample.tab`` of the forward jump from level m - j to level m (j = ``jump_length``), indexed
        by m: A = sqrt(a), S = sqrt(1 - a) with a = alphas_cumprod[m] / alphas_cumprod[m - j] (coordinates), then
        lr = log_cumprod[m] - log_cumprod[m - j] and l1mr = log(1 - exp(lr)) of the atom-type and of the bond-type schedule; level -1
        is the clean sample (alphas_cumprod 1, log_cumprod 0).  Composed in float64 from this module's schedule tables and rounded
        once, like ``fixed_step_table`` (whose rows A, S are this table's at m = j - 1).  Entries m < j - 1 are zeros, never read."""
        j = int(jump_length)
        if j < 1:
            raise ValueError("jump_length must be >= 1")
        tb = self.schedule_tables() if tables is None else tables
        T = int(tb["alphas_cumprod"].numel())
        ac = torch.cat([torch.ones(1, dtype=torch.float64), tb["alphas_cumprod"].detach().double().cpu()])        # [level + 1]
        lv = torch.cat([torch.zeros(1, dtype=torch.float64), tb["atom_type_trans"]["log_alphas_cumprod_v"].detach().double().cpu()])
        lb = torch.cat([torch.zeros(1, dtype=torch.float64), tb["bond_type_trans"]["log_alphas_cumprod_v"].detach().double().cpu()])
        tab = torch.zeros(6, T, dtype=torch.float64)
        if j <= T:
            m = torch.arange(j - 1, T)
            a = ac[m + 1] / ac[m + 1 - j]
            tab[0, m], tab[1, m] = a.sqrt(), (1.0 - a).sqrt()
            for row, lc in ((2, lv), (4, lb)):
                lr = lc[m + 1] - lc[m + 1 - j]
                tab[row, m], tab[row + 1, m] = lr, torch.log(1.0 - torch.exp(lr))
        return tab.float().contiguous()

    def _predict_x0_from_eps(self, xt, eps, t, batch):
        """x0 from a predicted noise (decompdiff.py:353-356); t [num_graphs], batch [n] on the device of the tables."""
        return self.sqrt_recip_alphas_cumprod[t][batch].unsqueeze(-1) * xt - \
            self.sqrt_recipm1_alphas_cumprod[t][batch].unsqueeze(-1) * eps

    def q_pos_posterior(self, x0, xt, t, batch):
        """Mean of q(x_{t-1} | x_t, x_0) (decompdiff.py:358-362)."""
        return self.posterior_mean_c0_coef[t][batch].unsqueeze(-1) * x0 + \
            self.posterior_mean_ct_coef[t][batch].unsqueeze(-1) * xt

    def _packed_weights(self):
        dev = self._device()
        # (the mean type selects the tab_pos rows: changing model.model_mean_type repacks)
        key = (str(dev), self.model_mean_type)
        # in-place parameter updates (optimizer.step on a loss of the caller's own, an EMA copy, param.data.copy_) bump the
        # tensors' version counters: the packed copy is rebuilt when their sum moves (the tensor list is kept: walking the
        # module tree costs 0.4 ms per call, the 600 attribute reads 0.05; DD_CHECK_PARAM_VERSIONS=0 turns the check off)
        if os.environ.get("DD_CHECK_PARAM_VERSIONS", "1") != "0":
            plist = self.__dict__.get("_param_list")
            if plist is None:
                plist = self.__dict__["_param_list"] = list(self.parameters())
            key = (key, sum(p._version for p in plist), id(plist))
        if self._packed is None or self._packed_key != key:
            if self._packed is not None:
                self._evict_chain_cache(0)                                  # cached chains point into the old arena
            sd = {k: v for k, v in self.state_dict().items()}
            arena, offsets, _ = packing.pack_model(sd, self.config, kernel_form=hip_lib.weights_form() == 1)
            # (the packed dict IS the schedule set of the module's own tables; a strided call's set: `_schedule_set`)
            self._packed = dict(arena=arena.to(dev), offsets=offsets.numpy().astype(np.int64).copy(),
                                **self._step_tables(self.schedule_tables(), dev))
            self._packed["bond_head"] = self._bond_head_descriptor(sd, self._packed)
            self._packed["node_out"] = self._node_out_descriptor(sd, self._packed)
            self._packed["model_opts"] = hip_lib.model_opts(self._packed["bond_head"], self._packed["node_out"], self.config.num_blocks)
            self._packed_key = key
        return self._packed


    def _step_tables(self, tables, dev):
        """The device tables every chain reads, composed from the `schedule_tables` dict ``tables``: tab_pos, tab_v, tab_b, tab_score
        (dd_sampler), with ``T`` (their length), ``tables`` and ``levels`` (None: the module's own schedule).  tab_fixed and
        tab_jump join them when a call first needs them (`_bind_call`)."""
        # (an unknown mean type never reaches a step kernel: sample_diffusion refuses it; forward does not read the rows)
        tab_pos = self.position_step_table("noise" if self.model_mean_type == "noise" else "C0", tables)
        # [4][T] schedule rows followed by the [K] class log-prior (uniform unless prior_*_types were given)
        cat = lambda t: torch.cat([t["log_alphas_v"], t["log_one_minus_alphas_v"], t["log_alphas_cumprod_v"],
                                   t["log_one_minus_alphas_cumprod_v"], t["prior_probs"].reshape(-1)]).detach().float().contiguous()
        return dict(tab_pos=tab_pos.to(dev), tab_v=cat(tables["atom_type_trans"]).to(dev), tab_b=cat(tables["bond_type_trans"]).to(dev),
                    tab_score=tables["pos_score_coef"].detach().float().contiguous().to(dev),
                    T=int(tables["pos_score_coef"].numel()), tables=tables, levels=None)

    _SCHEDULE_CACHE_MAX = 4

    def _schedule_set(self, pw, levels):
        """The schedule set (`_step_tables`) of a strided call over ``levels`` (a tuple of ascending ints): kept with the packed
        weights ``pw`` -- so per device and mean type, dropped when they are --, the least recently used beyond
        _SCHEDULE_CACHE_MAX forgotten (a cached chain holds its own set)."""
        sets = pw.setdefault("schedule_sets", {})
        sch = sets.pop(levels, None)
        if sch is None:
            sch = dict(self._step_tables(self.schedule_tables(levels), pw["arena"].device), levels=levels)
        sets[levels] = sch                                  # (re-inserted: most recently used last)
        while len(sets) > self._SCHEDULE_CACHE_MAX:
            sets.pop(next(iter(sets)))
        return sch

    def _bond_head_descriptor(self, sd, pw):
        """The dd_bond_head of the *_ex entry points: None for the lin head (the arena's BH_W1 / BH_b1 slots, the entry points'
        default); for 'pre_att' the factorised head of packing.bond_head_pre_att -- W_p = W1[:, 20:] / 2 sits in the BH_W1 slot
        (pack_global), b1 in BH_b1, W_r^T and the Gaussian centres in a small device buffer kept in the packed dict."""
        if self.bond_net_type != "pre_att":
            return None
        form = packing.bond_head_pre_att(sd, self.config)
        arena = pw["arena"]
        buf = torch.cat([form["W_r"].reshape(-1), form["offset"].reshape(-1)]).contiguous().to(arena.device)
        pw["bond_head_buf"] = buf
        g = self._global_offsets(pw)
        bh = hip_lib.DDBondHead()
        bh.kind, bh.num_r = hip_lib.BOND_HEAD_PRE_ATT, int(form["W_r"].shape[0])
        bh.W_p, bh.b1 = arena.data_ptr() + 4 * g["BH_W1"], arena.data_ptr() + 4 * g["BH_b1"]
        bh.W_r, bh.offset = buf.data_ptr(), buf.data_ptr() + 4 * form["W_r"].numel()
        bh.coeff = float(form["coeff"])
        return bh

    def _bond_head(self, pw=None):
        """ctypes pointer to this model's dd_bond_head, None for the lin head (NULL: the lin entry points' behaviour)."""
        pw = self._packed if pw is None else pw
        bh = pw.get("bond_head") if pw else None
        return None if bh is None else ctypes.pointer(bh)

    def _node_out_descriptor(self, sd, pw):
        """The dd_node_out of the *_ex2 entry points: None without x2h_out_fc; else the per-layer blocks of
        packing.node_out_fc in one device buffer kept in the packed dict (the descriptor points into it)."""
        if not self.x2h_out_fc:
            return None
        form = packing.node_out_fc({k: v.detach().float().cpu() for k, v in sd.items()}, self.config)
        buf = torch.stack([packing.node_out_block(f) for f in form]).contiguous().to(pw["arena"].device)
        pw["node_out_buf"] = buf
        no = hip_lib.DDNodeOut()
        no.num_layers = len(form)
        for l in range(len(form)):
            no.layer[l] = buf.data_ptr() + 4 * l * packing.NODE_OUT_BLOCK_FLOATS
        return no

    def _node_out(self, pw=None):
        """ctypes pointer to this model's dd_node_out, None without x2h_out_fc (NULL: the behaviour of the _ex entry points)."""
        pw = self._packed if pw is None else pw
        no = pw.get("node_out") if pw else None
        return None if no is None else ctypes.pointer(no)

    def _model_opts(self, pw=None):
        """ctypes pointer to this model's dd_model_opts (both descriptors and num_blocks), what every *_opts entry point takes."""
        pw = self._packed if pw is None else pw
        return ctypes.pointer(pw["model_opts"])

    def _layer0_tables(self, pw, dev):
        """dd_sampler.l0_tables for this weight set (built once): the first layer's projection / query rows of the 16
        (class, arm flag) combinations of a ligand atom and of the 5 x 16 (bond type, destination combination) pairs,
        produced by the forward's own embedding / projection / query kernels on a 16-atom problem (dd_layer0_tables)."""
        if "l0_tables" in pw:
            return pw["l0_tables"]
        pw["l0_tables"] = None
        if os.environ.get("DD_LAYER0_TABLES", "1") == "0" or self.num_classes != 8 or self.num_bond_classes != 5:
            return None
        lib = hip_lib.load()
        NL, K = 16, 15
        z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)
        i = torch.arange(NL, device=dev)
        keep = {"lig_pos": z(NL, 3), "lig_v": (i % 8).to(torch.int32).contiguous(),
                "lig_aux": torch.stack([(i < 8).float(), (i >= 8).float()], 1).contiguous(),
                "lig_bond": (torch.arange(NL - 1, device=dev) % 5).repeat(NL).to(torch.int32).contiguous(),
                "protein": z(4)}
        ws_floats = int(lib.dd_workspace_floats(1, 0, NL, K))
        keep["workspace"] = z(ws_floats)
        sm = hip_lib.DDSampler()
        sm.B, sm.NP, sm.NL, sm.K, sm.NF = 1, 0, NL, K, 0
        sm.num_layers, sm.T = int(self.config.num_layers), int(self.betas.numel())
        sm.weights, sm.slot_off = pw["arena"].data_ptr(), pw["offsets"].ctypes.data
        sm.protein_pos = sm.protein_h = keep["protein"].data_ptr()
        for k in ("lig_pos", "lig_v", "lig_aux", "lig_bond", "workspace"):
            setattr(sm, k, keep[k].data_ptr())
        sm.workspace_floats = ws_floats
        tables = z(hip_lib.L0_TABLE_FLOATS)
        hip_lib.check(lib.dd_layer0_tables(ctypes.byref(sm), hip_lib.ptr(tables), hip_lib.stream_ptr(dev)), "dd_layer0_tables")
        torch.cuda.current_stream(dev).synchronize()           # (the 16-atom problem's buffers die with this frame)
        pw["l0_tables"] = tables
        return tables

    # ------------------------------------------------------------------------------------------
    # Ragged batches (samples with different atom counts).  Every sample's chain is independent of the
    # rest of its batch (all graph ops of the reference are segmented by `batch`; tests/test_gpu_parity.py checks that
    # the kernels keep this bit for bit), so a ragged batch runs padded to its largest sample or as one dense launch
    # sequence per group of equal sizes.  Counts, validation, row maps and groups come from `batch_layout`.
    @staticmethod
    def _is_ragged(batch_protein, batch_ligand) -> bool:
        if batch_protein.numel() == 0 or batch_ligand.numel() == 0:
            return False
        n_p = BL.sample_counts(batch_protein)
        return not BL.BatchLayout(n_p, BL.sample_counts(batch_ligand, len(n_p))).is_dense

    @staticmethod
    def _sampling_layout(kw):
        """The validated layout of sample_diffusion's arguments.  (A sample without pocket atoms is left to the dense path.)"""
        if kw["ligand_fc_bond_index"] is None or kw["init_ligand_fc_bond_type"] is None:
            raise NotImplementedError("the uni_o2_bond path needs the fully connected ligand bond graph")
        has_full = kw["full_protein_pos"] is not None and kw["full_batch_protein"] is not None
        return BL.BatchLayout.from_batch(kw["batch_protein"], kw["batch_ligand"], kw["batch_prior"],
                                         kw["full_batch_protein"] if has_full else None, kw["batch_ligand_bond"],
                                         kw["ligand_fc_bond_index"], kw["init_ligand_fc_bond_type"].numel(), need_protein=False)

    def _sample_heterogeneous(self, kw, call):
        """Samples with different atom counts in one batch (PyG collate, utils/data.py:389-446).  Default: ONE launch
        sequence over the batch padded to its largest pocket / ligand with per-sample real counts (`_sample_padded`).
        Fallbacks to equal-size groups (`_sample_ragged`): DD_RAGGED_MODE=groups, or `batch_layout.fits_padded` says no."""
        layout = None
        if os.environ.get("DD_RAGGED_MODE", "padded") != "groups":
            layout = self._sampling_layout(kw)
            if BL.fits_padded(layout, self.config.knn):
                return self._sample_padded(kw, call, layout)
        return self._sample_ragged(kw, call, layout=layout)

    def _padded_inputs(self, protein_pos, protein_v, bp, ligand_pos, ligand_v, aux, bl, fc_index, bond_type, batch_ligand_bond,
                       n_p, n_l, center_pos_mode):
        """A heterogeneous flat batch validated by `BatchLayout.from_batch` (n_p / n_l: its atoms per sample) as the padded dense
        layout of dd_sampler.np_real / nl_real / bl_prefix (`BatchLayout.padded_rows`); padding rows are zeros.  Shared by the
        padded sampler and the ragged forward.  Returns the dense dict `d` of _make_sampler (positions centred by
        `center_pos_mode`), the per-sample offset, the masks, the row maps flat row -> padded row (rows_* on the host, d_* on
        the device) and the `_Placement` made of them."""
        dev = protein_pos.device
        hip_lib.require_gpu(protein_pos, "protein_pos")
        hip_lib.require_gpu(ligand_pos, "init_ligand_pos")
        layout = BL.BatchLayout(n_p, n_l)
        B, NP, NL, n_b = layout.B, max(n_p), max(n_l), layout.n_b
        Eb = NL * (NL - 1)
        rows_p, rows_l, rows_b = layout.padded_rows()
        d_p, d_l, d_b = rows_p.to(dev), rows_l.to(dev), rows_b.to(dev)
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32)
        if protein_v.dim() != 2 or protein_v.shape[1] != 29 or aux.dim() != 2 or aux.shape[1] != 2:
            raise ValueError("protein_v must be [n,29] and ligand_v_aux [n,2]")
        assert int(ligand_v.min()) >= 0 and int(ligand_v.max()) < self.num_classes, f"Error: {int(ligand_v.max())} >= {self.num_classes}"
        bt = bond_type
        assert int(bt.min()) >= 0 and int(bt.max()) < self.num_bond_classes, f"Error: {int(bt.max())} >= {self.num_bond_classes}"
        # center_pos (decompdiff.py:20-32): per-sample mean of the REAL protein atoms, fp32 in row order (as the dense path)
        if center_pos_mode == "protein":
            tot = torch.zeros(B, 3).index_add_(0, bp.cpu(), protein_pos.detach().float().cpu())
            offset = (tot / torch.tensor(n_p, dtype=torch.float32).clamp(min=1).view(B, 1)).to(dev)
        elif center_pos_mode == "none":
            offset = torch.zeros(B, 3, device=dev)
        else:
            raise NotImplementedError(center_pos_mode)
        zeros = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)
        ppos = zeros(B * NP, 3).index_copy_(0, d_p, f32(protein_pos) - offset[bp.to(dev)])
        lpos = zeros(B * NL, 3).index_copy_(0, d_l, f32(ligand_pos) - offset[bl.to(dev)])
        d = dict(B=B, NP=NP, NL=NL, protein_pos=ppos.view(B, NP, 3), ligand_pos=lpos.view(B, NL, 3),
                 protein_pos_centered=ppos.view(B, NP, 3), ligand_pos_centered=lpos.view(B, NL, 3),
                 protein_v=zeros(B * NP, 29).index_copy_(0, d_p, f32(protein_v)).view(B, NP, 29),
                 ligand_v=zeros(B * NL, dtype=torch.int32).index_copy_(0, d_l, ligand_v.to(device=dev, dtype=torch.int32)),
                 ligand_aux=zeros(B * NL, 2).index_copy_(0, d_l, f32(aux)).view(B, NL, 2),
                 bond=zeros(B * Eb, dtype=torch.int32).index_copy_(0, d_b, bt.to(device=dev, dtype=torch.int32)))
        prefix = np.concatenate([[0], np.cumsum(n_b)]).astype(np.int32)
        masks = {"np_real": torch.tensor(n_p, dtype=torch.int32), "nl_real": torch.tensor(n_l, dtype=torch.int32),
                 "bl_prefix": torch.from_numpy(prefix)}
        return dict(d=d, offset=offset, masks=masks, rows_l=rows_l, rows_b=rows_b, d_l=d_l, d_b=d_b,
                    place=_Placement(bl, sum(n_b), put_l=d_l, put_b=d_b, n_l=B * NL, n_b=B * Eb))

    def _sample_padded(self, kw, call, layout):
        """Heterogeneous batch as one padded dense batch: every sample's atoms are the first rows of its [NPmax] / [NLmax]
        blocks, the kernels read the real counts from dd_sampler.np_real / nl_real (padding atoms are no kNN candidates,
        own no softmax segment and are no members of one) and the results are gathered back into the caller's flat order.
        Exact: a sample's chain does not depend on its batch, with the one batch-wide quantity of the reference -- the
        armsca loss is averaged over the whole batch (guidance_funcs.py:78) -- unchanged because the batch is whole."""
        _check_ligand_atom_mask(kw.get("ligand_atom_mask"), kw["batch_ligand"].numel())
        pad = self._padded_inputs(kw["protein_pos"], kw["protein_v"], kw["batch_protein"], kw["init_ligand_pos"], kw["init_ligand_v"],
                                  kw["ligand_v_aux"], kw["batch_ligand"], kw["ligand_fc_bond_index"], kw["init_ligand_fc_bond_type"],
                                  kw["batch_ligand_bond"], layout.n_p, layout.n_l, call.center_pos_mode)
        d, offset = pad["d"], pad["offset"]
        rows = _chain_rows(call, pad["place"], offset, kw["prior_stds"], kw["ligand_decomp_batch"], kw["ligand_decomp_index"],
                           self.num_classes, (kw["full_protein_pos"], kw["full_batch_protein"]))
        s, bufs, ent = self._make_sampler(d, self._packed_weights(), call, rows, offset.contiguous(), masks=pad["masks"])   # (the padded batch keeps the caller's sample order)
        chain = dict(s=s, bufs=bufs, offset=offset, B=d["B"], NL=d["NL"], dev=d["protein_pos"].device, ent=ent,
                     t_traj=call.t_traj)
        self._run_chains([chain], call.n_pos, call.use_graph)
        out = self._collect_chain(chain, call.n_pos, call.keep_traj, rows_atoms=pad["rows_l"], rows_bonds=pad["rows_b"])
        self._restraint_results(call, [chain], out)
        self._last = (s, bufs)
        return out

    def _sample_ragged(self, kw, call, concurrent=None, split=1, layout=None):
        """One dense chain per group of samples of equal size (`BatchLayout.size_groups`).  ``split`` > 1 additionally cuts
        every group into that many sub-batches (measurement aid, tools/split_bench.py: two concurrent half-batches were
        measured slower than one chain).  ``layout``: what `_sampling_layout(kw)` gave the caller.
        With ``call.sample_keys`` (int64 [B], the caller's sample order) every group gets its members' keys; without keys group
        ``gi`` draws with ``call.seed + 7919 * gi``."""
        _check_ligand_atom_mask(kw.get("ligand_atom_mask"), kw["batch_ligand"].numel())
        dev = kw["protein_pos"].device
        layout = layout or self._sampling_layout(kw)
        B, has_full = layout.B, max(layout.n_f) > 0
        n_lig, n_bond = sum(layout.n_l), sum(layout.n_b)
        keep_traj, n_pos = call.keep_traj, call.n_pos
        out = {"pos": torch.empty(n_lig, 3, device=dev), "v": torch.empty(n_lig, dtype=torch.long, device=dev),
               "bond": torch.empty(n_bond, dtype=torch.long, device=dev)}
        traj: Dict[str, Optional[torch.Tensor]] = {k: None for k in ("pos_traj", "v_traj", "bond_traj", "v0_traj", "vt_traj", "bt_traj")}
        prepared = []
        for gi, g in enumerate(layout.size_groups([(b * split) // B for b in range(B)] if split > 1 else ())):
            G, r_l, r_b = len(g.ids), g.rows_l, g.rows_b
            b_p, b_l, fc = self._expected_layout(G, g.n_p, g.n_l, dev)          # (b_l: sample slot of each ligand row)
            place = _Placement(b_l, len(r_b), rows_l=r_l, rows_b=r_b, ids=g.ids, dev=dev)
            d_p, d_l, d_pr, d_b = g.rows_p.to(dev), place.d_l, g.rows_pr.to(dev), place.d_b
            old_pr0 = torch.tensor(g.first_pr, device=dev)
            chain = self._prepare_chain(
                kw["protein_pos"][d_p], kw["protein_v"][d_p], b_p, kw["init_ligand_pos"][d_l], kw["init_ligand_v"][d_l],
                kw["ligand_v_aux"][d_l], b_l, kw["prior_stds"][d_pr],
                kw["ligand_decomp_batch"].to(dev)[d_l] - old_pr0[b_l] + b_l * g.n_pr,
                kw["ligand_decomp_index"][d_l] if kw["ligand_decomp_index"] is not None else None, None, fc,
                kw["init_ligand_fc_bond_type"][d_b], kw["full_protein_pos"].to(dev)[g.rows_f.to(dev)] if has_full else None,
                BL.batch_vector(G, g.n_f, dev) if has_full else None,
                dataclasses.replace(call, seed=call.seed + 7919 * gi, drift_norm_batch=B),     # (the armsca loss is averaged over the whole batch)
                cache_slot=(g.ids[0] * split) // B,                # (sub-batches of one shape: own cached buffers each)
                place=place)                                       # (fixed / chain_init / noise / sample_keys: the group's share)
            prepared.append((chain, d_l, d_b, r_l, r_b))
        if concurrent is None:
            # measured on MI355X (tools/ragged_bench.py): with the runtime's default 4 hardware queues the
            # groups' graphs get in each other's way (0.7x); with GPU_MAX_HW_QUEUES=3 running them together gains 1.4x
            concurrent = os.environ.get("DD_RAGGED_CONCURRENT", "0") == "1"
        for cs in [[p[0] for p in prepared]] if concurrent else [[p[0]] for p in prepared]:
            self._run_chains(cs, n_pos, call.use_graph)
        for chain, d_l, d_b, r_l, r_b in prepared:
            r = self._collect_chain(chain, n_pos, keep_traj)
            out["pos"][d_l], out["v"][d_l], out["bond"][d_b] = r["pos"], r["v"], r["bond"]
            if keep_traj and n_pos > 0:
                for k, rows, n_tot in (("pos_traj", r_l, n_lig), ("v_traj", r_l, n_lig), ("v0_traj", r_l, n_lig),
                                       ("vt_traj", r_l, n_lig), ("bond_traj", r_b, n_bond), ("bt_traj", r_b, n_bond)):
                    st = torch.stack(r[k])                                         # [T, rows of this group, ...]
                    if traj[k] is None:
                        traj[k] = torch.empty((st.shape[0], n_tot) + tuple(st.shape[2:]), dtype=st.dtype)
                    traj[k][:, rows] = st
        for k in traj:
            out[k] = list(traj[k].unbind(0)) if traj[k] is not None else []
        if all(v is not None for v in traj.values()):
            out["_traj_stacked"] = dict(traj)
        if call.t_traj is not None:
            out["t_traj"] = call.t_traj.clone()
        self._restraint_results(call, [p[0] for p in prepared], out)
        return out

    # ------------------------------------------------------------------------------------------
    def _dense_inputs(self, protein_pos, protein_v, batch_protein, ligand_pos, ligand_v, ligand_v_aux, batch_ligand,
                      ligand_fc_bond_index, ligand_bond_type, ligand_atom_mask, layout=None, aux_onehot=None):
        """Flat PyG-style batch -> dense [B, ...] tensors (validated, no arithmetic).  ``layout`` = (B, NP, NL) already
        established for these very batch-vector / bond-list tensors by an earlier call: their checks are skipped."""
        for name, t in (("protein_pos", protein_pos), ("ligand_pos", ligand_pos)):
            hip_lib.require_gpu(t, name)
        _check_ligand_atom_mask(ligand_atom_mask, batch_ligand.numel())
        if ligand_fc_bond_index is None or ligand_bond_type is None:
            raise NotImplementedError("the uni_o2_bond path needs the fully connected ligand bond graph")
        if layout is not None:
            B = layout[0]
        else:
            B = int(batch_protein.max().item()) + 1 if batch_protein.numel() else 0
        if B <= 0:
            raise ValueError("empty batch")
        n_p, n_l = batch_protein.numel(), batch_ligand.numel()
        if n_p % B or n_l % B:
            raise NotImplementedError("ragged batches (different atom counts per sample) are not supported yet; "
                                      "batch samples of one pocket with equal ligand sizes")
        NP, NL = n_p // B, n_l // B
        dev = protein_pos.device
        if layout is None:
            exp_p, exp_l, exp_fc = self._expected_layout(B, NP, NL, dev)
            if not (torch.equal(batch_protein, exp_p) and torch.equal(batch_ligand, exp_l)):
                raise NotImplementedError("batch vectors must be sorted with equal counts per sample (PyG Batch order)")
        BL.check_size_limits(NP, NL)
        # the fused kernels use the closed-form fc layout of FeaturizeLigandBond('fc') (utils/transforms.py:331-337)
        if layout is None and (ligand_fc_bond_index.shape != exp_fc.shape or not torch.equal(ligand_fc_bond_index, exp_fc)):
            raise NotImplementedError("ligand_fc_bond_index must be the dst-major fully connected graph ('fc' mode)")
        if protein_v.dim() != 2 or protein_v.shape[1] != 29 or ligand_v_aux.dim() != 2 or ligand_v_aux.shape[1] != 2:
            raise ValueError("protein_v must be [n,29] and ligand_v_aux [n,2] (27 atom features + 2 arm indicators; "
                             "arm/scaffold indicator), as the sampling script builds them")
        if protein_pos.shape != (n_p, 3) or ligand_pos.shape != (n_l, 3) or protein_v.shape[0] != n_p \
                or ligand_v.shape != (n_l,) or ligand_v_aux.shape[0] != n_l:
            raise ValueError("per-atom tensors do not match the batch vectors")
        # class ids out of range: the reference's index_to_log_onehot asserts (transitions.py:66)
        # (aux_onehot: the arm / scaffold indicator rows are exactly (1,0) or (0,1) -- the layer-0 tables need that)
        vals = [ligand_v.min(), ligand_v.max(), ligand_bond_type.min().to(ligand_v.dtype), ligand_bond_type.max().to(ligand_v.dtype)]
        if aux_onehot is None:
            vals.append((((ligand_v_aux == 0) | (ligand_v_aux == 1)).all() & (ligand_v_aux.sum(-1) == 1).all()).to(ligand_v.dtype))
        res = torch.stack(vals).tolist()                                                                   # (one sync)
        lo_v, hi_v, lo_b, hi_b = res[:4]
        aux_ok = bool(res[4]) if aux_onehot is None else bool(aux_onehot)
        assert lo_v >= 0 and hi_v < self.num_classes, f"Error: {hi_v} >= {self.num_classes}"
        assert lo_b >= 0 and hi_b < self.num_bond_classes, f"Error: {hi_b} >= {self.num_bond_classes}"
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        return dict(B=B, NP=NP, NL=NL, aux_onehot=bool(aux_ok),
                    protein_pos=f32(protein_pos).view(B, NP, 3), protein_v=f32(protein_v).view(B, NP, -1),
                    ligand_pos=f32(ligand_pos).view(B, NL, 3), ligand_v=ligand_v.detach().to(torch.int32).contiguous(),
                    ligand_aux=f32(ligand_v_aux).view(B, NL, -1),
                    bond=ligand_bond_type.detach().to(torch.int32).contiguous())

    # ------------------------------------------------------------------------------------------
    # Chain resources.  Everything a chain keeps on the device (state, static inputs, workspace, trajectory buffers, the
    # dd_sampler struct) and its captured step graph are cached per shape: the start time and the Philox key live in
    # device memory (dd_sampler_reset), so a later chain of the same shape -- the next batch of a pocket, the next call of
    # the sampling script -- copies its inputs into the same buffers and replays the same graph instead of paying
    # allocation, 70 MB of memsets, stream capture and graph instantiation again (2.8 ms per call; the driver's
    # 20-step bench is 27 ms of GPU work).  Chains with injected noise (parity mode) are not cached.
    _CACHE_MAX = int(os.environ.get("DD_CHAIN_CACHE_SIZE", "4"))
    _graph_counter = 0
    _primed_devices: set = set()               # devices whose streamed-trajectory path has run once (_prime_streaming)
    # Step graphs of finished UNCACHED chains (injected noise: the parity tests) are parked, not destroyed one by one: the HIP
    # runtime of ROCm 7.2 crashed now and then (hipEventSynchronize / hipStreamBeginCapture, ~1 in 10 runs of the GPU suite) when a
    # single executable graph was destroyed while others stayed alive and another one was captured right after -- graphs only ever
    # go away all together, newest first (_drop_cached_graphs), here once _PARK_MAX of them have piled up.
    _parked_graphs: list = []
    _PARK_MAX = 12
    _chain_cache: Dict[tuple, dict] = {}      # process-wide (keys carry device and weight arena): ONE destruction order for all graphs

    def _evict_chain_cache(self, keep=0):
        """Drop the least recently used entries beyond `keep`.  Captured graphs are only ever destroyed newest-first and
        all together: destroying an OLDER executable graph while newer ones stay alive, then capturing another one, crashed
        inside hipGraphLaunch on ROCm 7.2 (reproducible in the GPU test suite); the surviving entries keep their buffers
        and re-capture their step graph on next use (0.4 ms)."""
        cache = getattr(self, "_chain_cache", None)
        if not cache or len(cache) <= keep:
            return
        self._drop_cached_graphs()
        while len(cache) > keep:
            cache.pop(next(iter(cache)))                  # oldest first (dicts keep insertion order)

    def _drop_cached_graphs(self):
        """Destroy every live step graph -- the cached entries' and the parked ones of finished uncached chains -- newest
        first and all together (see _evict_chain_cache); buffers stay cached."""
        cache = getattr(self, "_chain_cache", None) or {}
        live = [e for e in cache.values() if e.get("graph") is not None] + DecompScorePosNet3D._parked_graphs
        live = sorted(live, key=lambda e: -e.get("graph_id", 0))
        for d in {str(e["dev"]): e["dev"] for e in live}.values():     # the cache and the parked list are process-wide
            torch.cuda.synchronize(d)
        lib = hip_lib.load()
        for e in live:
            lib.dd_graph_destroy(e["graph"])
            e["graph"] = None
        DecompScorePosNet3D._parked_graphs = []

    # Validation / centring of the inputs that do not change between the calls of one sampling job (the pocket, the
    # batch vectors, the bond list).  A call that passes the SAME tensor objects with unchanged version counters reuses
    # the result of the previous call: layout checks (six device -> host syncs), the protein centroid (a device -> host
    # copy) and the centred protein block cost ~1 ms per call, 5 % of a 20-step call.  The entry holds references to
    # the tensors, so their memory cannot be recycled for other data while it is cached.
    def _static_memo_get(self, tensors, extra):
        m = self.__dict__.get("_static_memo")
        if m is None or m["extra"] != extra or len(m["tensors"]) != len(tensors):
            return None
        for t, (u, ver) in zip(tensors, m["tensors"]):
            if t is not u or (t is not None and t._version != ver):
                return None
        return m["value"]

    def _static_memo_put(self, tensors, extra, value):
        self.__dict__["_static_memo"] = dict(tensors=[(t, None if t is None else t._version) for t in tensors], extra=extra,
                                             value=value)

    def _expected_layout(self, B, NP, NL, dev):
        """PyG Batch vectors and the dst-major fully connected bond index of a dense batch (validated against the
        caller's tensors on every call; built once per shape)."""
        memo = self.__dict__.setdefault("_layout_memo", {})
        key = (B, NP, NL, str(dev))
        if key not in memo:
            if len(memo) > 16:
                memo.clear()
            memo[key] = BL.dense_vectors(B, NP, NL, dev)
        return memo[key]

    def _make_sampler(self, d, pw, call, rows, offset, masks=None, cache_slot=0):
        """The prepared chain (dd_sampler, its buffers, its cache entry) of one dense-layout batch ``d`` for the call record ``call``;
        ``rows``: the chain's per-row inputs (`_chain_rows`); ``masks``: the real counts of a padded batch."""
        n_pos = call.n_pos
        cacheable = call.noise is None and n_pos > 0 and self._CACHE_MAX > 0 and os.environ.get("DD_CHAIN_CACHE", "1") != "0"
        key, ent = self._chain_entry(d, pw, n_pos, call.keep_traj, cacheable, rows["decomp"] is not None,
                                     0 if rows["fpp"] is None else int(rows["fpp"].shape[1]), masks is not None, cache_slot,
                                     schedule=call.schedule)
        upload = self._upload_pocket(ent, d, pw, rows["fpp"], cacheable)
        self._upload_state(ent, d, rows["atom_std"], offset, rows["decomp"], masks)
        self._bind_call(ent, d, pw, rows["keys"], rows["fx"], call.resample, rows["ci"], rows["rs"], n_pos)
        use_l0 = self._fill_sampler(ent, d, pw, call.t_start, call.seed, rows["noise"],
                                    _drift_fields(call.drift, rows["decomp"] is not None), call.drift_norm_batch, upload)
        self._start_chain(ent, n_pos, rows["fx"], rows["ci"])
        # everything that shapes the captured step graph besides the (cached) pointers
        sm = ent["s"]
        ent["sig"] = (sm.drift_armsca, sm.armsca_min_d, sm.armsca_max_d, sm.armsca_scale, sm.drift_clash, sm.clash_sigma,
                      sm.clash_gamma, sm.clash_scale, sm.drift_repul, sm.repul_max_d, sm.repul_scale, sm.drift_norm_batch,
                      int(hip_lib.load().dd_debug_options_epoch()), use_l0, ent["keyed"], rows["fx"] is not None, ent["fixed"],
                      call.resample is not None, ent["restraint_sig"])
        if cacheable:
            DecompScorePosNet3D._chain_cache[key] = ent    # (re-inserted: most recently used last)
            self._evict_chain_cache(self._CACHE_MAX)
        return sm, ent["bufs"], ent

    def _chain_entry(self, d, pw, n_steps, keep_traj, cacheable, has_decomp=False, NF=0, masked=False, cache_slot=0, schedule=None):
        """(cache key, entry) of a chain of this shape: taken out of the cache (``cacheable``) or allocated, with the dd_sampler
        fields that never change.  ``n_steps``: trajectory positions of the chain.  ``schedule``: the schedule set whose tables the
        chain reads (None: ``pw`` itself, the module's own); its levels belong to the key -- a chain's graph carries the table
        pointers -- and the entry holds the set."""
        sch = pw if schedule is None else schedule
        lib = hip_lib.load()
        dev = d["protein_pos"].device
        B, NP, NL = d["B"], d["NP"], d["NL"]
        N = NP + NL
        K = min(int(self.config.knn), N - 1)
        Eb = NL * (NL - 1)
        arena, offs = pw["arena"], pw["offsets"]
        cap = n_steps
        if cacheable and keep_traj:
            # (traj_capacity_hint: a caller that knows the chain length of its later calls -- bench.py's warm-up calls are shorter than its
            #  timed call -- sizes the cached buffers for it, so that call meets the same chain entry and step graph)
            hint = int(getattr(self, "traj_capacity_hint", 0) or 0)
            cap = max(32, 1 << (max(int(n_steps), hint) - 1).bit_length())   # trajectory capacity: 5 and 20 steps share buffers
        key = (str(dev), B, NP, NL, K, NF, cap if keep_traj else 0, bool(keep_traj), has_decomp, arena.data_ptr(),
               masked, int(cache_slot), self.bond_net_type, self.x2h_out_fc, int(self.config.num_blocks),     # cache_slot: chains of ONE call that share a shape need separate buffers
               sch["levels"])
        ent = DecompScorePosNet3D._chain_cache.pop(key, None) if cacheable else None
        if ent is not None:
            return key, ent
        z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)
        bufs: Dict[str, Optional[torch.Tensor]] = {}
        # static inputs (own buffers: a cached graph points at them)
        bufs["protein_pos"], bufs["protein_h"] = z(B, NP, 3), z(B * NP, H)
        bufs["lig_aux"], bufs["atom_std"], bufs["offset"] = z(B, NL, 2), z(B * NL, 3), z(B, 3)
        bufs["decomp_index"] = z(B * NL, dtype=torch.int32) if has_decomp else None
        bufs["full_protein_pos"] = z(B, NF, 3) if NF else None
        # state
        bufs["lig_pos"], bufs["lig_v"], bufs["lig_bond"] = z(B, NL, 3), z(B * NL, dtype=torch.int32), z(B * Eb, dtype=torch.int32)
        bufs["step_counter"] = z(4, dtype=torch.int32)             # run state: steps done, t_start, seed lo / hi
        if masked:                                                 # padded heterogeneous batch (dd_sampler.np_real ...)
            bufs["np_real"], bufs["nl_real"] = z(B, dtype=torch.int32), z(B, dtype=torch.int32)
            bufs["bl_prefix"] = z(B + 1, dtype=torch.int32)
        bufs["pred_pos"], bufs["pred_v"], bufs["pred_bond"] = z(B * NL, 3), z(B * NL, self.num_classes), z(B * Eb, 5)
        ws_floats = int(lib.dd_workspace_floats(B, NP, NL, K))
        bufs["workspace"] = z(ws_floats)
        if not masked and self._layer0_tables(pw, dev) is not None:        # layer-0 tables (dd_sampler.l0_*)
            bufs["l0_P"], bufs["l0_qn"] = z(B * N, 640), z(B * N, 128)
        if keep_traj and n_steps > 0:
            bufs["traj_pos"] = z(cap, B * NL, 3)
            bufs["traj_v"] = z(cap, B * NL, dtype=torch.int32)
            bufs["traj_bond"] = z(cap, B * Eb, dtype=torch.int32)
            bufs["traj_v0"] = z(cap, B * NL, self.num_classes)
            bufs["traj_vt"] = z(cap, B * NL, self.num_classes)
            bufs["traj_bt"] = z(cap, B * Eb, 5)
        sm = hip_lib.DDSampler()
        sm.B, sm.NP, sm.NL, sm.K, sm.NF = B, NP, NL, K, NF
        sm.num_layers, sm.T = int(self.config.num_layers), sch["T"]
        sm.num_v = int(self.num_classes)
        sm.weights = arena.data_ptr()
        sm.slot_off = offs.ctypes.data
        sm.tab_pos, sm.tab_v, sm.tab_b = sch["tab_pos"].data_ptr(), sch["tab_v"].data_ptr(), sch["tab_b"].data_ptr()
        sm.tab_score = sch["tab_score"].data_ptr()
        sm.workspace_floats = ws_floats
        return key, dict(s=sm, bufs=bufs, graph=None, graph_sig=None, dev=dev, pw=pw, sch=sch)

    def _upload_pocket(self, ent, d, pw, full_protein_pos, cacheable):
        """The pocket side of a chain's inputs (protein coordinates / embedded features, arm indicators, full protein,
        layer-0 protein rows) is uploaded once per cached entry and pocket: a later call that passes the SAME tensor objects
        with unchanged version counters (the next batch of the pocket, the sampling script's loop) finds them in place --
        five launches less in front of the first graph replay.
        CONTRACT of the skip: it keys on the identity of the caller's tensors AND their version counters.  Writes that do not bump
        the counter (t.data.copy_, set_, another library writing through data_ptr) are invisible to it: after such a write call
        model.invalidate_pocket_uploads() or set DD_POCKET_UPLOAD_SKIP=0 (every call then uploads).  The cache entry holds
        references to those tensors for as long as it lives (evicted with the chain cache).
        Returns (src, pocket_in_place) for `_fill_sampler`, which records the upload once everything is enqueued."""
        bufs, B, NP = ent["bufs"], d["B"], d["NP"]
        src = d.get("upload_src") if (cacheable and os.environ.get("DD_POCKET_UPLOAD_SKIP", "1") != "0") else None
        pocket_in_place = (src is not None and ent.get("uploaded") is not None and ent.get("uploaded_pw") is pw
                           and ent.get("uploaded_mode") == d.get("upload_mode") and len(src) == len(ent["uploaded"])
                           and all(t is u and (t is None or t._version == ver) for t, (u, ver) in zip(src, ent["uploaded"])))
        ent["uploaded"] = None
        if not pocket_in_place:
            arena, goff = pw["arena"], self._global_offsets(pw)
            bufs["protein_pos"].copy_(d["protein_pos_centered"])
            hip_lib.check(hip_lib.load().dd_embed_protein(hip_lib.ptr(d["protein_v"].view(B * NP, -1)), B * NP,
                                                          ctypes.c_void_p(arena[goff["W_pemb"]:].data_ptr()),
                                                          ctypes.c_void_p(arena[goff["b_pemb"]:].data_ptr()),
                                                          hip_lib.ptr(bufs["protein_h"]), hip_lib.stream_ptr(ent["dev"])), "dd_embed_protein")
            bufs["lig_aux"].copy_(d["ligand_aux"])
            if full_protein_pos is not None:
                bufs["full_protein_pos"].copy_(full_protein_pos)
        return src, pocket_in_place

    @staticmethod
    def _upload_state(ent, d, atom_std, offset, decomp_index, masks):
        """This chain's ligand side: stds, offset, decomposition, first state and, padded batch, the real counts."""
        bufs = ent["bufs"]
        bufs["atom_std"].copy_(atom_std.reshape(-1, 3))
        bufs["offset"].copy_(offset)
        if decomp_index is not None:
            bufs["decomp_index"].copy_(decomp_index.reshape(-1))
        bufs["lig_pos"].copy_(d["ligand_pos_centered"])
        bufs["lig_v"].copy_(d["ligand_v"])
        bufs["lig_bond"].copy_(d["bond"])
        if masks is not None:
            for k in ("np_real", "nl_real", "bl_prefix"):
                bufs[k].copy_(masks[k])

    def _bind_call(self, ent, d, pw, keys, fixed, resample, chain_init, restraints=None, n_pos=0):
        """The per-call inputs that the kernels read through pointers at every launch -- per-sample noise keys, fixed atoms (fx_*),
        the resampling epoch, the chain init (ci_*): the buffers belong to the (cached) entry and are created when first needed,
        their contents to this call, so the entry's captured graph serves the next chain with other keys, masks and known values.
        ``keys``: int64 [B] (host or device) in the order of the chain's samples, or None (the chain draws with its seed); ``fixed`` /
        ``chain_init``: the ``fx`` / ``ci`` of `_chain_rows`; ``resample``: the validated dict of `_as_resample`; ``restraints``: the
        ``rs`` of `_chain_rows`; ``n_pos``: the chain's positions (the rows of the restraint trajectories).  Leaves on the entry ``keyed``, ``fixed`` (the mode), ``resample``, ``restraints``, the host structs,
        and ``launch``: the step-launch arguments of this chain."""
        bufs, dev = ent["bufs"], ent["dev"]
        sch = ent["sch"]                                    # (tab_fixed / tab_jump: composed from the chain's own schedule set)
        A, E = d["B"] * d["NL"], d["B"] * d["NL"] * (d["NL"] - 1)
        fx, ci = fixed or {}, chain_init or {}
        replace, noised = fx.get("mode") == "replace", ci.get("mode") == "noised"
        with_cc = fixed is not None and (replace or resample is not None)      # (a jump noises around the centres in hold mode too)
        i32, f32, bound = torch.int32, torch.float32, {}
        for name, src, shape, dtype, wanted in (
                ("sample_keys", keys, (d["B"],), torch.int64, keys is not None),
                ("fx_mask", fx.get("mask"), (A,), torch.uint8, fixed is not None), ("fx_v0", fx.get("v0"), (A,), i32, fixed is not None),
                ("fx_b0", fx.get("b0"), (E,), i32, fixed is not None), ("fx_x0c", fx.get("x0c"), (A, 3), f32, fixed is not None),
                ("fx_cc", fx.get("cc"), (A, 3), f32, with_cc),
                ("epoch", None, (1,), i32, resample is not None),          # (zeroed by dd_sampler_reset_resample: it starts with the chain)
                ("ci_cc", ci.get("cc"), (A, 3), f32, chain_init is not None), ("ci_std", ci.get("std"), (A, 3), f32, chain_init is not None),
                ("ci_lp_v", ci.get("atom_lp"), (self.num_classes,), f32, ci.get("atom_lp") is not None),
                ("ci_lp_b", ci.get("bond_lp"), (self.num_bond_classes,), f32, ci.get("bond_lp") is not None),
                ("ci_x0c", ci.get("x0c"), (A, 3), f32, ci.get("x0c") is not None), ("ci_v0", ci.get("v0"), (A,), i32, ci.get("v0") is not None),
                ("ci_b0", ci.get("b0"), (E,), i32, ci.get("b0") is not None)):
            if wanted and bufs.get(name) is None:
                bufs[name] = torch.zeros(shape, dtype=dtype, device=dev)
            if wanted and src is not None:
                bufs[name].copy_(src.reshape(shape))
            bound[name] = bufs[name] if wanted else None
        if (replace or noised) and sch.get("tab_fixed") is None:
            sch["tab_fixed"] = self.fixed_step_table(sch["tables"]).to(dev)
        ent["keyed"], ent["fixed"], ent["fixed_struct"] = keys is not None, fx.get("mode"), None
        if fixed is not None:
            ent["fixed_struct"] = hip_lib.fixed_struct(fx["mode"], bound["fx_mask"], bound["fx_v0"], bound["fx_b0"], bound["fx_x0c"],
                                                       bound["fx_cc"], sch["tab_fixed"] if replace else None)
        # resampling: the jump table belongs to the schedule set (one per jump length); neither j nor r reaches the captured graph
        ent["resample"], ent["resample_struct"] = None, None
        if resample is not None:
            tabs = sch.setdefault("tab_jump", {})
            if resample["j"] not in tabs:
                tabs[resample["j"]] = self.resample_jump_table(resample["j"], sch["tables"]).to(dev)
            ent["resample"] = dict(resample)
            ent["resample_struct"] = hip_lib.resample_struct(resample["j"], tabs[resample["j"]], bound["epoch"])
        # chain init: the launch is part of the chain's preparation (_start_chain), not of its captured graph
        ent["init_struct"] = None
        if chain_init is not None:
            ent["init_struct"] = hip_lib.init_struct(ci["mode"], bound["ci_cc"], bound["ci_std"], bound["ci_lp_v"], bound["ci_lp_b"],
                                                     bound["ci_x0c"], bound["ci_v0"], bound["ci_b0"], sch["tab_fixed"] if noised else None)
        # distance restraints: the arrays hold a CAPACITY of entries (a power of two, at least 8) that the captured graph's launch
        # carries as R; the call's R entries come first and weight-0 entries of the last sample fill the rest (they add nothing)
        ent["restraints"], ent["restraints_struct"], ent["restraint_sig"] = None, None, None
        if restraints is not None:
            rs, nB = restraints, d["B"]
            cap = max(8, 1 << max(rs["R"] - 1, 0).bit_length(), int(bufs["rs_weight"].numel()) if bufs.get("rs_weight") is not None else 0)
            if bufs.get("rs_weight") is None or int(bufs["rs_weight"].numel()) != cap:
                z = lambda *shape, dtype=f32: torch.zeros(*shape, dtype=dtype, device=dev)
                bufs.update(rs_ptr=z(nB + 1, dtype=i32), rs_point=z(cap, 3), rs_min_d=z(cap), rs_max_d=z(cap), rs_weight=z(cap),
                            rs_atom=z(cap, dtype=i32), rs_group=z(cap, dtype=i32), rs_dist=z(cap), rs_winner=z(cap, dtype=i32),
                            rs_grad=z(A, 3))
            pad = cap - rs["R"]
            ptr = rs["ptr"].clone()
            ptr[nB] = cap
            fill = lambda t, v: torch.cat([t.to(dev), torch.full((pad,) + tuple(t.shape[1:]), v, dtype=t.dtype, device=dev)])
            for name, t, v in (("rs_point", rs["point"], 0.0), ("rs_min_d", rs["min_d"], 0.0), ("rs_max_d", rs["max_d"], math.inf),
                               ("rs_weight", rs["weight"], 0.0), ("rs_atom", rs["atom"], -1), ("rs_group", rs["group"], RESTRAINT_ANY)):
                bufs[name].copy_(fill(t, v))
            bufs["rs_ptr"].copy_(ptr)
            # the general form (typed / pair / harmonic / trajectories): its arrays are laid out the same way and ALL handed over, so
            # that one graph serves any values; an entry without it hands none over and is served by the point kernel as before
            general, rows = {}, 0
            if rs["general"]:
                if bufs.get("rs_pair") is None or int(bufs["rs_pair"].numel()) != cap:
                    zi = lambda: torch.zeros(cap, dtype=i32, device=dev)
                    bufs.update(rs_cls=zi(), rs_cls2=zi(), rs_pair=zi(), rs_atom2=zi(), rs_group2=zi(), rs_form=zi(), rs_winner2=zi())
                as_bits = lambda m: torch.where(m >= 2 ** 31, m - 2 ** 32, m).to(i32)      # (a 32-bit mask in an int32 tensor)
                for name, t, v in (("rs_cls", as_bits(rs["cls"]), -1), ("rs_cls2", as_bits(rs["cls2"]), -1), ("rs_pair", rs["pair"].to(i32), 0),
                                   ("rs_atom2", rs["atom2"], -1), ("rs_group2", rs["group2"], hip_lib.RESTRAINT_NONE), ("rs_form", rs["form"], 0)):
                    bufs[name].copy_(fill(t, v))
                general = dict(cls=bufs["rs_cls"], cls2=bufs["rs_cls2"], pair=bufs["rs_pair"], atom2=bufs["rs_atom2"],
                               group2=bufs["rs_group2"], form=bufs["rs_form"])
                if rs["traj"]:
                    have = bufs.get("rs_dist_traj")
                    if have is None or int(have.shape[1]) != cap or int(have.shape[0]) < max(int(n_pos), 1):
                        rows = max(int(n_pos), 1)
                        bufs.update(rs_dist_traj=torch.zeros(rows, cap, dtype=f32, device=dev),
                                    rs_winner_traj=torch.zeros(rows, cap, dtype=i32, device=dev),
                                    rs_winner2_traj=torch.zeros(rows, cap, dtype=i32, device=dev))
                    rows = int(bufs["rs_dist_traj"].shape[0])
                    general.update(dist_traj=bufs["rs_dist_traj"], winner_traj=bufs["rs_winner_traj"], winner2_traj=bufs["rs_winner2_traj"])
            ent["restraints"] = rs
            ent["restraints_struct"] = hip_lib.restraints_struct(cap, *(bufs[k] for k in ("rs_ptr", "rs_point", "rs_min_d", "rs_max_d",
                                                                                        "rs_weight", "rs_atom", "rs_group")),
                                                                 rs["scale"], rs["t_min"], rs["t_max"], traj_positions=rows, **general)
            # (what the captured launch carries by value, and which kernel it is: "general" / the trajectory rows, 0 = none)
            ent["restraint_sig"] = (cap, rs["scale"], rs["t_min"], rs["t_max"], "general" if rs["general"] else "point", rows)
        ref = lambda st: None if st is None else ctypes.byref(st)
        ent["launch"] = dict(keys=hip_lib.ptr(bound["sample_keys"]), fixed=ref(ent["fixed_struct"]), resample=ref(ent["resample_struct"]),
                             restraints=ref(ent["restraints_struct"]))

    def _fill_sampler(self, ent, d, pw, t_start, seed, noise, drift_fields, drift_norm_batch, upload):
        """The per-call fields of the entry's dd_sampler -- injected noise, layer-0 tables, start time, seed, buffer pointers, drift
        terms -- and the protein rows of the layer-0 tables; ``upload``: what `_upload_pocket` returned.  Returns "uses the tables"."""
        sm, bufs, dev = ent["s"], ent["bufs"], ent["dev"]
        src, pocket_in_place = upload
        for k in ("u_v", "u_b", "eps"):
            bufs[k] = None if noise is None else noise[k].to(device=dev, dtype=torch.float32).contiguous()
        # layer-0 tables: only for arm / scaffold indicator rows that are exactly (1,0) or (0,1) (d["aux_onehot"])
        use_l0 = bufs.get("l0_P") is not None and bool(d.get("aux_onehot", False))
        sm.l0_tables = self._layer0_tables(pw, dev).data_ptr() if use_l0 else None
        sm.l0_P = bufs["l0_P"].data_ptr() if use_l0 else None
        sm.l0_qn = bufs["l0_qn"].data_ptr() if use_l0 else None
        sm.t_start = int(t_start)
        sm.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        for k in ("protein_pos", "protein_h", "lig_aux", "atom_std", "offset", "decomp_index", "full_protein_pos",
                  "lig_pos", "lig_v", "lig_bond", "step_counter", "u_v", "u_b", "eps", "traj_pos", "traj_v",
                  "traj_bond", "traj_v0", "traj_vt", "traj_bt", "pred_pos", "pred_v", "pred_bond", "workspace",
                  "np_real", "nl_real", "bl_prefix"):
            t = bufs.get(k)
            if t is not None:
                assert t.is_contiguous() and t.device == dev, k
            setattr(sm, k, t.data_ptr() if t is not None else None)
        for k, v in drift_fields.items():
            setattr(sm, k, v)
        sm.drift_norm_batch = int(drift_norm_batch)
        if use_l0 and not (pocket_in_place and ent.get("uploaded_l0")):     # protein rows of the layer-0 tables (this chain's pocket)
            hip_lib.check(hip_lib.load().dd_layer0_prepare(ctypes.byref(sm), hip_lib.stream_ptr(dev)), "dd_layer0_prepare")
        if src is not None:
            ent["uploaded"] = [(t, None if t is None else t._version) for t in src]
            ent["uploaded_pw"], ent["uploaded_l0"], ent["uploaded_mode"] = pw, bool(use_l0), d.get("upload_mode")
        return bool(use_l0)

    def _start_chain(self, ent, n_steps, fixed, chain_init):
        """The launches in front of a chain's first step: the reset of its run state, its first level and its held rows."""
        lib, sm, st, L = hip_lib.load(), ctypes.byref(ent["s"]), hip_lib.stream_ptr(ent["dev"]), ent["launch"]
        draw_level = fixed is not None and fixed["mode"] == "replace" and fixed["init"] == "draw"
        if L["resample"] is not None:                      # (the epoch starts with the chain)
            hip_lib.check(lib.dd_sampler_reset_resample(sm, L["resample"], st), "dd_sampler_reset_resample")
        elif n_steps > 0 or draw_level or chain_init is not None:      # (a chain of no steps still prepares its first level / held rows)
            hip_lib.check(lib.dd_sampler_reset(sm, st), "dd_sampler_reset")
        # the chain's first level drawn on the device (every real row), in front of the held rows' preparation
        if chain_init is not None:
            hip_lib.check(lib.dd_chain_init(sm, L["keys"], ctypes.byref(ent["init_struct"]), st), "dd_chain_init")
        # held rows in front of the first step: hold -- the known values; replace, init 'draw' -- level t_start at Philox time
        # t_start + 1 ('given': init_ligand_* already holds that level)
        if fixed is not None and (fixed["mode"] == "hold" or draw_level):
            hip_lib.check(lib.dd_fixed_init(sm, L["keys"], L["fixed"], st), "dd_fixed_init")

    def _run_forward(self, d, pw, masks=None):
        """One forward() call on the dense-layout batch ``d``: an entry of its own (never cached), pocket and ligand uploaded,
        the score network launched; the predictions over the dense [B*NL] / [B*Eb] rows."""
        dev = d["protein_pos"].device
        atom_std, offset = torch.ones(d["B"] * d["NL"], 3, device=dev), torch.zeros(d["B"], 3, device=dev)     # (not read by a forward)
        _, ent = self._chain_entry(d, pw, 0, False, False, masked=masks is not None)
        upload = self._upload_pocket(ent, d, pw, None, False)
        self._upload_state(ent, d, atom_std, offset, None, masks)
        self._fill_sampler(ent, d, pw, 0, 0, None, _drift_fields(None, False), 0, upload)
        hip_lib.check(hip_lib.load().dd_forward_opts(ctypes.byref(ent["s"]), self._model_opts(pw), hip_lib.stream_ptr(dev)), "dd_forward")
        _check_queue(ent["s"], dev)
        self._last, bufs = (ent["s"], ent["bufs"]), ent["bufs"]
        preds = {"pred_ligand_pos": bufs["pred_pos"], "pred_ligand_v": bufs["pred_v"]}     # ([B*NL,3], [B*NL,num_classes])
        if self.bond_diffusion:
            preds["pred_bond"] = bufs["pred_bond"]
        return preds

    def _side_stream(self, dev):
        st = getattr(self, "_stream", None)
        if st is None or st.device != dev:
            st = torch.cuda.Stream(device=dev)
            self._stream = st
        return st

    def _stream_pool(self, dev, n):
        pool = getattr(self, "_streams", None)
        if pool is None or (pool and pool[0].device != dev):
            pool = []
        while len(pool) < n:
            pool.append(torch.cuda.Stream(device=dev))
        self._streams = pool
        return pool[:n]

    def _global_offsets(self, pw):
        n = int(self.config.num_layers) * len(packing.LAYER_SLOTS)
        return {k: int(pw["offsets"][n + i]) for i, k in enumerate(packing.GLOBAL_SLOTS)}

    # ------------------------------------------------------------------------------------------
    def _forward_heterogeneous(self, protein_pos, protein_v, batch_protein, ligand_pos, ligand_v, ligand_v_aux, batch_ligand,
                               ligand_fc_bond_index, ligand_bond_type, ligand_atom_mask):
        """forward() on samples with different atom counts (the same two ways as `_sample_heterogeneous`): one padded
        dd_forward_ex with per-sample real counts, or one dense forward per group of equal sizes."""
        hip_lib.require_gpu(protein_pos, "protein_pos")
        hip_lib.require_gpu(ligand_pos, "init_ligand_pos")
        _check_ligand_atom_mask(ligand_atom_mask, batch_ligand.numel())
        if ligand_fc_bond_index is None or ligand_bond_type is None:
            raise NotImplementedError("the uni_o2_bond path needs the fully connected ligand bond graph")
        dev = protein_pos.device
        layout = BL.BatchLayout.from_batch(batch_protein, batch_ligand, ligand_fc_bond_index=ligand_fc_bond_index.to(dev),
                                           n_bonds=ligand_bond_type.numel())
        n_p, n_l = layout.n_p, layout.n_l
        BL.check_size_limits(n_p, n_l)
        if os.environ.get("DD_RAGGED_MODE", "padded") != "groups" and BL.fits_padded(layout, self.config.knn):
            pad = self._padded_inputs(protein_pos, protein_v, batch_protein, ligand_pos, ligand_v, ligand_v_aux, batch_ligand,
                                      ligand_fc_bond_index, ligand_bond_type, None, n_p, n_l, "none")
            preds = self._run_forward(pad["d"], self._packed_weights(), masks=pad["masks"])
            return {k: t.index_select(0, pad["d_b" if k == "pred_bond" else "d_l"]) for k, t in preds.items()}
        # one dense forward per group of equal (protein, ligand) sizes, rows put back in the caller's order
        out = {"pred_ligand_pos": torch.empty(sum(n_l), 3, device=dev), "pred_ligand_v": torch.empty(sum(n_l), self.num_classes, device=dev)}
        if self.bond_diffusion:
            out["pred_bond"] = torch.empty(sum(layout.n_b), 5, device=dev)
        for g in layout.size_groups():
            r_p, r_l, r_b = g.rows_p.to(dev), g.rows_l.to(dev), g.rows_b.to(dev)
            b_p, b_l, fc = self._expected_layout(len(g.ids), g.n_p, g.n_l, dev)
            r = self.forward(protein_pos[r_p], protein_v[r_p], b_p, None, ligand_pos[r_l], ligand_v[r_l], ligand_v_aux[r_l],
                             b_l, None, None, None, None, None, fc, ligand_bond_type[r_b])
            out["pred_ligand_pos"][r_l], out["pred_ligand_v"][r_l] = r["pred_ligand_pos"], r["pred_ligand_v"]
            if self.bond_diffusion:
                out["pred_bond"][r_b] = r["pred_bond"]
        return out

    def forward(self, protein_pos, protein_v, batch_protein, protein_group_idx,
                init_ligand_pos, init_ligand_v, init_ligand_v_aux, batch_ligand, ligand_group_idx,
                prior_centers, prior_stds, batch_prior, prior_group_idx,
                ligand_fc_bond_index, init_ligand_fc_bond_type,
                ligand_atom_mask=None, time_step=None, return_all=False):
        """Score network once (reference: models/decompdiff.py:213-351).  ``time_step``, the group
        indices and the prior tensors are accepted for signature compatibility; the shipped
        configuration never reads them (time_emb_dim=0, add_prior_node=False).

        A batch whose samples differ in size (a PyG ``Batch`` of different complexes; layout validated by
        ``batch_layout.BatchLayout.from_batch``) is accepted: it runs as ONE launch sequence over the batch padded to its
        largest pocket / ligand with the real counts in ``dd_sampler.np_real / nl_real / bl_prefix`` (the layer-0 tables,
        which need a dense batch, are off for that call), or -- ``DD_RAGGED_MODE=groups``, or ``batch_layout.fits_padded``
        says no -- as one dense call per group of equal sizes.  Either way the predictions cover the real atoms and
        bonds only, in the flat order of the inputs.  ``ligand_atom_mask``: None or an all-True mask, as in
        :meth:`sample_diffusion`."""
        if return_all:
            raise NotImplementedError("return_all (per-block intermediates) is a training-time option")
        with torch.no_grad():
            if self._is_ragged(batch_protein, batch_ligand):
                return self._forward_heterogeneous(protein_pos, protein_v, batch_protein, init_ligand_pos, init_ligand_v,
                                                   init_ligand_v_aux, batch_ligand, ligand_fc_bond_index,
                                                   init_ligand_fc_bond_type, ligand_atom_mask)
            d = self._dense_inputs(protein_pos, protein_v, batch_protein, init_ligand_pos, init_ligand_v,
                                   init_ligand_v_aux, batch_ligand, ligand_fc_bond_index, init_ligand_fc_bond_type,
                                   ligand_atom_mask)
            d["protein_pos_centered"], d["ligand_pos_centered"] = d["protein_pos"], d["ligand_pos"]
            return self._run_forward(d, self._packed_weights())

    def train(self, mode: bool = True):
        self.__dict__["_packed"] = None                     # parameters are about to change (or just did)
        return super().train(mode)

    def get_diffusion_loss(self, protein_pos, protein_v, batch_protein, protein_group_idx,
                           ligand_pos, ligand_v, ligand_v_aux, batch_ligand, ligand_group_idx,
                           prior_centers, prior_stds, prior_num_atoms, batch_prior, prior_group_idx,
                           ligand_decomp_batch, ligand_decomp_index,
                           ligand_fc_bond_index=None, ligand_fc_bond_type=None, batch_ligand_bond=None, ligand_atom_mask=None,
                           time_step=None):
        """Training / validation objective of the reference (models/decompdiff.py:419-550), same arguments and result keys.

        With autograd enabled the network runs through :mod:`decompdiff_amd.training` (torch dense layers + the HIP graph
        ops with analytic backward passes), so ``results['losses']`` can be back-propagated into all parameters.  Under
        ``torch.no_grad()`` (the reference's validation loop) the network output comes from the fused ``dd_forward``
        kernels instead.  The batch layout is validated on every call for both paths (`training.check_batch_layout`,
        i.e. `batch_layout.BatchLayout.from_batch`); samples of different sizes -- the reference's
        training batches -- run as one padded, masked dense pass by default (`training.network_padded`), and as one dense
        sub-batch per distinct size (`training.network_grouped`) with ``DD_TRAIN_PAD=0`` or when `batch_layout.fits_padded`
        says no."""
        from . import training
        _check_ligand_atom_mask(ligand_atom_mask, batch_ligand.numel())
        if ligand_fc_bond_index is None or ligand_fc_bond_type is None or batch_ligand_bond is None:
            raise NotImplementedError("the uni_o2_bond path needs the fully connected ligand bond graph")
        hip_lib.require_gpu(protein_pos, "protein_pos")
        grad = torch.is_grad_enabled()
        if grad:
            self.__dict__["_packed"] = None                 # an optimizer step will follow: never reuse a packed copy
            net = training.network
        else:
            def net(model, p_pos, p_v, b_p, x_t, v_t, aux, b_l, fc, b_t):
                return model.forward(p_pos, p_v, b_p, None, x_t, v_t, aux, b_l, None, None, None, None, None, fc, b_t)
        return training.diffusion_loss(self, protein_pos, protein_v, batch_protein, ligand_pos, ligand_v, ligand_v_aux,
                                       batch_ligand, prior_centers, prior_stds, prior_num_atoms, batch_prior,
                                       ligand_decomp_batch, ligand_fc_bond_index, ligand_fc_bond_type, batch_ligand_bond,
                                       time_step=time_step, network_fn=net)

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def sample_diffusion(self, protein_pos, protein_v, batch_protein, protein_group_idx,
                         init_ligand_pos, init_ligand_v, ligand_v_aux, batch_ligand, ligand_group_idx,
                         prior_centers, prior_stds, prior_num_atoms, batch_prior, prior_group_idx,
                         ligand_decomp_batch, ligand_decomp_index,
                         ligand_atom_mask=None,
                         ligand_fc_bond_index=None, init_ligand_fc_bond_type=None, batch_ligand_bond=None,
                         num_steps=None, center_pos_mode=None,
                         energy_drift_opt=None,
                         full_protein_pos=None, full_batch_protein=None,
                         noise=None, seed=None, keep_traj=True, use_graph=True, start_step=0, _drift_norm_batch=0,
                         sample_keys=None, fixed=None, resample=None, init=None, time_levels=None):
        """Reverse diffusion (reference: models/decompdiff.py:552-703), same arguments and return
        keys.  Extra keyword-only knobs (all optional, reference call sites never pass them):

        * ``noise``  dict(u_v [T,B*NL,8], u_b [T,B*Eb,5], eps [T,B*NL,3]) — pre-drawn noise in the
          reference's draw order (parity mode); ``None`` -> device Philox keyed by ``seed``.
        * ``seed``   key of the device Philox streams.  ``None`` (what the reference's script gets, it passes no
          seed): a fresh 64-bit key is drawn from torch's global CPU generator on every call, so successive calls
          see independent noise and ``torch.manual_seed`` / the script's ``seed_all`` govern the chain exactly as
          they govern the reference's ``torch.randn_like`` draws (decompdiff.py:620,633,680).
        * ``start_step`` — resume a chain: the state passed in is x_t / v_t / b_t after ``start_step`` reverse steps,
          i.e. the first step runs at t = num_timesteps - 1 - start_step (``noise`` then holds the draws of the
          remaining ``num_steps`` steps only).
        * ``sample_keys`` — one 64-bit noise key per sample (a length-B int64 tensor, or a sequence of ints in [0, 2**64);
          see :func:`sample_keys`): sample b then receives exactly the draws that a call on that sample alone with
          ``seed=sample_keys[b]`` receives, whatever batch it sits in -- dense, padded or grouped, at any position, with
          any B -- so its chain is reproducible bit for bit under re-batching, sharding and re-ordering.  Excludes
          ``noise`` and an explicit ``seed`` (ValueError).
        * ``fixed`` — conditional generation (EXTENSION; the reference's ``ligand_atom_mask`` hook, decompdiff.py:597,621-622,
          682-683, cannot run): ``dict(mask bool [n_ligand], pos [n,3], v [n], bond [n_bond], mode="hold" | "replace", init=...)``
          in the caller's row order.  ``mask`` True = the atom is held at the known ``pos`` / ``v``; a bond is held at ``bond``
          iff both its endpoints are.  The network and the drift terms see the whole ligand; free rows step exactly as without
          ``fixed`` with the same draws, and ``v0_traj`` / ``vt_traj`` / ``bt_traj`` stay the network's and the posterior's for
          every row.  ``hold``: the held rows keep the known values through every step (reported coordinates:
          ``(known - offset) + offset`` in fp32).  ``replace`` (RePaint): the step at time t leaves the held rows at a fresh
          forward-process sample of their clean values at level t - 1, drawn with the row's own draws of that step, and the
          step at t = 0 leaves the clean values; ``init="draw"`` (default without ``noise`` and with ``start_step == 0``) draws
          their level ``t_start`` on the device first, ``init="given"`` (required with ``noise`` / ``start_step > 0``) takes the
          held rows of ``init_ligand_*`` as that level.  ``replace`` needs ``prior_centers``.  Bad shapes, dtypes, modes or
          classes raise ValueError; so does a ``ligand_atom_mask`` that masks atoms out.
        * ``resample`` — RePaint's resampling ("jump-back") schedule, valid only together with ``fixed`` and without ``noise``:
          ``dict(jump_length=j, n_resample=r)``.  After every j reverse steps (jump points anchored at the call's last level) the
          WHOLE ligand is diffused forward again by j levels on the device and denoised once more, r passes in all
          (:func:`resample_schedule` is the contract: ``num_steps + (r - 1) * j * (num_steps // j)`` reverse steps).  In ``replace``
          mode a jump moves every row, in ``hold`` mode the held atoms and the bonds between them keep their bits; both modes
          need ``prior_centers``.  A revisited time draws afresh (its Philox time word carries the number of jumps done), with the
          addressing of ``seed`` / ``sample_keys`` unchanged, so a keyed sample's chain stays independent of its batch.  The
          trajectories have one entry per reverse step ("position"; jumped states are not recorded) and the result gains
          ``t_traj``, the int64 times of the positions.  The schedule belongs to the call's range: with ``start_step`` / a
          shorter ``num_steps`` a split chain is NOT the unsplit one.  ``r = 1`` or ``j > num_steps``: bit for bit the call
          without ``resample``.  Wrong keys or types, ``j < 1``, ``r < 1``, no ``fixed``, ``noise=``: ValueError.
        * ``init`` — draw the chain's FIRST state on the device (dd_chain_init) instead of taking it from ``init_ligand_*``, which must
          then be ``None`` (ValueError otherwise; shapes come from ``batch_ligand`` / ``ligand_fc_bond_index`` /
          ``ligand_decomp_batch``).  The draws use the chain's own Philox addressing -- ``seed`` and the flat row, or
          ``sample_keys`` and the row of the sample's own enumeration -- on streams of their own (5 / 6 / 9), so with
          ``sample_keys`` a sample's starting point is as independent of its batch as its chain: nothing of the sample depends
          on the batching any more.  ``dict(mode="prior", centers=None, stds=None, atom_prior=None, bond_prior=None)``:
          coordinates ``centre + e * std`` around the per-atom gather of ``centers`` / ``stds`` [n_prior,3] through
          ``ligand_decomp_batch`` (default ``prior_centers`` / ``prior_stds``; arguments of their own because the reference's
          subpocket / stat modes draw the first coordinates around other centres than the chain uses), classes from the
          probability vectors ``atom_prior`` / ``bond_prior`` (default: the model's transition priors; uniform: the reference's
          ``log_sample_categorical(zeros)``); needs ``start_step == 0``.  ``dict(mode="noised", pos, v, bond[, centers, stds,
          atom_prior, bond_prior])`` -- partial diffusion: a KNOWN ligand in the caller's row order is noised by the forward
          process to level ``num_timesteps - 1 - start_step``, the level the first step expects, and denoised from there; needs
          ``prior_centers``.  Both exclude ``noise=``.  Composes with ``seed``, ``sample_keys``, ``fixed`` (the held rows are then
          prepared as always, after the draw; ``fixed['init'] = 'given'`` keeps the drawn level at the held rows), ``resample``,
          the drift terms, ``use_graph`` and every batch path; a call with ``num_steps=0`` returns the drawn state.  Bad modes,
          keys, shapes, dtypes, classes or combinations raise ValueError before anything is launched.  ``None``: today's call.
        * ``energy_drift_opt`` may list, once, a fourth term with the caller's own geometry (EXTENSION):
          ``dict(type="restraint", sample=[R], point=[R,3], min_d=, max_d=, weight=1.0, atom=None|[R], group=None|[R], scale=False,
          t_min=None, t_max=None)`` -- restraint r asks that an atom of sample ``sample[r]`` stays ``min_d .. max_d`` (scalars or
          [R]; ``min_d`` may be 0, ``max_d`` +inf) from ``point[r]`` (the frame of ``protein_pos``): the ligand atom ``atom[r]`` (a
          flat row of the caller's order), or, where ``atom[r] == -1`` (``atom=None``: everywhere), the nearest member of
          ``group[r]`` -- ``RESTRAINT_ANY`` (default: every atom of the sample), -1 (scaffold) or an arm id.  Energy
          ``sum_r weight_r (relu(min_d_r - d_r) + relu(d_r - max_d_r))`` with no division by B or R, so a sample's gradient does
          not depend on its batch; the step subtracts its gradient at x_t (times ``pos_score_coef[t]`` with ``scale``) next to the
          other terms while ``t_min <= t <= t_max`` (default: always).  Composes with every batch path, ``sample_keys``, ``fixed``
          (held atoms count as targets), ``resample``, ``init``, ``start_step`` and ``use_graph``; R = 0 is legal.  The result
          gains ``restraint_dist`` [R] and ``restraint_atom`` [R] (the flat row of the atom that counts, or -1: an empty group)
          of the final state.  Bad keys, shapes, dtypes, non-finite values, ``min_d > max_d``, an ``atom`` of another sample, a
          scaffold / arm group without ``ligand_decomp_index``, the term listed twice: ValueError before anything is launched.
          Optional keys of the same entry (the general form; an entry without them runs the point kernel, bit for bit as before):
          ``classes`` / ``classes2`` -- None, a bool tensor [R, num_classes], or R entries of None | class ids: the endpoint's
          candidates are those whose CURRENT atom class (the chain's ``v_t``) is in the set, an explicit atom included;
          ``atom2`` / ``group2`` -- as ``atom`` / ``group``: restraint r is a PAIR restraint iff ``atom2[r] >= 0`` or ``group2[r]``
          is given (``RESTRAINT_NONE`` or None in a list: no second endpoint), its distance that of the nearest pair (i, j), i != j,
          of the two candidate sets (first in (i, j) order), the gradient +c u on i and -c u on j; ``point`` may then be None;
          ``form`` -- ``"linear"`` (default) | ``"harmonic"`` (``weight (relu(min_d - d)^2 + relu(d - max_d)^2)``), or R of them;
          ``traj=True`` -- the result gains ``restraint_dist_traj`` [n_pos, R] and ``restraint_atom_traj`` [n_pos, R] (with pairs
          also ``restraint_atom2_traj``): entry p holds the distance and winner(s) at the state (x_t, v_t) that the step of
          position p took its gradient from, window open or not, whatever ``keep_traj`` says.  With pairs the result gains
          ``restraint_atom2`` [R] (-1 for a point restraint or an empty pair).  Class ids outside ``[0, num_classes)``, an empty
          class set, ``atom2`` of another sample or equal to ``atom``, a pair without a second endpoint, an arm / scaffold
          ``group2`` without ``ligand_decomp_index``, an unknown ``form``, a non-bool ``traj``: ValueError.
        * ``time_levels`` — strided sampling (EXTENSION): a strictly decreasing sequence, numpy array or 1-D
          integer tensor of S >= 2 time levels in ``[0, num_timesteps - 1]``, in execution order (:func:`stride_levels` makes an
          evenly spaced one).  The chain then runs over these levels only, as the chain of a model whose schedule is the respaced
          one with S timesteps (``alphas_cumprod'[tau] = alphas_cumprod[level tau]``, betas recomputed; the categorical schedules
          likewise; composed in float64 from the config's schedule): the network takes no time input and the step kernels take time
          through their tables only, so every kernel serves it unchanged.  ``num_steps`` defaults to S; ``start_step`` and
          ``num_steps`` count POSITIONS of the list (``start_step + num_steps <= S``), position p runs at level
          ``time_levels[start_step + p]``, and a split chain equals the unsplit one.  The list's last position lands on the clean
          sample as the reference's t = 0 step does (no noise), whether or not its level is 0.  The Philox time word of a position
          is its VIRTUAL level ``tau = S - 1 - position`` (of the whole list), not the real level.  Everything that counts steps
          counts positions: ``noise`` holds ``[num_steps, ...]`` draws, ``resample``'s ``jump_length`` is in positions.  Real time
          enters in two places, both mapped on the host: a restraint's ``t_min`` / ``t_max`` stay REAL levels (the term acts at the
          positions whose real level lies in the window; none: the term never acts, distances are still reported), and
          ``init=dict(mode="noised")`` noises to the real level ``time_levels[start_step]``.  The result gains ``t_traj``, the int64
          real levels of the positions (with ``resample``: of the schedule's positions).  Bools, non-ints, a level twice, a list
          that does not decrease, levels out of range, S < 2, ``start_step + num_steps > S``: ValueError before anything is
          launched.  ``None``: today's call.
        * ``keep_traj`` — record the six trajectories on the device and copy them once at the end.
        * ``use_graph`` — replay one captured hipGraph per step instead of eager launches.
        """
        if self.model_mean_type not in ("C0", "noise"):          # ('noise': folded into tab_pos, position_step_table)
            raise ValueError(self.model_mean_type)
        levels, T = None, self.num_timesteps            # T: the timesteps of the schedule the chain runs on
        if time_levels is not None:
            levels = _as_time_levels(time_levels, self.num_timesteps)
            T = int(levels.numel())
            if num_steps is not None and (int(start_step) < 0 or int(num_steps) + int(start_step) > T):
                raise ValueError("num_steps (+ start_step) exceeds the positions of time_levels")
        if num_steps is None:
            num_steps = T
        if sample_keys is not None:
            if noise is not None or seed is not None:
                raise ValueError("sample_keys excludes noise= and an explicit seed=: a chain draws from one source")
            sample_keys = _as_sample_keys(sample_keys, batch_ligand)
            seed = 0                                             # (not read by a keyed chain; no draw from torch's generator)
        if resample is not None:
            resample = _as_resample(resample, fixed, noise, T, num_steps, start_step)
        if init is not None:
            dev = protein_pos.device
            init = _as_init(init, batch_ligand, ligand_fc_bond_index, ligand_decomp_batch, prior_centers, prior_stds,
                            (init_ligand_pos, init_ligand_v, init_ligand_fc_bond_type), noise, start_step, T,
                            self.num_classes, self.num_bond_classes, dev)
            # placeholders of the right shapes: the launch of dd_chain_init overwrites every real row before anything reads it
            init_ligand_pos = torch.zeros(batch_ligand.numel(), 3, device=dev)
            init_ligand_v = torch.zeros(batch_ligand.numel(), dtype=torch.long, device=dev)
            init_ligand_fc_bond_type = torch.zeros(int(ligand_fc_bond_index.shape[1]), dtype=torch.long, device=dev)
        if fixed is not None:
            fixed = _as_fixed(fixed, batch_ligand.numel(), ligand_fc_bond_index, init_ligand_fc_bond_type, self.num_classes,
                              self.num_bond_classes, noise, start_step, prior_centers, ligand_decomp_batch, ligand_atom_mask,
                              protein_pos.device, need_cc=resample is not None)
        energy_drift_opt, restraints = _split_restraints(energy_drift_opt)
        if restraints is not None:
            restraints = _as_restraints(restraints, batch_ligand, ligand_decomp_index, self.num_timesteps, self.num_classes)
            if levels is not None:                           # (the window: real levels -> the virtual range; none: weights of 0, the
                window = _virtual_window(levels, restraints["t_min"], restraints["t_max"])     # term adds exact zeros as a closed window does)
                if window is None:
                    restraints = dict(restraints, weight=torch.zeros_like(restraints["weight"]), t_min=0, t_max=T - 1)
                else:
                    restraints = dict(restraints, t_min=window[0], t_max=window[1])
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        key_t = (protein_pos, batch_protein, batch_ligand, ligand_fc_bond_index, ligand_v_aux)
        static = self._static_memo_get(key_t, center_pos_mode)        # (only dense batches are remembered)
        call = _Call(T, num_steps, start_step, center_pos_mode, energy_drift_opt, noise, seed, keep_traj, use_graph,
                     _drift_norm_batch, sample_keys, fixed, resample, init, restraints,
                     None if levels is None else self._schedule_set(self._packed_weights(), tuple(levels.tolist())), levels)
        if static is None and self._is_ragged(batch_protein, batch_ligand):
            return self._sample_heterogeneous(
                dict(protein_pos=protein_pos, protein_v=protein_v, batch_protein=batch_protein, init_ligand_pos=init_ligand_pos,
                     init_ligand_v=init_ligand_v, ligand_v_aux=ligand_v_aux, batch_ligand=batch_ligand, prior_stds=prior_stds,
                     batch_prior=batch_prior, ligand_decomp_batch=ligand_decomp_batch, ligand_decomp_index=ligand_decomp_index,
                     ligand_fc_bond_index=ligand_fc_bond_index, init_ligand_fc_bond_type=init_ligand_fc_bond_type,
                     batch_ligand_bond=batch_ligand_bond, full_protein_pos=full_protein_pos, full_batch_protein=full_batch_protein,
                     ligand_atom_mask=ligand_atom_mask), call)
        chain = self._prepare_chain(protein_pos, protein_v, batch_protein, init_ligand_pos, init_ligand_v, ligand_v_aux,
                                    batch_ligand, prior_stds, ligand_decomp_batch, ligand_decomp_index, ligand_atom_mask,
                                    ligand_fc_bond_index, init_ligand_fc_bond_type, full_protein_pos, full_batch_protein, call,
                                    static=static)
        if static is None and "static" in chain:
            self._static_memo_put(key_t, center_pos_mode, chain["static"])
        tr = self.__dict__.get("_trace")
        if tr is not None:
            tr.append(("prepared>", time.perf_counter()))
        self._run_chains([chain], call.n_pos, use_graph)
        out = self._collect_chain(chain, call.n_pos, keep_traj)
        self._restraint_results(call, [chain], out)
        if tr is not None:
            tr.append(("collected>", time.perf_counter()))
        self._last = (chain["s"], chain["bufs"])
        return out

    def _prepare_chain(self, protein_pos, protein_v, batch_protein, init_ligand_pos, init_ligand_v, ligand_v_aux,
                       batch_ligand, prior_stds, ligand_decomp_batch, ligand_decomp_index, ligand_atom_mask,
                       ligand_fc_bond_index, init_ligand_fc_bond_type, full_protein_pos, full_batch_protein, call,
                       static=None, cache_slot=0, place=None):
        """Validate one dense batch, centre it, allocate its state / workspace and fill the ``dd_sampler`` struct for the call
        record ``call``.  ``static``: what an earlier call with the same pocket / batch-vector tensors established
        (_static_memo_get).  ``place``: which of the call's rows are this chain's (a group of a ragged batch; None: all)."""
        d = self._dense_inputs(protein_pos, protein_v, batch_protein, init_ligand_pos, init_ligand_v, ligand_v_aux,
                               batch_ligand, ligand_fc_bond_index, init_ligand_fc_bond_type, ligand_atom_mask,
                               layout=None if static is None else static["layout"],
                               aux_onehot=None if static is None else static["aux_onehot"])
        dev = d["protein_pos"].device
        B, NP, NL = d["B"], d["NP"], d["NL"]
        # center_pos (decompdiff.py:20-32): subtract the per-sample protein centroid
        if static is not None:
            offset = static["offset"]
        elif call.center_pos_mode == "protein":
            # scatter_mean(protein_pos, batch_protein, dim=0) (decompdiff.py:25): fp32 accumulation in row order / count --
            # the same arithmetic as the CPU scatter, on the host (B*NP*3 floats), so the offset that is re-added to
            # every output is bit-identical to the reference's
            pp = d["protein_pos"].detach().cpu().reshape(B * NP, 3)
            tot = torch.zeros(B, 3).index_add_(0, torch.arange(B).repeat_interleave(NP), pp)
            offset = (tot / float(max(NP, 1))).to(dev)
        elif call.center_pos_mode == "none":
            offset = torch.zeros(B, 3, device=dev)
        else:
            raise NotImplementedError(call.center_pos_mode)
        d["protein_pos_centered"] = static["protein_pos_centered"] if static is not None else \
            (d["protein_pos"] - offset[:, None, :]).contiguous()
        d["ligand_pos_centered"] = (d["ligand_pos"] - offset[:, None, :]).contiguous()
        rows = _chain_rows(call, place or _Placement(batch_ligand, d["bond"].numel()), offset, prior_stds, ligand_decomp_batch,
                           ligand_decomp_index, self.num_classes, (full_protein_pos, full_batch_protein))
        pw = self._packed_weights()
        # (what the pocket-side device buffers of a cached entry were filled from: _upload_pocket skips the upload if these very
        #  tensors come again unchanged; the centring mode shapes protein_pos_centered / offset)
        d["upload_src"] = (protein_pos, protein_v, ligand_v_aux, full_protein_pos, full_batch_protein) \
            if call.center_pos_mode in ("protein", "none") else None
        d["upload_mode"] = call.center_pos_mode
        s, bufs, ent = self._make_sampler(d, pw, call, rows, offset.contiguous(), cache_slot=cache_slot)
        return dict(s=s, bufs=bufs, offset=offset, B=B, NL=NL, dev=dev, ent=ent,
                    t_traj=call.t_traj,
                    static=dict(layout=(B, NP, NL), offset=offset, protein_pos_centered=d["protein_pos_centered"],
                                aux_onehot=d["aux_onehot"]))

    @staticmethod
    def _chain_runs(chain, num_steps):
        """[(reverse steps, followed by a jump)] of a prepared chain: the resampling schedule's runs, or one run of ``num_steps``."""
        rs = chain["ent"].get("resample")
        return rs["runs"] if rs else ([(int(num_steps), False)] if num_steps > 0 else [])

    @staticmethod
    def _pieces(runs, piece):
        """The streamed chain's pieces [(lo, hi, ops)]: positions [lo, hi) of the trajectories and the launches that fill them --
        replay counts and "jump" -- in order.  Pieces hold at most ``piece`` positions and end on run boundaries (a run that fits no
        piece is cut), and a jump goes with the run in front of it.  One run without a jump: the plain chain's equal pieces."""
        pieces, ops, lo, hi = [], [], 0, 0
        for n, jump in runs:
            if hi > lo and hi - lo + n > piece:
                pieces.append((lo, hi, ops))
                ops, lo = [], hi
            while n > piece:
                pieces.append((lo, lo + piece, [piece]))
                lo = hi = lo + piece
                n -= piece
            if n:
                ops.append(n)
                hi += n
            if jump:
                ops.append("jump")
            if hi - lo >= piece:
                pieces.append((lo, hi, ops))
                ops, lo = [], hi
        if hi > lo or ops:
            pieces.append((lo, hi, ops))
        return pieces

    def _jump(self, chain, stream):
        """Enqueue the forward jump of a resampled chain (and the rebase of its run state) on ``stream`` (a raw handle)."""
        L = chain["ent"]["launch"]
        hip_lib.check(hip_lib.load().dd_resample_jump(ctypes.byref(chain["s"]), L["keys"], L["fixed"], L["resample"], stream),
                      "dd_resample_jump")

    # Step-graph lifetime (see _parked_graphs, _evict_chain_cache): the one place that creates, numbers and parks an entry's graph.
    @staticmethod
    def _is_cached(ent):
        return any(e is ent for e in DecompScorePosNet3D._chain_cache.values())

    def _ensure_step_graph(self, chain, steps_per_graph, stream):
        """The entry's step graph for (its signature, ``steps_per_graph``, ``stream`` -- a raw handle): kept, or captured (again)."""
        cls, ent = DecompScorePosNet3D, chain["ent"]
        gsig = (ent["sig"], steps_per_graph, stream)
        if ent.get("graph") is not None and ent["graph_sig"] != gsig:      # launch structure changed: capture again
            self._drop_cached_graphs()
        if ent.get("graph") is None:
            if len(cls._parked_graphs) >= cls._PARK_MAX:
                self._drop_cached_graphs()                 # (all live graphs, newest first; cached entries re-capture on next use)
            ent["graph"], ent["graph_sig"] = self._create_step_graph(chain, steps_per_graph, stream), gsig
            cls._graph_counter += 1
            ent["graph_id"] = cls._graph_counter
        return ent["graph"]

    @staticmethod
    def _release_step_graph(ent, cached):
        """After the run (the streams are idle): a cached entry keeps its graph for the next chain, any other graph is parked."""
        if not cached:
            DecompScorePosNet3D._parked_graphs.append({"graph": ent["graph"], "graph_id": ent["graph_id"], "dev": ent["dev"]})
            ent["graph"] = None

    def _run_chains(self, chains, num_steps, use_graph):
        """Advance every prepared chain by ``num_steps`` (resampled chains: positions -- every chain of a call shares the schedule;
        the runs of graph replays or eager steps alternate with jump launches on the chain's stream).  One chain: the captured step graph replayed on a dedicated
        stream (the legacy default stream cannot be captured).  Several chains (the equal-size groups of a ragged batch):
        one graph and one stream each, replayed round-robin so the groups overlap on the GPU."""
        lib = hip_lib.load()
        dev = chains[0]["dev"]
        cur = torch.cuda.current_stream(dev)
        if (len(chains) == 1 and use_graph and num_steps > 0 and "traj_pos" in chains[0]["bufs"]
                and os.environ.get("DD_TRAJ_STREAMING", "1") != "0"):
            return self._run_chain_streaming(chains[0], num_steps)
        if len(chains) == 1 or not use_graph:
            side = self._side_stream(dev)
            side.wait_stream(cur)
            if use_graph and num_steps > 0:
                # (not dd_sample_steps_graph: that entry point creates AND destroys its graph per call -- see _parked_graphs)
                for c in chains:
                    cached = self._is_cached(c["ent"])
                    graph = self._ensure_step_graph(c, 1, side.cuda_stream)
                    try:
                        for n, jump in self._chain_runs(c, num_steps):
                            hip_lib.check(lib.dd_graph_launch(graph, int(n), side.cuda_stream), "dd_graph_launch")
                            if jump:
                                self._jump(c, side.cuda_stream)
                    finally:
                        side.synchronize()
                        self._release_step_graph(c["ent"], cached)
            else:
                # (dd_sample_steps_guided with NULL keys / fixed / resample / restraints IS dd_sample_steps_opts: in dd_api.hip the
                #  whole suffix chain only delegates to it)
                with torch.cuda.stream(side):
                    for c in chains:
                        L, sm, st = c["ent"]["launch"], ctypes.byref(c["s"]), hip_lib.stream_ptr(dev)
                        for n, jump in self._chain_runs(c, num_steps):
                            hip_lib.check(self._step_entry(lib, "dd_sample_steps", L)(sm, self._model_opts(), *self._step_extras(lib, L),
                                                                                       int(n), st), "dd_sample_steps_guided")
                            if jump:
                                self._jump(c, st)
            cur.wait_stream(side)
            return
        if len(chains) > 64:                            # dd_sample_steps_graph_multi takes at most 64 chains
            self._run_chains(chains[:64], num_steps, use_graph)
            self._run_chains(chains[64:], num_steps, use_graph)
            return
        pool = self._stream_pool(dev, len(chains))
        for st in pool:
            st.wait_stream(cur)
        n = len(chains)
        if any(c["ent"].get("keyed") or c["ent"].get("fixed") or c["ent"].get("restraints") for c in chains):
            # keyed chains, chains with fixed atoms or restraints: dd_sample_steps_graph_multi_* takes none of them -- one step graph per chain on its own stream, replayed
            # round-robin from this thread; no other graph is alive across their creation and they go away newest first and all
            # together (see _parked_graphs)
            self._drop_cached_graphs()
            graphs = []
            try:
                for c, st in zip(chains, pool):
                    graphs.append(self._create_step_graph(c, 1, st.cuda_stream))
                for n, jump in self._chain_runs(chains[0], num_steps):      # (one call: every chain has the same runs)
                    for _ in range(int(n)):
                        for g, st in zip(graphs, pool):
                            hip_lib.check(lib.dd_graph_launch(g, 1, st.cuda_stream), "dd_graph_launch")
                    if jump:
                        for c, st in zip(chains, pool):
                            self._jump(c, st.cuda_stream)
            finally:
                for st in pool:
                    st.synchronize()
                for g in reversed(graphs):
                    lib.dd_graph_destroy(g)
            for st in pool:
                cur.wait_stream(st)
            return
        ss = (ctypes.POINTER(hip_lib.DDSampler) * n)(*[ctypes.pointer(c["s"]) for c in chains])
        sts = (ctypes.c_void_p * n)(*[st.cuda_stream for st in pool])
        # (the C entry point captures one graph per chain and destroys them at the end: no other graph may be alive across
        #  that, see _parked_graphs -- cached entries re-capture theirs on next use)
        self._drop_cached_graphs()
        opts = (ctypes.POINTER(hip_lib.DDModelOpts) * n)(*([self._model_opts()] * n))
        hip_lib.check(lib.dd_sample_steps_graph_multi_opts(ss, opts, n, int(num_steps), sts), "dd_sample_steps_graph_multi")
        for st in pool:
            cur.wait_stream(st)

    @staticmethod
    def _step_entry(lib, stem, L):
        """``stem`` + "_guided", the one step pair this file calls.  A build from before that pair, loaded with DD_IGNORE_ABI=1 by the
        A/B tools (tools/ab_builds.py), serves chains without restraints through the pair it forwards from."""
        if hasattr(lib, stem + "_guided") or L["restraints"] is not None:
            return getattr(lib, stem + "_guided")
        return getattr(lib, stem + ("_resample" if L["resample"] is not None else "_fixed"))

    @staticmethod
    def _step_extras(lib, L):
        """The NULL-able arguments between ``opts`` and the step count of the entry point `_step_entry` chose."""
        if hasattr(lib, "dd_graph_create_guided") or L["restraints"] is not None:
            return L["keys"], L["fixed"], L["resample"], L["restraints"]
        return (L["keys"], L["fixed"]) + ((L["resample"],) if L["resample"] is not None else ())

    def _create_step_graph(self, chain, steps_per_graph, stream):
        """Capture ``steps_per_graph`` reverse steps of a prepared chain on ``stream`` (a raw stream handle) into a new step graph;
        a keyed chain's kernels read the keys from the entry's own buffer."""
        lib, L, graph = hip_lib.load(), chain["ent"]["launch"], ctypes.c_void_p()
        args = (int(steps_per_graph), stream, ctypes.byref(graph))
        # (with NULL keys / fixed / resample / restraints this IS dd_graph_create_opts: the suffix chain of dd_api.hip only delegates)
        rc = self._step_entry(lib, "dd_graph_create", L)(ctypes.byref(chain["s"]), self._model_opts(), *self._step_extras(lib, L), *args)
        hip_lib.check(rc, "dd_graph_create")
        return graph

    _TRAJ_KEYS = ("traj_pos", "traj_v", "traj_bond", "traj_v0", "traj_vt", "traj_bt")

    def _run_chain_streaming(self, chain, num_steps, prime=True, runs=None):
        """One chain, trajectories kept: the step graph is replayed in chunks and every finished chunk of the six
        trajectory buffers is drained to the host (device -> pinned staging on a copy stream -> the result tensors,
        with the int32 -> int64 widening in that last host copy) while the GPU is already working on the next chunk,
        instead of one big blocking copy after the loop (scripts/sample_diffusion_decomp.py:361-364 reads them on the CPU).
        The host copies are numpy, i.e. single-threaded, on purpose: a torch CPU op spins up every core of the box and
        the HIP runtime's own threads then fall behind — measured 2.4 ms/step instead of 1.38 with 16-step chunks."""
        lib = hip_lib.load()
        dev, bufs, s = chain["dev"], chain["bufs"], chain["s"]
        cur = torch.cuda.current_stream(dev)
        side = self._side_stream(dev)
        copy_st = getattr(self, "_copy_stream", None)
        if copy_st is None or copy_st.device != dev:
            copy_st = self._copy_stream = torch.cuda.Stream(device=dev)
        keys = self._TRAJ_KEYS
        ent = chain["ent"]
        per_step = sum(bufs[k][0].numel() * bufs[k].element_size() for k in keys)
        # ~24 MB per chunk: the last chunk is the only one whose drain is not hidden (a few ms)
        chunk = int(os.environ.get("DD_TRAJ_CHUNK", "0")) or max(8, min(128, (24 << 20) // max(per_step, 1)))
        side.wait_stream(cur)
        spg = int(os.environ.get("DD_STEPS_PER_GRAPH", "1"))
        if runs is None:
            runs = self._chain_runs(chain, num_steps)
        if spg < 1 or num_steps % spg or chunk % spg or ent.get("resample"):      # (resampled chains: runs of any length)
            spg = 1
        cached = self._is_cached(ent)
        # Priming runs BEFORE this call looks at the cached graph handle: the priming chain goes through this very function
        # and may itself create -- or, if its launch structure differs, destroy and re-create -- the entry's graph.
        if (prime and cached and str(dev) not in DecompScorePosNet3D._primed_devices
                and os.environ.get("DD_PRIME", "1") != "0"):
            if self._prime_streaming(chain, spg):          # once per process and device (a 100-pocket job creates 100 graphs)
                DecompScorePosNet3D._primed_devices.add(str(dev))
        graph = self._ensure_step_graph(chain, spg, side.cuda_stream)     # (after priming: never a handle the priming chain destroyed)

        dbg = int(os.environ.get("DD_TRAJ_DEBUG", "0"))
        widen = {"traj_v": torch.int64, "traj_bond": torch.int64}
        host = {}                                          # staging views and result tensors: set up AFTER the first launch

        def setup_host_side():
            # staging: two flat pinned buffers per process and device, carved per shape (a pinned allocation costs tens of ms --
            # a job over 100 pockets of different sizes must not repeat it per pocket); grown only if a chunk needs more
            sizes = {k: chunk * bufs[k][0].numel() * bufs[k].element_size() for k in keys}
            need = sum((n + 255) // 256 * 256 for n in sizes.values())
            cache = getattr(self, "_staging", None)
            if cache is None or cache[0] != str(dev) or cache[1] < need:
                cap = max(need, 32 << 20)
                cache = self._staging = (str(dev), cap, [torch.empty(cap, dtype=torch.uint8).pin_memory() for _ in range(2)])
            slots = []
            for flat in cache[2]:
                sl, off = {}, 0
                for k in keys:
                    sl[k] = flat[off:off + sizes[k]].view(bufs[k].dtype).view((chunk,) + tuple(bufs[k].shape[1:]))
                    off += (sizes[k] + 255) // 256 * 256
                slots.append(sl)
            # Result tensors are allocated at the trajectory CAPACITY of the cached entry (32, 64, ... steps) and returned as
            # views of their first num_steps rows: a 5-step warm-up and a 20-step call then ask the allocator for blocks of the
            # same size, so the second call finds the first one's freed pages instead of faulting in fresh ones.
            rows = int(bufs[keys[0]].shape[0]) if os.environ.get("DD_FINAL_CAP", "1") != "0" else num_steps
            rows = max(rows, num_steps)
            final = {k: torch.empty((rows,) + tuple(bufs[k].shape[1:]), dtype=widen.get(k, bufs[k].dtype))[:num_steps] for k in keys}
            host.update(slots=slots, final=final, final_np={k: v.numpy() for k, v in final.items()},
                        slots_np=[{k: v.numpy() for k, v in sl.items()} for sl in slots])

        def drain(item):
            lo, hi, slot, done = item
            if not dbg & 8:
                done.synchronize()
            if dbg & 2:
                return
            if dbg & 16:
                for k in keys:
                    host["final"][k][lo:hi].copy_(host["slots"][slot][k][:hi - lo])
                return
            for k in keys:                             # single-threaded on purpose (see the docstring)
                np.copyto(host["final_np"][k][lo:hi], host["slots_np"][slot][k][:hi - lo], casting="same_kind")

        pending = []
        tr = self.__dict__.get("_trace")                   # tools/bench_call_trace.py: wall-clock stamps, no extra syncs
        mark = (lambda name: tr.append((name, time.perf_counter()))) if tr is not None else (lambda name: None)
        try:
            # a chain shorter than one chunk is still drained in ~3 pieces: only the last piece's copy is exposed
            piece = min(chunk, max(8, -(-num_steps // 3)))
            if spg > 1:
                piece = max(spg, piece // spg * spg)
            pieces = self._pieces(runs, piece)
            for c, (lo, hi, ops) in enumerate(pieces):
                mark(f"launch{c}<")
                if tr is not None and c == 0:              # (trace mode: the device's own clock around every piece)
                    gpu_ev = [torch.cuda.Event(enable_timing=True)]
                    gpu_ev[0].record(side)
                for op in ops:
                    if op == "jump":
                        self._jump(chain, side.cuda_stream)
                    else:
                        hip_lib.check(lib.dd_graph_launch(graph, op // spg, side.cuda_stream), "dd_graph_launch")
                mark(f"launch{c}>")
                ev = torch.cuda.Event(enable_timing=tr is not None)
                ev.record(side)
                if tr is not None:
                    gpu_ev.append(ev)
                if c == 0:
                    # everything the host needs for the drains is built while the device runs the first piece: the first
                    # graph replay is enqueued ~0.1 ms earlier (20-step calls: what the driver's bench line times)
                    setup_host_side()
                slots = host["slots"]
                # The previous piece is drained BEFORE this piece's copies are enqueued (the device has this piece's replays
                # queued, so it never waits for the host): at most one piece's copies -- 6 copies, torch's 6 pinned-block
                # events, 2 of ours -- are ever outstanding on the copy stream.  With two pieces outstanding the HIP runtime
                # blocked the host for 5.5 ms inside the 15th enqueue of a process's first three-piece call (an async copy of
                # 111 KB) and the device lost 0.85 ms in the piece that was running (profiles/round5_call_trace.txt).
                if pending:
                    drain(pending.pop(0))
                    mark(f"drained{c - 1}>")
                copy_st.wait_event(ev)
                mark(f"waitev{c}>")
                with torch.cuda.stream(copy_st):
                    for k in keys:
                        if not dbg & 1:
                            slots[c % 2][k][:hi - lo].copy_(bufs[k][lo:hi], non_blocking=True)
                            mark(f"cp{c}.{k[5:]}>")
                done = torch.cuda.Event()
                done.record(copy_st)
                pending.append((lo, hi, c % 2, done))
                if c == 0 and not dbg & 4:
                    tail = pieces[-1][0]
                    for k in keys:                     # first touch of the pages the un-hidden last drain writes
                        host["final_np"][k][tail:].fill(0)
                mark(f"copies{c}>")
            while pending:
                drain(pending.pop(0))
                mark("drained_tail>")
        finally:
            side.synchronize()
            copy_st.synchronize()
            mark("synced>")
            if tr is not None:
                tr.extend((f"[device ms piece {i}: {gpu_ev[i].elapsed_time(gpu_ev[i + 1]):.3f}]", time.perf_counter())
                          for i in range(len(gpu_ev) - 1))
            self._release_step_graph(ent, cached)
        final = host["final"]
        cur.wait_stream(side)
        chain["traj_cpu"] = final

    def _prime_streaming(self, chain, spg=1):
        """One-off per process and device, with the first cached chain that is streamed: stream a short chain (3 pieces of
        8 steps) through the same launch / copy / drain code once and put the chain's state back.  The first streamed
        call of a process that is three or more pieces long stalls the device for ~1 ms in its second or third piece
        (EXPERIMENTS.md R3-8: 10.6 instead of 9.7 ms for one 8-step piece); a 20-step chain after a 5-step warm-up would
        otherwise pay that inside the caller's timed call.  Returns False if this chain cannot be used for it."""
        bufs, s = chain["bufs"], chain["s"]
        n = min(int(bufs["traj_pos"].shape[0]), 24, int(s.t_start) + 1)     # (never past t = 0)
        n = n // max(1, spg) * max(1, spg)                                  # whole graph replays: the same step graph as the caller's
        if n < 17:
            return False
        state = {k: bufs[k].clone() for k in ("lig_pos", "lig_v", "lig_bond", "step_counter")}
        self._run_chain_streaming(chain, n, prime=False, runs=[(n, False)])     # (plain steps: no jumps, the epoch stays)
        chain.pop("traj_cpu", None)
        for k, v in state.items():
            bufs[k].copy_(v)
        torch.cuda.synchronize(chain["dev"])
        return True

    @staticmethod
    def _restraint_results(call, chains, out):
        """``restraint_dist`` [R] / ``restraint_atom`` [R] (the caller's flat ligand row of the atom that counts, or -1) of a call with a
        ``restraint`` entry, in the caller's restraint order: ONE dd_drift_restraint launch per chain on its final state."""
        if call.restraints is None:
            return
        lib, R, n_pos = hip_lib.load(), call.restraints["R"], call.n_pos
        general, traj = bool(call.restraints.get("general")), bool(call.restraints.get("traj"))
        pairs = general and bool(call.restraints["pair"].any())
        dist, atom, atom2 = torch.full((R,), math.inf), torch.full((R,), -1, dtype=torch.long), torch.full((R,), -1, dtype=torch.long)
        dist_t, atom_t, atom2_t = (torch.full((n_pos, R), math.inf), torch.full((n_pos, R), -1, dtype=torch.long),
                                   torch.full((n_pos, R), -1, dtype=torch.long))
        for c in chains:
            ent, bufs, dev = c["ent"], c["bufs"], c["dev"]
            rs = ent["restraints"]
            flat = lambda w: torch.where(w >= 0, rs["first"] + w, w)          # (rows within the sample -> the caller's flat rows)
            if not general:
                hip_lib.check(lib.dd_drift_restraint(hip_lib.ptr(bufs["lig_pos"]), hip_lib.ptr(bufs.get("decomp_index")), hip_lib.ptr(bufs.get("nl_real")),
                                                     c["B"], c["NL"], ctypes.byref(ent["restraints_struct"]), None, hip_lib.ptr(bufs["rs_grad"]), 0,
                                                     hip_lib.ptr(bufs["rs_dist"]), hip_lib.ptr(bufs["rs_winner"]), hip_lib.stream_ptr(dev)),
                              "dd_drift_restraint")
            else:                                                           # (no run state: the trajectory rows stay as the chain left them)
                hip_lib.check(lib.dd_drift_restraint2(hip_lib.ptr(bufs["lig_pos"]), hip_lib.ptr(bufs["lig_v"]), hip_lib.ptr(bufs.get("decomp_index")),
                                                      hip_lib.ptr(bufs.get("nl_real")), c["B"], c["NL"], ctypes.byref(ent["restraints_struct"]), None,
                                                      hip_lib.ptr(bufs["rs_grad"]), 0, hip_lib.ptr(bufs["rs_dist"]), hip_lib.ptr(bufs["rs_winner"]),
                                                      hip_lib.ptr(bufs["rs_winner2"]), hip_lib.stream_ptr(dev)), "dd_drift_restraint2")
                atom2[rs["order"]] = flat(bufs["rs_winner2"][:rs["R"]].cpu().long())
            dist[rs["order"]] = bufs["rs_dist"][:rs["R"]].cpu()
            atom[rs["order"]] = flat(bufs["rs_winner"][:rs["R"]].cpu().long())
            if traj and n_pos > 0:
                dist_t[:, rs["order"]] = bufs["rs_dist_traj"][:n_pos, :rs["R"]].cpu()
                atom_t[:, rs["order"]] = flat(bufs["rs_winner_traj"][:n_pos, :rs["R"]].cpu().long())
                atom2_t[:, rs["order"]] = flat(bufs["rs_winner2_traj"][:n_pos, :rs["R"]].cpu().long())
        out["restraint_dist"], out["restraint_atom"] = dist, atom
        if pairs:
            out["restraint_atom2"] = atom2
        if traj:
            out["restraint_dist_traj"], out["restraint_atom_traj"] = dist_t, atom_t
            if pairs:
                out["restraint_atom2_traj"] = atom2_t

    def _collect_chain(self, chain, num_steps, keep_traj, rows_atoms=None, rows_bonds=None):
        """Result dict of a finished chain.  rows_atoms / rows_bonds (padded batches): the rows of the dense [B*NL] /
        [B*Eb] layouts that are real, in the caller's flat order."""
        bufs, B, NL, offset = chain["bufs"], chain["B"], chain["NL"], chain["offset"]
        ligand_pos = bufs["lig_pos"].view(B, NL, 3) + offset[:, None, :]
        dev = chain["dev"]
        _check_queue(chain["s"], dev)
        pick_a = (lambda t: t) if rows_atoms is None else (lambda t, r=rows_atoms.to(dev): t.index_select(0, r))
        pick_b = (lambda t: t) if rows_bonds is None else (lambda t, r=rows_bonds.to(dev): t.index_select(0, r))
        out = {
            "pos": pick_a(ligand_pos.reshape(B * NL, 3)),
            "v": pick_a(bufs["lig_v"]).long(),
            "bond": pick_b(bufs["lig_bond"]).long(),
        }
        if keep_traj and num_steps > 0:
            cpu = chain.get("traj_cpu") or {k: bufs[k][:num_steps].cpu() for k in self._TRAJ_KEYS}
            sel_a = (lambda t: t) if rows_atoms is None else (lambda t: t.index_select(1, rows_atoms))
            sel_b = (lambda t: t) if rows_bonds is None else (lambda t: t.index_select(1, rows_bonds))
            st = {"pos_traj": sel_a(cpu["traj_pos"]), "v_traj": sel_a(cpu["traj_v"].long()), "bond_traj": sel_b(cpu["traj_bond"].long()),
                  "v0_traj": sel_a(cpu["traj_v0"]), "vt_traj": sel_a(cpu["traj_vt"]), "bt_traj": sel_b(cpu["traj_bt"])}
            for k, t in st.items():
                out[k] = list(t.unbind(0))
            # the same data as [T, rows, ...] tensors (the lists above are views of them): lets the harness split per
            # sample without stacking 6 x T tensors again
            out["_traj_stacked"] = st
        else:
            for k in ("pos_traj", "v_traj", "bond_traj", "v0_traj", "vt_traj", "bt_traj"):
                out[k] = []
        if chain.get("t_traj") is not None:                # resampled chains: the time of every position
            out["t_traj"] = chain["t_traj"].clone()
        return out
