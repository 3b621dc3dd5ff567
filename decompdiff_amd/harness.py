"""Sampling harness: the batch loop around ``model.sample_diffusion``.

Counterpart of ``sample_diffusion_ligand_decomp`` in
/root/reference/scripts/sample_diffusion_decomp.py:57-457 for the ``ref_prior`` / ``beta_prior(v2)`` modes
(equal atom counts per sample): per batch it draws the initial ligand coordinates around the arm / scaffold
prior centres, the initial bond and atom types (same torch-CPU RNG order as the reference, :163-194,306-312),
assembles the PyG-style flat batch (:300-326, increments of utils/data.py:439-444), calls
``model.sample_diffusion`` (:329-360) and splits the result per sample exactly like :361-410:

    pred_pos [NL,3] float64, pred_v [NL] int64, pred_pos_traj [T,NL,3] float64, pred_v_traj [T,NL],
    pred_v0_traj / pred_vt_traj [T,NL,8], pred_bond_index [2,Eb] (sample-local atom ids), pred_bond_type [Eb],
    pred_b_traj [T,Eb], pred_bt_traj [T,Eb,5], decomp_mask [NL] (arm id, -1 = scaffold)

RDKit reconstruction (:416-457) is a CPU chemistry step outside the hot path and is not done
here; the returned dicts carry everything it consumes.
"""
from __future__ import annotations

import time
from typing import Dict, List, Optional

import numpy as np
import torch

from . import synth
from .model import sample_keys
from .pocket_data import PocketData, build_batch


def unbatch_traj(traj: List[torch.Tensor], n_data: int, cum: np.ndarray, dtype=None, stacked=None) -> List[np.ndarray]:
    """reference: unbatch_v_traj (:46-53) — list over steps of [sum_n, ...] -> per sample [T, n_i, ...].  ``stacked``:
    the same trajectory as one [T, sum_n, ...] CPU tensor when the model provides it (no re-stacking; the per-sample
    arrays are then views of it)."""
    if len(traj) == 0:
        return [np.zeros((0,)) for _ in range(n_data)]
    stacked = stacked.numpy() if stacked is not None else torch.stack([t.cpu() for t in traj]).numpy()   # [T, sum_n, ...]
    if dtype is not None:
        stacked = stacked.astype(dtype)
    return [stacked[:, cum[k]:cum[k + 1]] for k in range(n_data)]


@torch.no_grad()
def sample_diffusion_ligand_decomp(model, pocket, num_samples: int, batch_size: int = 16,
                                   device="cuda:0", num_steps: Optional[int] = None, center_pos_mode: str = "protein",
                                   energy_drift_opt=None, per_sample_std_scale=None, noise_fn=None, seed: int = 0,
                                   use_graph: bool = True, prior_mode: str = "ref_prior", num_atoms_mode: str = "ref",
                                   arms_natoms_config=None, scaffold_natoms_config=None, natoms_sampler=None,
                                   atom_prior_probs=None, bond_prior_probs=None, pool_batches: int = 1,
                                   sample_key_seed: Optional[int] = None, first_sample_index: int = 0,
                                   fixed_fn=None, fixed_mode: str = "hold", resample=None, init: str = "host",
                                   restraints_fn=None, restraint_opts=None, time_levels=None) -> Dict[str, list]:
    """Sample ``num_samples`` ligands for one pocket in batches of ``batch_size``.

    ``pool_batches`` > 1 assembles that many consecutive batches exactly as the reference would (same random draws, same
    order) and hands them to the model as ONE collated batch: in the modes whose samples differ in size the model runs
    one dense group per distinct size, and pooling turns many groups of one or two samples into a few groups of several
    (4 pooled batches of 16 with 12 distinct sizes: 12 groups of ~5 instead of 4 x 12 groups of ~1).  Results come back
    in the reference's sample order; with device-generated noise the per-sample streams depend on the grouping, as the
    reference's depend on its batching.

    ``pocket`` is a :class:`synth.Pocket` (synthetic, ``ref_prior``-style batches with equal sizes) or a
    :class:`pocket_data.PocketData` (the reference's ``data`` fields; every ``prior_mode`` / ``num_atoms_mode`` of
    scripts/sample_diffusion_decomp.py:78-298, including the modes whose samples differ in size).

    ``noise_fn(batch_index, n_ligand_atoms, n_bonds, num_steps)`` may return pre-drawn reference-order noise for
    a batch (parity mode); otherwise the device Philox generator is used with ``seed + batch_index``.

    ``sample_key_seed`` (not None): per-sample noise keys instead -- output sample ``g`` of this call draws with
    ``model.sample_keys(sample_key_seed, first_sample_index + g)`` in every model call (``sample_diffusion(sample_keys=...)``; only
    for models that take the extra keywords; excludes ``noise_fn``), so the CHAIN of a sample no longer depends on ``batch_size``,
    ``pool_batches`` or on which process runs it: a shard of a larger job passes its first global sample index.  The keys make
    the chains reproducible, not -- with ``init="host"`` -- this function's initial draws: the initial coordinates, atom and bond
    types are then still drawn from torch's CPU generator in the reference's order, batch by batch, and so still depend on the
    batching (and a keyed model call draws nothing from that generator).  ``init="device"`` removes that limitation.

    ``init``: ``"host"`` (default) -- the path above, unchanged.  ``"device"`` (needs ``sample_key_seed``, excludes ``noise_fn``;
    ValueError otherwise) -- the JOB's contract: output sample ``first_sample_index + g`` is identical under any ``batch_size``,
    ``pool_batches``, shard or order, in size, initial state, chain, results and all trajectories, so a job can be re-run one
    sample at a time, resharded, or resumed.  Every sample is assembled ALONE (``build_batch(pocket, 1, ...)`` /
    ``synth.build_sampling_batch(pocket, 1, ...)``) with torch's and numpy's global generators seeded from that sample's key
    for the assembly -- so the atom counts of the ``prior`` / ``old`` / ``stat`` modes belong to the sample -- and restored
    afterwards: the caller's generators end the call in the state they entered it.  A call's samples are collated with
    ``synth.concat_sampling_batches``, the host-drawn ``init_ligand_*`` are dropped, and the model draws the first state on the
    device: ``sample_diffusion(init=dict(mode="prior", centers=..., stds=..., atom_prior=atom_prior_probs,
    bond_prior=bond_prior_probs), sample_keys=...)`` with the centres / stds the assembly drew its coordinates around.

    ``fixed_fn(sample_index, decomp_index_of_sample)`` (not None): conditional generation -- for output sample
    ``first_sample_index + g`` it returns ``dict(mask [n] bool, pos [n,3], v [n], bond [n*(n-1)])``, the sample's known atoms in
    the sample's own row order (``decomp_index_of_sample``: its arm ids, -1 = scaffold), or None for nothing held.  The dicts are
    collated into one flat ``fixed`` per model call (``sample_diffusion(fixed=...)`` with ``mode=fixed_mode``; only for models
    that take the extra keywords); a size that does not match the sample raises ValueError.  Works with ``pool_batches`` and
    ``sample_key_seed``; the batches' own draws and order do not change.

    ``resample`` (not None; needs ``fixed_fn``): ``dict(jump_length=j, n_resample=r)``, handed to every model call that holds
    atoms (``sample_diffusion(resample=...)``, RePaint's jump-back schedule); the trajectories then have one entry per position of
    ``model.resample_schedule`` instead of one per step.  A model call in which ``fixed_fn`` held nothing runs the plain chain.

    ``restraints_fn(sample_index, decomp_index_of_sample)`` (not None): distance restraints -- for output sample
    ``first_sample_index + g`` it returns ``dict(point [r,3], min_d, max_d[, weight, atom, group])`` (``atom``: rows of the SAMPLE's
    own order, -1 = use ``group``; the rest as the ``restraint`` entry of ``sample_diffusion(energy_drift_opt=...)``), or None.  The
    dicts are collated into one ``restraint`` entry per model call (`collate_restraints`; ``restraint_opts``: its ``scale`` /
    ``t_min`` / ``t_max``), appended to ``energy_drift_opt``.  Works with ``pool_batches``, ``sample_key_seed`` and
    ``init="device"``; the output gains ``restraint_dist`` / ``restraint_atom`` per sample (``restraint_atom``: sample-local row).
    The dict may carry the general form's keys -- ``classes`` / ``classes2``, ``atom2`` (sample rows) / ``group2``, ``form`` -- and
    ``restraint_opts`` its ``traj``; the output then also has ``restraint_atom2`` (-1 off the pairs) and, with ``traj``,
    ``restraint_dist_traj`` / ``restraint_atom_traj`` / ``restraint_atom2_traj`` [positions, r] per sample.

    ``time_levels`` (not None; only for models that take the extra keywords): strided sampling -- the strictly decreasing list of
    time levels every model call runs over (``sample_diffusion(time_levels=...)``, `stride_levels`), in every ``init`` mode;
    ``num_steps`` then counts positions of the list and ``None`` means the whole list.
    """
    out = {k: [] for k in ("pred_pos", "pred_v", "pred_pos_traj", "pred_v_traj", "pred_v0_traj", "pred_vt_traj",
                           "pred_bond_index", "pred_bond_type", "pred_b_traj", "pred_bt_traj", "decomp_mask")}
    time_list = []
    num_batch = int(np.ceil(num_samples / batch_size))
    pool_batches = max(1, int(pool_batches))
    if time_levels is not None and not _accepts_extras(model):
        raise ValueError("time_levels needs a model whose sample_diffusion takes time_levels=")
    steps = (model.num_timesteps if time_levels is None else len(time_levels)) if num_steps is None else num_steps

    def assemble_alone(g_local):
        """init="device": sample ``g_local`` of this call assembled alone under its own key -> (kwargs, [size], init centers, stds)"""
        key = int(sample_keys(sample_key_seed, int(first_sample_index) + g_local).item()) & 0xFFFFFFFFFFFFFFFF
        torch.manual_seed(key)
        np.random.seed([key & 0xFFFFFFFF, key >> 32])
        if isinstance(pocket, PocketData):
            drawn = []
            b, n_atoms, _ = build_batch(pocket, 1, prior_mode=prior_mode, num_atoms_mode=num_atoms_mode,
                                        num_classes=model.num_classes, num_bond_classes=model.num_bond_classes,
                                        arms_natoms_config=arms_natoms_config, scaffold_natoms_config=scaffold_natoms_config,
                                        natoms_sampler=natoms_sampler, atom_prior_probs=atom_prior_probs,
                                        bond_prior_probs=bond_prior_probs, init_out=drawn)
            centers, stds = drawn[0]
        else:
            scale = None if per_sample_std_scale is None else [per_sample_std_scale[g_local]]
            b = synth.build_sampling_batch(pocket, 1, num_bond_classes=model.num_bond_classes, num_classes=model.num_classes,
                                           per_sample_std_scale=scale)
            n_atoms, centers, stds = [pocket.num_ligand_atoms], b["prior_centers"], b["prior_stds"]
        return b, n_atoms, centers, stds

    def build(i):
        """batch i as the reference assembles it: (kwargs, ligand sizes, injected noise or None, init centers / stds or None)"""
        n_data = batch_size if i < num_batch - 1 else num_samples - batch_size * (num_batch - 1)
        if init == "device":
            gen_state = (torch.get_rng_state(), np.random.get_state())
            try:
                alone = [assemble_alone(i * batch_size + k) for k in range(n_data)]
            finally:
                torch.set_rng_state(gen_state[0])
                np.random.set_state(gen_state[1])
            batch = alone[0][0] if n_data == 1 else synth.concat_sampling_batches([a[0] for a in alone])
            return batch, [a[1][0] for a in alone], None, (torch.cat([a[2] for a in alone], 0), torch.cat([a[3] for a in alone], 0))
        if isinstance(pocket, PocketData):
            batch, n_atoms, _ = build_batch(pocket, n_data, prior_mode=prior_mode, num_atoms_mode=num_atoms_mode,
                                            num_classes=model.num_classes, num_bond_classes=model.num_bond_classes,
                                            arms_natoms_config=arms_natoms_config,
                                            scaffold_natoms_config=scaffold_natoms_config, natoms_sampler=natoms_sampler,
                                            atom_prior_probs=atom_prior_probs, bond_prior_probs=bond_prior_probs)
        else:
            scale = None
            if per_sample_std_scale is not None:
                scale = list(per_sample_std_scale[i * batch_size: i * batch_size + n_data])
            batch = synth.build_sampling_batch(pocket, n_data, num_bond_classes=model.num_bond_classes,
                                               num_classes=model.num_classes, per_sample_std_scale=scale)
            n_atoms = [pocket.num_ligand_atoms] * n_data
        noise = noise_fn(i, sum(n_atoms), sum(n * (n - 1) for n in n_atoms), steps) if noise_fn is not None else None
        return batch, n_atoms, noise, None

    if init not in ("host", "device"):
        raise ValueError(f"init must be 'host' or 'device', got {init!r}")
    if init == "device" and (sample_key_seed is None or noise_fn is not None):
        raise ValueError("init='device' needs sample_key_seed and excludes noise_fn: the first state is drawn with the samples' keys")
    if init == "device" and not _accepts_extras(model):
        raise ValueError("init='device' needs a model whose sample_diffusion takes sample_keys= and init=")
    if sample_key_seed is not None and noise_fn is not None:
        raise ValueError("sample_key_seed excludes noise_fn: a chain draws from one source")
    if resample is not None and (fixed_fn is None or noise_fn is not None):
        raise ValueError("resample needs fixed_fn and excludes noise_fn")
    n_done = 0                                                             # samples of the earlier model calls
    for i in range(0, num_batch, pool_batches):
        parts = [build(j) for j in range(i, min(num_batch, i + pool_batches))]
        if len(parts) == 1:
            batch, n_atoms, noise, drawn_around = parts[0]
        else:                                                              # one collated batch (PyG increments re-applied)
            batch = synth.concat_sampling_batches([p[0] for p in parts])
            n_atoms = [n for p in parts for n in p[1]]
            noise = None if parts[0][2] is None else {k: torch.cat([p[2][k] for p in parts], 1) for k in parts[0][2]}
            drawn_around = None if parts[0][3] is None else tuple(torch.cat([p[3][j] for p in parts], 0) for j in (0, 1))
        n_data = len(n_atoms)
        n_bonds = [n * (n - 1) for n in n_atoms]
        if init == "device":                                               # (the host-drawn first state is dropped)
            batch = dict(batch, init_ligand_pos=None, init_ligand_v=None, init_ligand_fc_bond_type=None)
        dev_batch = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in batch.items()}
        extra = dict(noise=noise, seed=seed + i, use_graph=use_graph) if _accepts_extras(model) else {}
        if sample_key_seed is not None and extra:
            first = int(first_sample_index) + n_done
            extra = dict(use_graph=use_graph, sample_keys=sample_keys(sample_key_seed, range(first, first + n_data)))
            if init == "device":
                extra["init"] = dict(mode="prior", centers=drawn_around[0], stds=drawn_around[1],
                                     atom_prior=None if atom_prior_probs is None else torch.as_tensor(np.asarray(atom_prior_probs, np.float32)),
                                     bond_prior=None if bond_prior_probs is None else torch.as_tensor(np.asarray(bond_prior_probs, np.float32)))
        if fixed_fn is not None and extra:
            fixed = collate_fixed(fixed_fn, int(first_sample_index) + n_done, n_atoms, batch["ligand_decomp_index"], fixed_mode)
            if fixed is not None:
                extra["fixed"] = fixed
                if resample is not None:
                    extra["resample"] = resample
        if time_levels is not None:
            extra["time_levels"] = time_levels
        drift_opt, rs_entry = energy_drift_opt, None
        if restraints_fn is not None and extra:
            rs_entry = collate_restraints(restraints_fn, int(first_sample_index) + n_done, n_atoms, batch["ligand_decomp_index"],
                                          **(restraint_opts or {}))
            drift_opt = list(energy_drift_opt or []) + [rs_entry]
        n_done += n_data
        t1 = time.time()
        r = model.sample_diffusion(num_steps=num_steps, center_pos_mode=center_pos_mode,
                                   energy_drift_opt=drift_opt, **extra, **dev_batch)
        cum_atoms = np.cumsum([0] + n_atoms)                                   # (:367)
        cum_bonds = np.cumsum([0] + n_bonds)                                   # (:390-393)
        pos = r["pos"].cpu().numpy().astype(np.float64)
        v = r["v"].cpu().numpy()
        bond = r["bond"].cpu().numpy()
        bond_index = batch["ligand_fc_bond_index"].numpy()
        decomp = batch["ligand_decomp_index"].numpy()
        stk = r.get("_traj_stacked") or {}
        pos_traj = unbatch_traj(r["pos_traj"], n_data, cum_atoms, np.float64, stk.get("pos_traj"))
        v_traj = unbatch_traj(r["v_traj"], n_data, cum_atoms, None, stk.get("v_traj"))
        v0_traj = unbatch_traj(r["v0_traj"], n_data, cum_atoms, None, stk.get("v0_traj"))
        vt_traj = unbatch_traj(r["vt_traj"], n_data, cum_atoms, None, stk.get("vt_traj"))
        b_traj = unbatch_traj(r["bond_traj"], n_data, cum_bonds, None, stk.get("bond_traj"))
        bt_traj = unbatch_traj(r["bt_traj"], n_data, cum_bonds, None, stk.get("bt_traj"))
        for k in range(n_data):
            a0, a1, b0, b1 = cum_atoms[k], cum_atoms[k + 1], cum_bonds[k], cum_bonds[k + 1]
            out["pred_pos"].append(pos[a0:a1])
            out["pred_v"].append(v[a0:a1])
            out["pred_bond_index"].append(bond_index[:, b0:b1] - a0)          # sample-local atom ids (:395)
            out["pred_bond_type"].append(bond[b0:b1])
            out["decomp_mask"].append(decomp[a0:a1])
            out["pred_pos_traj"].append(pos_traj[k])
            out["pred_v_traj"].append(v_traj[k])
            out["pred_v0_traj"].append(v0_traj[k])
            out["pred_vt_traj"].append(vt_traj[k])
            out["pred_b_traj"].append(b_traj[k])
            out["pred_bt_traj"].append(bt_traj[k])
            if rs_entry is not None:
                mine = rs_entry["sample"] == k
                ra = r["restraint_atom"][mine]
                out.setdefault("restraint_dist", []).append(r["restraint_dist"][mine].numpy())
                out.setdefault("restraint_atom", []).append(torch.where(ra >= 0, ra - int(a0), ra).numpy())
                # (the general form; second atoms are reported for every sample as soon as any call of the job has a pair -- filled
                #  in below --, so that a sample's output does not depend on its batch)
                for key in ("restraint_atom2",) + (("restraint_dist_traj", "restraint_atom_traj", "restraint_atom2_traj") if rs_entry.get("traj") else ()):
                    part = r[key][..., mine] if key in r else None
                    if part is not None and key != "restraint_dist_traj":
                        part = torch.where(part >= 0, part - int(a0), part)
                    out.setdefault(key, []).append(None if part is None else part.numpy())
        time_list.append(time.time() - t1)
    for key, like in (("restraint_atom2", "restraint_atom"), ("restraint_atom2_traj", "restraint_atom_traj")):
        if key in out and all(v is None for v in out[key]):
            del out[key]
        elif key in out:
            out[key] = [np.full_like(out[like][g], -1) if v is None else v for g, v in enumerate(out[key])]
    out["time_list"] = time_list
    return out


def collate_fixed(fixed_fn, first_index: int, n_atoms: List[int], decomp_index: torch.Tensor, mode: str):
    """The per-sample dicts of ``fixed_fn`` for the samples ``first_index ...`` of one model call (``n_atoms``: their ligand sizes,
    ``decomp_index``: the call's flat arm ids) as ONE flat ``fixed`` dict in the call's row order; None if nothing is held."""
    parts, a0 = [], 0
    for k, n in enumerate(n_atoms):
        f = fixed_fn(first_index + k, decomp_index[a0:a0 + n])
        a0 += n
        if f is None:
            f = dict(mask=torch.zeros(n, dtype=torch.bool), pos=torch.zeros(n, 3), v=torch.zeros(n, dtype=torch.long),
                     bond=torch.zeros(n * (n - 1), dtype=torch.long))
            parts.append((f, False))
            continue
        f = {key: torch.as_tensor(f[key]) for key in ("mask", "pos", "v", "bond")}
        for key, shape in (("mask", (n,)), ("pos", (n, 3)), ("v", (n,)), ("bond", (n * (n - 1),))):
            if tuple(f[key].shape) != shape:
                raise ValueError(f"fixed_fn: sample {first_index + k} has {n} ligand atoms, '{key}' must have shape {shape}, "
                                 f"got {tuple(f[key].shape)}")
        parts.append((f, True))
    if not any(held for _, held in parts):
        return None
    out = {key: torch.cat([f[key] for f, _ in parts], 0) for key in ("mask", "pos", "v", "bond")}
    out["pos"] = out["pos"].to(torch.float32)
    out["mode"] = mode
    return out


def collate_restraints(restraints_fn, first_index: int, n_atoms: List[int], decomp_index: torch.Tensor, scale=False, t_min=None,
                       t_max=None, traj=False):
    """The per-sample dicts of ``restraints_fn`` for the samples ``first_index ...`` of one model call (``n_atoms``: their ligand
    sizes, ``decomp_index``: the call's flat arm ids) as ONE ``restraint`` entry of energy_drift_opt: samples numbered by their
    place in the call, explicit atoms moved from the sample's rows to the call's flat rows.  A sample for which the function
    returns None has no restraints; a call without any still carries the (empty) entry.  The general form's keys pass through when
    any sample gives one: ``atom2`` like ``atom`` (sample rows -> flat rows), ``group2`` (a number, or one value each with
    RESTRAINT_NONE / None for "no second endpoint"), ``classes`` / ``classes2`` (a bool tensor [r, num_classes] or r entries of
    None | class ids), ``form`` (a name or r names); ``point`` may be left out by a sample whose restraints are all pairs."""
    from .model import RESTRAINT_ANY, RESTRAINT_NONE
    cols = {k: [] for k in ("sample", "point", "min_d", "max_d", "weight", "atom", "group")}
    extra = {k: [] for k in ("atom2", "group2", "classes", "classes2", "form")}
    used = set()
    a0 = 0
    for k, n in enumerate(n_atoms):
        f = restraints_fn(first_index + k, decomp_index[a0:a0 + n])
        if f is not None:
            if f.get("point") is None:                        # (pairs only: the count comes from the second endpoint)
                second = f.get("atom2") if f.get("atom2") is not None else f.get("group2")
                if second is None or torch.as_tensor(second).dim() != 1:
                    raise ValueError(f"restraints_fn: sample {first_index + k} gives no point and no atom2 / group2 of one value per restraint")
                point = torch.zeros(len(second), 3)
            else:
                point = torch.as_tensor(f["point"], dtype=torch.float32).reshape(-1, 3)
            r = int(point.shape[0])
            used |= {key for key in extra if f.get(key) is not None}

            def col(name, default, dtype):                     # a number for all r restraints, or one value each
                t = torch.as_tensor(f.get(name, default), dtype=dtype)
                return t.expand(r) if t.dim() == 0 else t
            atom = col("atom", -1, torch.long)
            if tuple(atom.shape) != (r,) or bool((atom < -1).any()) or bool((atom >= n).any()):
                raise ValueError(f"restraints_fn: sample {first_index + k} has {n} ligand atoms, 'atom' must hold {r} rows in [-1, {n})")
            cols["sample"].append(torch.full((r,), k, dtype=torch.long))
            cols["point"].append(point)
            cols["atom"].append(torch.where(atom >= 0, atom + a0, atom))
            cols["group"].append(col("group", RESTRAINT_ANY, torch.long))
            atom2 = col("atom2", -1, torch.long)
            if tuple(atom2.shape) != (r,) or bool((atom2 < -1).any()) or bool((atom2 >= n).any()):
                raise ValueError(f"restraints_fn: sample {first_index + k} has {n} ligand atoms, 'atom2' must hold {r} rows in [-1, {n})")
            extra["atom2"].append(torch.where(atom2 >= 0, atom2 + a0, atom2))
            g2 = f.get("group2")
            if g2 is not None and not torch.is_tensor(g2) and not isinstance(g2, int):
                g2 = [RESTRAINT_NONE if g is None else g for g in g2]
            g2 = torch.as_tensor(RESTRAINT_NONE if g2 is None else g2, dtype=torch.long)
            extra["group2"].append(g2.expand(r) if g2.dim() == 0 else g2)
            for name in ("classes", "classes2"):
                c = f.get(name)
                if torch.is_tensor(c) and c.dtype == torch.bool and c.dim() == 2:
                    c = [row.nonzero()[:, 0].tolist() for row in c]
                c = [None] * r if c is None else list(c)
                extra[name].append(c)
            form = f.get("form", "linear")
            extra["form"].append([form] * r if isinstance(form, str) else list(form))
            if any(len(extra[name][-1]) != r for name in extra):
                raise ValueError(f"restraints_fn: sample {first_index + k} has {r} restraints, every general field must be one value or hold {r}")
            for name, default in (("min_d", None), ("max_d", None), ("weight", 1.0)):
                if f.get(name, default) is None:
                    raise ValueError(f"restraints_fn: sample {first_index + k} gives no {name}")
                cols[name].append(col(name, default, torch.float32))
            if any(tuple(cols[name][-1].shape) != (r,) for name in ("group", "min_d", "max_d", "weight")):
                raise ValueError(f"restraints_fn: sample {first_index + k} has {r} points, every other field must be a number or hold {r} values")
        a0 += n
    empty = {"sample": torch.long, "point": torch.float32, "atom": torch.long, "group": torch.long}
    out = {k: (torch.cat(v) if v else torch.zeros((0, 3) if k == "point" else (0,), dtype=empty.get(k, torch.float32))) for k, v in cols.items()}
    out = dict(out, type="restraint", scale=bool(scale), t_min=t_min, t_max=t_max)
    for key in sorted(used):                                   # (an entry no sample gave a general key to stays a point entry)
        parts = extra[key]
        out[key] = torch.cat(parts) if key in ("atom2", "group2") and parts else [v for part in parts for v in part]
    if traj:
        out["traj"] = True
    return out


def _accepts_extras(model) -> bool:
    """The HIP model takes ``noise / seed / use_graph``; a model with the bare reference signature does not."""
    import inspect
    try:
        return "use_graph" in inspect.signature(model.sample_diffusion).parameters
    except (TypeError, ValueError):
        return False


# index -> atomic number of the 8 atom classes, ligand_atom_mode 'basic' (utils/transforms.py:41-50,73-75)
ATOMIC_NUMBER_OF_CLASS = (1, 6, 7, 8, 9, 15, 16, 17)
# ligand_atom_mode 'add_aromatic': class -> (atomic number, aromatic), 13 classes (utils/transforms.py:52-66)
AROMATIC_CLASSES = ((1, False), (6, False), (6, True), (7, False), (7, True), (8, False), (8, True), (9, False), (15, False), (15, True),
                    (16, False), (16, True), (17, False))
# ligand_atom_mode 'full': class -> (atomic number, hybridisation, aromatic), 23 classes (utils/transforms.py:15-39)
FULL_CLASSES = ((1, "S", False), (6, "SP", False), (6, "SP2", False), (6, "SP2", True), (6, "SP3", False), (7, "SP", False),
                (7, "SP2", False), (7, "SP2", True), (7, "SP3", False), (8, "SP2", False), (8, "SP2", True), (8, "SP3", False),
                (9, "SP3", False), (15, "SP2", False), (15, "SP2", True), (15, "SP3", False), (15, "SP3D", False), (16, "SP2", False),
                (16, "SP2", True), (16, "SP3", False), (16, "SP3D", False), (16, "SP3D2", False), (17, "SP3", False))
NUM_CLASSES_OF_MODE = {"basic": 8, "add_aromatic": 13, "full": 23}


def atomic_numbers_from_index(pred_v, mode: str = "basic") -> List[int]:
    """trans.get_atomic_number_from_index(pred_v, mode) (utils/transforms.py:73-83)."""
    idx = [int(i) for i in np.asarray(pred_v).tolist()]
    if mode == "basic":
        return [ATOMIC_NUMBER_OF_CLASS[i] for i in idx]
    if mode == "add_aromatic":
        return [AROMATIC_CLASSES[i][0] for i in idx]
    if mode == "full":
        return [FULL_CLASSES[i][0] for i in idx]
    raise ValueError(mode)


def is_aromatic_from_index(pred_v, mode: str = "basic"):
    """trans.is_aromatic_from_index(pred_v, mode) (utils/transforms.py:86-95): None for 'basic'."""
    idx = [int(i) for i in np.asarray(pred_v).tolist()]
    if mode == "add_aromatic":
        return [AROMATIC_CLASSES[i][1] for i in idx]
    if mode == "full":
        return [FULL_CLASSES[i][2] for i in idx]
    if mode == "basic":
        return None
    raise ValueError(mode)


def bond_graph(pred_bond_index, pred_bond_type):
    """The undirected molecular graph the reference's reconstruction builds from the predicted fully connected bond list
    (utils/reconstruct.py:593-606: a directed entry (i, j) with i < j and type > 0 becomes one bond, type 1-4 = single,
    double, triple, aromatic): ``(bonds [(i, j, order)], n_fragments)`` without RDKit.  ``n_fragments == 1`` is the
    reference's "complete" criterion (``'.' not in smiles``, scripts/sample_diffusion_decomp.py:445)."""
    bi = np.asarray(pred_bond_index)
    bt = np.asarray(pred_bond_type)
    n = int(bi.max()) + 1 if bi.size else 0
    bonds = [(int(i), int(j), int(t)) for i, j, t in zip(bi[0], bi[1], bt) if i < j and t > 0]
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for i, j, _ in bonds:
        parent[find(i)] = find(j)
    return bonds, len({find(a) for a in range(n)})


def to_result_records(out: Dict[str, list], ligand_filename: Optional[str] = None, reconstruct=None,
                      atom_enc_mode: str = "basic") -> List[dict]:
    """Per-sample records in the layout of the reference's ``result.pt`` (scripts/sample_diffusion_decomp.py:416-457,
    609-619): ``mol, smiles, pred_pos, pred_v, pred_pos_traj, pred_v_traj, decomp_mask, pred_bond_index (list),
    pred_bond_type`` (+ ``ligand_filename``), so that ``evaluate_mol_from_meta_full.py`` can consume them unchanged.

    Molecule reconstruction is RDKit/OpenBabel CPU chemistry outside the sampling hot path: pass the
    reference's ``recon.reconstruct_from_generated_with_bond`` (utils/reconstruct.py:579) -- or anything with its
    signature ``reconstruct(pred_pos, atomic_numbers, pred_bond_index, pred_bond_type) -> mol`` -- where those packages
    exist; a ``(mol, smiles)`` return is accepted too, otherwise ``smiles`` comes from ``Chem.MolToSmiles`` when RDKit is
    importable.  An exception from the callable is a failed reconstruction: ``mol`` None and ``smiles`` '' -- exactly
    what the reference stores (:440-443).  Without a callable the same placeholders are stored.  ``atom_enc_mode``: the
    ``ligand_atom_mode`` of the checkpoint (``basic`` / ``add_aromatic`` / ``full``: 8 / 13 / 23 atom classes, :422)."""
    records = []
    for i in range(len(out["pred_pos"])):
        bond_index = np.asarray(out["pred_bond_index"][i]).tolist()
        mol, smiles = None, ""
        if reconstruct is not None:
            try:
                r = reconstruct(out["pred_pos"][i], atomic_numbers_from_index(out["pred_v"][i], atom_enc_mode), bond_index,
                                out["pred_bond_type"][i])
                if isinstance(r, tuple):
                    mol, smiles = r
                else:
                    mol = r
                    try:
                        from rdkit import Chem                     # noqa: only where the chemistry stack exists
                        smiles = Chem.MolToSmiles(mol)
                    except ImportError:
                        smiles = ""
            except Exception:                                      # recon.MolReconsError in the reference
                mol, smiles = None, ""
        rec = {"mol": mol, "smiles": smiles, "pred_pos": out["pred_pos"][i], "pred_v": out["pred_v"][i],
               "pred_pos_traj": out["pred_pos_traj"][i], "pred_v_traj": out["pred_v_traj"][i],
               "decomp_mask": out["decomp_mask"][i], "pred_bond_index": bond_index,
               "pred_bond_type": out["pred_bond_type"][i]}
        if ligand_filename is not None:
            rec["ligand_filename"] = ligand_filename
        records.append(rec)
    return records


def save_result_pt(records: List[dict], path: str) -> None:
    """``torch.save(results, .../result.pt)`` (scripts/sample_diffusion_decomp.py:616-619): the list of per-sample dicts."""
    torch.save(records, path)


def load_result_pt(path: str) -> List[dict]:
    """What ``evaluate_mol_from_meta_full.py`` does first: ``torch.load(result.pt)`` (numpy arrays inside: full unpickling)."""
    return torch.load(path, weights_only=False)
