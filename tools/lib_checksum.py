#!/usr/bin/env python
"""Checksums of short seeded chains -- to confirm that two builds of the library (DD_HIP_LIB=...) give bit-identical results.
One line per case: the shipped model on C-small B=8, a 37-atom-ligand batch and the large pocket; then, on the small pocket,
a bond_net_type='pre_att' model, an x2h_out_fc model, a ragged batch as one padded launch sequence (nl_real, no layer-0
tables) and as size groups (several chains replayed together), a B=1 chain (lin_node inside the node launch, by shape) and
an eager chain (dd_sample_steps instead of graph replay).
usage: DD_HIP_LIB=path [DD_DRIFT=1] [DD_OPTS=key=value,...] python tools/lib_checksum.py [steps]"""
import os as _os
if _os.environ.get("DD_OPTS"): _os.environ.setdefault("DD_HIP_LIB", _os.path.join(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))), "decompdiff_amd", "lib", "libdecompdiff_hip_dbg.so"))  # measurement build: dd_debug_set_option

import os, sys, hashlib, torch
sys.path.insert(0, ".")
from decompdiff_amd import DecompScorePosNet3D, hip_lib, shipped_config, synth
for kv in os.environ.get("DD_OPTS", "").split(","):      # dd_debug_set_option settings, e.g. DD_OPTS="24=0"
    if kv:
        k, v = kv.split("="); assert hip_lib.load().dd_debug_set_option(int(k), int(v)) == 0
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 12
dev = torch.device("cuda:0")
drift = ([dict(type="armsca_prox", min_d=1.2, max_d=1.9), dict(type="clash", sigma=2.0, gamma=4.0)]
         if os.environ.get("DD_DRIFT") == "1" else None)          # (configs/sampling_drift.yml values)


def model(**over):
    cfg = shipped_config(**over)
    m = DecompScorePosNet3D(cfg, 29, 10, 8); sd = m.state_dict(); sd.update(synth.synthetic_state_dict(cfg, 0)); m.load_state_dict(sd)
    return m.to(dev)


def dense(pocket, B):
    return lambda: synth.build_sampling_batch(pocket, B)


def ragged():
    """Three complexes that differ in pocket and ligand size (one and two member tiles), collated."""
    parts = []
    for i, (nl, np_) in enumerate(((9, 150), (20, 120), (17, 131))):
        arm = max(2, nl // 4)
        p = synth.make_pocket(seed=300 + i, num_protein=np_, arm_atoms=(arm, arm), scaffold_atoms=nl - 2 * arm, num_full_protein=np_ + 150)
        parts.append(synth.build_sampling_batch(p, 1))
    return synth.concat_sampling_batches(parts)


def checksum(name, m, make_batch, n_steps, env=None, **kw):
    torch.manual_seed(0)
    b = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in make_batch().items()}
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        r = m.sample_diffusion(num_steps=n_steps, center_pos_mode="protein", seed=7, energy_drift_opt=drift, **kw, **b)
    except RuntimeError as e:                             # e.g. a measurement schedule that has no node-output stage (out_fc)
        if "decompdiff_hip" not in str(e):
            raise
        print(name, "refused:", str(e).split("failed: ")[-1], flush=True)
        return
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    h = hashlib.sha256()
    for k in ("pos", "v", "bond"):
        h.update(r[k].cpu().numpy().tobytes())
    h.update(torch.stack(r["v0_traj"]).numpy().tobytes())
    print(name, h.hexdigest()[:16], flush=True)


lin = model()
checksum("small", lin, dense(synth.make_pocket_small(0), 8), steps)
checksum("mid37", lin, dense(synth.make_pocket(5, 347, (12, 12), 13, num_full_protein=360), 4), steps)
checksum("large", lin, dense(synth.make_pocket_large(0), 2), steps)
few = min(steps, 12)
small2 = dense(synth.make_pocket_small(0), 2)
checksum("pre_att", model(bond_net_type="pre_att"), small2, few)
checksum("out_fc", model(x2h_out_fc=True), small2, few)
checksum("ragged_padded", lin, ragged, few, env={"DD_RAGGED_MODE": "padded"})
checksum("ragged_groups", lin, ragged, few, env={"DD_RAGGED_MODE": "groups"})
checksum("b1", lin, dense(synth.make_pocket_small(0), 1), few)
checksum("eager", lin, small2, few, use_graph=False)
