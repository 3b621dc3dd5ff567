#!/usr/bin/env python
"""Reverse-step time of the sampler with the lin and the 'pre_att' bond head on C-small pockets (300 + 30 atoms), batch of 8,
production noise, 1000-step calls timed with HIP events after a warm-up call of the same length, the two heads alternating.
One JSON line per head.  usage: python tools/preatt_step_time.py [--batch 8] [--steps 1000] [--reps 3]"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
from decompdiff_amd import DecompScorePosNet3D, shipped_config, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--steps", type=int, default=1000)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda:0")
torch.manual_seed(0)
b = synth.build_sampling_batch(synth.make_pocket_small(0), args.batch)
bd = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
models = {}
for kind in ("lin", "pre_att"):
    cfg = shipped_config(bond_net_type=kind)
    m = DecompScorePosNet3D(cfg, 29, 10, 8)
    sd = m.state_dict()
    sd.update(synth.synthetic_state_dict(cfg, 0))
    m.load_state_dict(sd)
    models[kind] = m.to(dev)
run = lambda m: m.sample_diffusion(num_steps=args.steps, center_pos_mode="protein", seed=1, **bd)
for m in models.values():
    run(m)                                              # warm-up: kernels loaded, chain captured and cached
torch.cuda.synchronize()
ms = {kind: [] for kind in models}
for _ in range(args.reps):
    for kind, m in models.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(m)
        e1.record()
        torch.cuda.synchronize()
        ms[kind].append(e0.elapsed_time(e1) / args.steps)
for kind, v in ms.items():
    print(json.dumps(dict(bond_net_type=kind, batch=args.batch, NP=300, NL=30, steps=args.steps, ms_per_step=round(min(v), 4),
                          steps_per_s=round(1000.0 / min(v), 1), ms_per_step_all=[round(x, 4) for x in v])), flush=True)
