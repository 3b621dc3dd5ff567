#!/usr/bin/env python
"""Reverse-step time with per-sample noise keys against the seeded chain, at the bench shape (C-small pocket, 300 + 30 atoms,
batch 8): the same model and batch, `seed=` and `sample_keys=` calls alternating inside every repetition.  Production noise,
captured chains, trajectories kept (what bench.py times): calls of --steps steps timed with HIP events after a warm-up call of
the same length.  One JSON line per mode and batch size, then the ratio keyed / seeded of the medians.
usage: python tools/keyed_step_time.py [--batch 8] [--steps 500] [--reps 5]"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
from decompdiff_amd import DecompScorePosNet3D, sample_keys, shipped_config, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, nargs="+", default=[8])
ap.add_argument("--steps", type=int, default=500)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")

cfg = shipped_config()
m = DecompScorePosNet3D(cfg, 29, 10, 8)
sd = m.state_dict()
sd.update(synth.synthetic_state_dict(cfg, 0))
m.load_state_dict(sd, strict=True)
m = m.to(dev)
for B in args.batch:
    torch.manual_seed(0)
    b = synth.build_sampling_batch(synth.make_pocket_small(0), B)
    bd = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
    modes = {"seeded": dict(seed=1), "keyed": dict(sample_keys=sample_keys(1, range(B)))}
    run = lambda kw: m.sample_diffusion(num_steps=args.steps, center_pos_mode="protein", **bd, **kw)
    for kw in modes.values():                                      # warm-up: kernels loaded, both step graphs captured once
        run(kw)
    torch.cuda.synchronize()
    ms = {k: [] for k in modes}
    for _ in range(args.reps):
        for k, kw in modes.items():                                # (the two share one cached entry: each call re-captures its graph)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(kw)
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.steps)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    for k, v in ms.items():
        print(json.dumps(dict(mode=k, batch=B, NP=300, NL=30, steps=args.steps, ms_per_step=round(min(v), 4),
                              ms_per_step_median=round(med[k], 4), ms_per_step_all=[round(x, 4) for x in v])), flush=True)
    print(json.dumps(dict(batch=B, keyed_over_seeded_median=round(med["keyed"] / med["seeded"], 4),
                          keyed_over_seeded_min=round(min(ms["keyed"]) / min(ms["seeded"]), 4))), flush=True)
