#!/usr/bin/env python
"""Reverse-step time of the sampler at several kNN widths (knn 32 / 48 / 64 by default) on C-small pockets (300 + 30 atoms),
batch of 8, production noise, timed with HIP events around whole calls after a warm-up call of the same length.
One JSON line per knn.  usage: python tools/knn_step_time.py [--knn 32 48 64] [--batch 8] [--steps 50] [--reps 3]"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
from decompdiff_amd import DecompScorePosNet3D, shipped_config, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--knn", type=int, nargs="+", default=[32, 48, 64])
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda:0")
torch.manual_seed(0)
b = synth.build_sampling_batch(synth.make_pocket_small(0), args.batch)
bd = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
for knn in args.knn:
    cfg = shipped_config(knn=knn)
    m = DecompScorePosNet3D(cfg, 29, 10, 8)
    sd = m.state_dict()
    sd.update(synth.synthetic_state_dict(cfg, 0))
    m.load_state_dict(sd)
    m = m.to(dev)
    run = lambda: m.sample_diffusion(num_steps=args.steps, center_pos_mode="protein", seed=1, **bd)
    run()                                               # warm-up: kernels loaded, chain captured and cached
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / args.steps)
    print(json.dumps(dict(knn=knn, batch=args.batch, NP=300, NL=30, steps=args.steps, ms_per_step=round(min(ms), 4),
                          ms_per_step_all=[round(x, 4) for x in ms])), flush=True)
