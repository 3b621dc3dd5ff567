#!/usr/bin/env python
"""Reverse-step time with fixed atoms (`sample_diffusion(fixed=...)`) against the unfixed chain, at the bench shape (C-small pocket,
300 + 30 atoms, batch 8) with one third of every ligand held: the same model and batch, the calls `fixed=None`, `hold` and `replace`
alternating inside every repetition.  Production noise, captured chains, trajectories kept (what bench.py times): calls of --steps
steps timed with HIP events after a warm-up call of the same length.  One JSON line per mode, then the ratios to the unfixed median.
usage: python tools/fixed_step_time.py [--batch 8] [--steps 500] [--reps 5]"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
from decompdiff_amd import DecompScorePosNet3D, shipped_config, synth  # noqa: E402

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
    n, nb = b["init_ligand_pos"].shape[0], b["init_ligand_fc_bond_type"].numel()
    NL = n // B
    mask = (torch.arange(n) % NL) >= NL - NL // 3                  # the last third of every ligand (the scaffold rows come last)
    g = torch.Generator().manual_seed(1)
    known = dict(mask=mask, pos=b["prior_centers"][b["ligand_decomp_batch"]] + 0.8 * torch.randn(n, 3, generator=g),
                 v=torch.randint(0, 8, (n,), generator=g), bond=torch.randint(0, 5, (nb,), generator=g))
    modes = {"unfixed": dict(), "hold": dict(fixed=dict(known, mode="hold")), "replace": dict(fixed=dict(known, mode="replace"))}
    run = lambda kw: m.sample_diffusion(num_steps=args.steps, center_pos_mode="protein", seed=1, **bd, **kw)
    for kw in modes.values():                                      # warm-up: kernels loaded, every step graph captured once
        run(kw)
    torch.cuda.synchronize()
    ms = {k: [] for k in modes}
    for _ in range(args.reps):
        for k, kw in modes.items():                                # (the three share one cached entry: each call re-captures its graph)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(kw)
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.steps)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    for k, v in ms.items():
        print(json.dumps(dict(mode=k, batch=B, NP=300, NL=NL, held_atoms_per_sample=int(mask.sum()) // B, steps=args.steps,
                              ms_per_step=round(min(v), 4), ms_per_step_median=round(med[k], 4),
                              ms_per_step_all=[round(x, 4) for x in v])), flush=True)
    print(json.dumps(dict(batch=B, hold_over_unfixed_median=round(med["hold"] / med["unfixed"], 4),
                          replace_over_unfixed_median=round(med["replace"] / med["unfixed"], 4))), flush=True)
