#!/usr/bin/env python
"""Reverse-step time of the narrow bond layer (h_node_in_bond_net = False) on C-small pockets (300 + 30 atoms):
  narrow   the narrow model;
  zeroext  the same weights zero-extended through the wide path of the same build (five ligand projections per layer whose
           results are exact zeros, gathered and added per bond);
  shipped  the shipped (wide) configuration with its own synthetic weights -- what must not have moved.  Run the tool a second
           time with DD_HIP_LIB pointing at a build of the parent commit (--models shipped) for the before / after pair.
Production noise, captured chains: calls of --steps steps timed with HIP events after a warm-up call of the same length, the
models alternating inside every repetition.  One JSON line per model and batch size.
usage: python tools/hnode_step_time.py [--batch 1 8] [--steps 500] [--reps 5] [--models narrow zeroext shipped]"""
import argparse
import json
import os
import re
import sys

import torch

sys.path.insert(0, ".")
from decompdiff_amd import DecompScorePosNet3D, hip_lib, shipped_config, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
ap.add_argument("--steps", type=int, default=500)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--models", nargs="+", default=["narrow", "zeroext", "shipped"], choices=["narrow", "zeroext", "shipped"])
args = ap.parse_args()
dev = torch.device("cuda:0")


def zero_extend(sd):
    out = {}
    for k, v in sd.items():
        m = re.search(r"\.bond_layer\.(hk|hv|hq)_func\.net\.0\.weight$", k)
        if m:
            v = torch.cat([v, torch.zeros(128, 128 if m.group(1) == "hq" else 256)], 1)
        out[k] = v
    return out


def load(cfg, sd):
    m = DecompScorePosNet3D(cfg, 29, 10, 8)
    full = m.state_dict()
    full.update(sd)
    m.load_state_dict(full, strict=True)
    return m.to(dev)


narrow_cfg = shipped_config(h_node_in_bond_net=False)
narrow_sd = synth.synthetic_state_dict(narrow_cfg, 0)
build = {"narrow": lambda: load(narrow_cfg, narrow_sd), "zeroext": lambda: load(shipped_config(), zero_extend(narrow_sd)),
         "shipped": lambda: load(shipped_config(), synth.synthetic_state_dict(shipped_config(), 0))}
models = {k: build[k]() for k in args.models}
lib = os.environ.get("DD_HIP_LIB") or "default"
for B in args.batch:
    torch.manual_seed(0)
    b = synth.build_sampling_batch(synth.make_pocket_small(0), B)
    bd = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
    run = lambda m: m.sample_diffusion(num_steps=args.steps, center_pos_mode="protein", seed=1, **bd)
    outs = {k: run(m) for k, m in models.items()}                  # warm-up: kernels loaded, chain captured and cached
    torch.cuda.synchronize()
    if "narrow" in outs and "zeroext" in outs:                     # (faster and different is not faster)
        assert all(torch.equal(outs["narrow"][k], outs["zeroext"][k]) for k in ("pos", "v", "bond")), "narrow != zero-extended wide"
    ms = {k: [] for k in models}
    for _ in range(args.reps):
        for k, m in models.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(m)
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.steps)
    for k, v in ms.items():
        print(json.dumps(dict(model=k, lib=lib, abi=int(hip_lib.load().dd_abi_version()), batch=B, NP=300, NL=30, steps=args.steps,
                              ms_per_step=round(min(v), 4), ms_per_step_median=round(sorted(v)[len(v) // 2], 4),
                              ms_per_step_all=[round(x, 4) for x in v])), flush=True)
