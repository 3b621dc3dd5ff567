#!/usr/bin/env python
"""Cost of a second block (num_blocks = 2: the kNN graph and the edge weights rebuilt in front of the second pass over the layers)
on C-small pockets (300 + 30 atoms): reverse-step time of the sampler for a 1 x L and a 2 x L model of the same weights
(production noise, calls of --steps steps timed with HIP events after a warm-up call of the same length, the two models
alternating), and for a 1 x 2L model -- as many layers and no block boundary -- so that the boundary's own cost shows as the
difference.  One JSON line per model.  With --forwards N the script instead runs N plain forward passes of the 2 x L model and
nothing else: the run to put under `rocprofv3 --kernel-trace --stats` for the duration of the boundary launch (k_graph on the workspace's x).
usage: python tools/blocks_step_time.py [--batch 8] [--layers 6] [--steps 1000] [--reps 3] [--forwards 0]"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
from decompdiff_amd import DecompScorePosNet3D, shipped_config, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--layers", type=int, default=6)
ap.add_argument("--steps", type=int, default=1000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--forwards", type=int, default=0)
args = ap.parse_args()
dev = torch.device("cuda:0")
torch.manual_seed(0)
b = synth.build_sampling_batch(synth.make_pocket_small(0), args.batch)
bd = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}


def build(nb, L):
    cfg = shipped_config(num_blocks=nb, num_layers=L)
    m = DecompScorePosNet3D(cfg, 29, 10, 8)
    sd = m.state_dict()
    sd.update(synth.synthetic_state_dict(cfg, 0))
    m.load_state_dict(sd)
    return m.to(dev)


if args.forwards:
    m = build(2, args.layers)
    for _ in range(args.forwards):
        m(protein_pos=bd["protein_pos"], protein_v=bd["protein_v"], batch_protein=bd["batch_protein"], protein_group_idx=None,
          init_ligand_pos=bd["init_ligand_pos"], init_ligand_v=bd["init_ligand_v"], init_ligand_v_aux=bd["ligand_v_aux"],
          batch_ligand=bd["batch_ligand"], ligand_group_idx=None, prior_centers=None, prior_stds=None, batch_prior=None,
          prior_group_idx=None, ligand_fc_bond_index=bd["ligand_fc_bond_index"], init_ligand_fc_bond_type=bd["init_ligand_fc_bond_type"])
    torch.cuda.synchronize()
    sys.exit(0)

models = {(1, args.layers): build(1, args.layers), (2, args.layers): build(2, args.layers), (1, 2 * args.layers): build(1, 2 * args.layers)}
run = lambda m: m.sample_diffusion(num_steps=args.steps, center_pos_mode="protein", seed=1, **bd)
for m in models.values():
    run(m)                                              # warm-up: kernels loaded, chain captured and cached
torch.cuda.synchronize()
ms = {k: [] for k in models}
for _ in range(args.reps):
    for k, m in models.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(m)
        e1.record()
        torch.cuda.synchronize()
        ms[k].append(e0.elapsed_time(e1) / args.steps)
for (nb, L), v in ms.items():
    print(json.dumps(dict(num_blocks=nb, num_layers=L, batch=args.batch, NP=300, NL=30, steps=args.steps, ms_per_step=round(min(v), 4),
                          ms_per_step_all=[round(x, 4) for x in v])), flush=True)
