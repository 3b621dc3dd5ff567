"""Fixtures for kNN graphs wider than the shipped knn = 32 (DD_KNN_MAX = 64), generated from the REFERENCE itself.

    python tools/make_knn_golden.py [--only forward_k48|traj3_k64|loss_grad_k48]

Uses the helpers of oracle/make_golden.py (reference model through oracle/ref_shims.py, the same synthetic weights and
pockets); only the `knn` of the configuration differs.  Writes under tests/golden/:
  forward_k48.npz              one forward, knn = 48, 300 + 30 atoms, B = 2
  traj3_k64_b4_{plain,drift}.npz   3 reverse steps, knn = 64, 300 + 30 atoms, B = 4 (the oracle replays them on injected noise)
  loss_grad_k48.npz            get_diffusion_loss + backward, knn = 48, B = 2 (losses, outputs, gradients, gradient norms)
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from decompdiff_amd import synth                      # noqa: E402
from decompdiff_amd.config import shipped_config      # noqa: E402
from oracle import make_golden as MG                  # noqa: E402
from oracle import ref_shims                          # noqa: E402

B4_STD = [1.0, 0.9, 0.8, 1.1]


def reference(knn):
    cfg = shipped_config(knn=knn)
    sd = synth.synthetic_state_dict(cfg, seed=0)
    return cfg, sd, ref_shims.load_reference_model(cfg.to_dict(), sd)


def gen_forward_k48():
    cfg, sd, ref = reference(48)
    pocket = synth.make_pocket_small(seed=0)
    torch.manual_seed(2021)
    batch = synth.build_sampling_batch(pocket, 2)
    pr = MG.ref_forward(ref, batch)
    with torch.no_grad():
        po = MG.oracle_forward(sd, cfg, batch)
    worst = max(MG.maxabs(pr[k], po[k]) for k in pr)
    out = MG.np_inputs(batch)
    out.update({"out_" + k: v.numpy() for k, v in pr.items()})
    out["knn"], out["weight_seed"] = np.array(48), np.array(0)
    out["oracle_vs_reference_maxabs"] = np.array(worst)
    np.savez_compressed(os.path.join(MG.GOLDEN, "forward_k48.npz"), **out)
    print(f"[forward_k48] oracle maxabs diff = {worst:g}")


def gen_traj3_k64():
    cfg, sd, ref = reference(64)
    MG.gen_traj(ref, sd, cfg, "traj3_k64_b4_plain", synth.make_pocket_small(8), 4, 3, None, 2071)
    MG.gen_traj(ref, sd, cfg, "traj3_k64_b4_drift", synth.make_pocket_small(8), 4, 3, MG.DRIFT, 2072, std_scale=B4_STD)


def gen_loss_grad_k48():
    """As oracle/make_golden.py gen_loss, knn = 48, on a batch of two 90 + 12 atom complexes."""
    cfg, sd, ref = reference(48)
    pocket = synth.make_pocket(31, 90, (4, 3), 5, num_full_protein=0)
    torch.manual_seed(78)
    batch = synth.build_sampling_batch(pocket, 2, per_sample_std_scale=[1.0, 0.9])
    time_step = torch.tensor([700, 12])
    kw = dict(protein_pos=batch["protein_pos"], protein_v=batch["protein_v"], batch_protein=batch["batch_protein"],
              protein_group_idx=batch["protein_group_idx"], ligand_pos=batch["init_ligand_pos"], ligand_v=batch["init_ligand_v"],
              ligand_v_aux=batch["ligand_v_aux"], batch_ligand=batch["batch_ligand"], ligand_group_idx=batch["ligand_group_idx"],
              prior_centers=batch["prior_centers"], prior_stds=batch["prior_stds"], prior_num_atoms=batch["prior_num_atoms"],
              batch_prior=batch["batch_prior"], prior_group_idx=batch["prior_group_idx"],
              ligand_decomp_batch=batch["ligand_decomp_batch"], ligand_decomp_index=batch["ligand_decomp_index"],
              ligand_fc_bond_index=batch["ligand_fc_bond_index"], ligand_fc_bond_type=batch["init_ligand_fc_bond_type"],
              batch_ligand_bond=batch["batch_ligand_bond"], time_step=time_step)
    ref.zero_grad()
    torch.manual_seed(1234)
    res = ref.get_diffusion_loss(**kw)
    loss = res["losses"]["pos"] + 100.0 * res["losses"]["v"] + 100.0 * res["losses"]["bond"]
    loss.backward()
    out = MG.np_inputs(batch)
    out["time_step"] = time_step.numpy()
    out["noise_seed"], out["knn"] = np.array(1234), np.array(48)
    for k in ("pos", "v", "bond"):
        out["loss_" + k] = res["losses"][k].detach().numpy()
    for k in ("pred_ligand_pos", "pred_ligand_v", "x0"):
        out["out_" + k] = res[k].detach().numpy()
    params = dict(ref.named_parameters())
    for k in MG.GRAD_KEYS:
        out["grad__" + k.replace(".", "__")] = params[k].grad.numpy()
    names = sorted(k for k, p_ in params.items() if p_.requires_grad and p_.grad is not None)
    out["grad_norm_names"] = np.array(names)
    out["grad_norms"] = np.array([float(params[k].grad.double().norm()) for k in names])
    np.savez_compressed(os.path.join(MG.GOLDEN, "loss_grad_k48.npz"), **out)
    print(f"[loss_grad_k48] losses pos {float(res['losses']['pos']):.6g} v {float(res['losses']['v']):.6g} "
          f"bond {float(res['losses']['bond']):.6g}; {len(names)} parameter gradients")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, choices=["forward_k48", "traj3_k64", "loss_grad_k48"])
    args = ap.parse_args()
    torch.set_num_threads(int(os.environ.get("DD_GOLDEN_THREADS", min(16, os.cpu_count() or 1))))
    jobs = {"forward_k48": gen_forward_k48, "traj3_k64": gen_traj3_k64, "loss_grad_k48": gen_loss_grad_k48}
    for name, fn in jobs.items():
        if args.only in (None, name):
            fn()


if __name__ == "__main__":
    main()
