"""Fixtures of the num_blocks > 1 cases that the oracle does not restate, generated from the REFERENCE itself.

    python tools/make_blocks_golden.py

The oracle (oracle/model.py, oracle/diffusion.py) has the block loop but only the lin bond head, no node output MLPs and the C0
parameterisation.  For a two-block model with `bond_net_type: pre_att`, with `x2h_out_fc: True` and with `model_mean_type: noise`
the yardstick is the reference model (through oracle/ref_shims.py, the synthetic weights of every other fixture).  Writes
tests/golden/blocks_ref.npz:
  2x3_preatt_*, 2x3_outfc_*   forward at 48 + 12 atoms, B = 2: inputs (in_*), outputs (out_*)
  noise_step_*                one reverse step at t = 500 with injected noise: inputs, noise (noise_*), results
  *_boundary_x / _batch       the coordinates the reference's kNN call saw at the head of the second block, and their sample ids

A fixture is only kept if, at that block boundary, no centre's K-th and (K+1)-th neighbour are closer than 6e-4 A to a tie
(tests/blocks_fixtures.py: a near-tie makes the graph, and with it the output, a coin toss in any implementation): the batch
seed is advanced until the condition holds, and the chosen seed is stored.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import blocks_fixtures as BF                          # noqa: E402
from decompdiff_amd import synth                      # noqa: E402
from oracle import make_golden as MG                  # noqa: E402
from oracle import ref_shims                          # noqa: E402

GAP = 6e-4


def reference(**over):
    cfg = BF.config(2, 3, **over)
    sd = synth.synthetic_state_dict(cfg, seed=0)
    return cfg, ref_shims.load_reference_model(cfg.to_dict(), sd)


class KnnCalls:
    """Records the coordinates of every kNN call of the reference's refine net."""

    def __enter__(self):
        self.mod = sys.modules["models.encoders.uni_transformer_edge"]
        self.inner, self.calls = self.mod.knn_graph, []

        def knn_graph(x, k, batch=None, **kw):
            self.calls.append((x.detach().clone(), batch.clone()))
            return self.inner(x, k=k, batch=batch, **kw)
        self.mod.knn_graph = knn_graph
        return self

    def __exit__(self, *exc):
        self.mod.knn_graph = self.inner


def keep(name, out, calls, seed, K=32):
    assert len(calls) == 2, len(calls)                 # one forward of a two-block model
    x, bv = calls[1]
    gap = BF.knn_gap(x, bv, K)
    if gap < GAP:
        return False
    out[name + "_boundary_x"], out[name + "_boundary_batch"] = x.numpy()[None], bv.numpy()
    out[name + "_seed"] = np.array(seed)
    print(f"[{name}] batch seed {seed}: gap at the block boundary {gap:.3g} A")
    return True


def gen_forward(name, out):
    f = BF.FORWARD[name]
    cfg, ref = reference(**f["over"])
    for seed in range(f["seed"], f["seed"] + 1000, 10):
        batch = BF.batch(f["pocket"], f["B"], seed)
        with KnnCalls() as rec:
            want = MG.ref_forward(ref, batch)
        if keep(name, out, rec.calls, seed):
            break
    else:
        raise RuntimeError(name)
    out.update({name + "_" + k: v for k, v in MG.np_inputs(batch).items()})
    for k in BF.KEYS:
        out[f"{name}_out_{k}"] = want[k].numpy()


def gen_noise_step(out, t_start=500):
    name = "noise_step"
    s = BF.SAMPLING
    cfg, ref = reference(model_mean_type="noise")
    for seed in range(s["seed"], s["seed"] + 1000, 10):
        batch = BF.batch(s["pocket"], s["B"], seed)
        state = torch.get_rng_state()
        with KnnCalls() as rec:
            r = MG.run_ref_sampling(ref, batch, 1, None, t_start)
        if keep(name, out, rec.calls, seed):
            break
    else:
        raise RuntimeError(name)
    torch.set_rng_state(state)
    noise = synth.draw_step_noise(1, batch["init_ligand_pos"].size(0), batch["init_ligand_fc_bond_type"].size(0))
    out.update({name + "_" + k: v for k, v in MG.np_inputs(batch).items()})
    out.update({f"{name}_noise_{k}": v.numpy() for k, v in noise.items()})
    out[name + "_t_start"] = np.array(t_start)
    out[name + "_pos"], out[name + "_v"], out[name + "_bond"] = r["pos"].numpy(), r["v"].numpy(), r["bond"].numpy()
    out[name + "_log_v_recon"], out[name + "_log_v_prob"] = r["v0_traj"][0].numpy(), r["vt_traj"][0].numpy()
    out[name + "_log_b_prob"] = r["bt_traj"][0].numpy()


def main():
    out = {}
    gen_forward("2x3_preatt", out)
    gen_forward("2x3_outfc", out)
    gen_noise_step(out)
    path = os.path.join(MG.GOLDEN, "blocks_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
