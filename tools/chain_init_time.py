#!/usr/bin/env python
"""Time of the chain-init launch (`dd_chain_init`, both modes, unkeyed and keyed) beside the time the host path spends on the same
state: the draws of `init_ligand_pos / _v / _fc_bond_type` from torch's CPU generator (as `synth.build_sampling_batch` draws them) and
their upload.  The launch is timed with HIP events on the launch stream around --launches back-to-back launches after a warm-up; the
host path with the wall clock around draws + `.to(device)` + synchronize.  One JSON line per shape.
usage: python tools/chain_init_time.py [--reps 7] [--launches 200]"""
import argparse
import ctypes
import json
import sys
import time

import torch

sys.path.insert(0, ".")
from decompdiff_amd import DecompScorePosNet3D, hip_lib, sample_keys, shipped_config, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--launches", type=int, default=200)
args = ap.parse_args()
dev = torch.device("cuda:0")

cfg = shipped_config()
m = DecompScorePosNet3D(cfg, 29, 10, 8)
sd = m.state_dict()
sd.update(synth.synthetic_state_dict(cfg, 0))
m.load_state_dict(sd, strict=True)
m = m.to(dev)
lib = hip_lib.load()
med = lambda v: sorted(v)[len(v) // 2]
SHAPES = ((8, synth.make_pocket_small(0)), (16, synth.make_pocket(1, 300, (10, 10), 17)))     # B = 8 with 30 atoms, B = 16 with 37

for B, pocket in SHAPES:
    torch.manual_seed(0)
    b = synth.build_sampling_batch(pocket, B)
    n, nb = b["init_ligand_pos"].shape[0], b["init_ligand_fc_bond_type"].numel()
    known = dict(pos=b["init_ligand_pos"], v=b["init_ligand_v"], bond=b["init_ligand_fc_bond_type"])
    bd = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
    bd.update(init_ligand_pos=None, init_ligand_v=None, init_ligand_fc_bond_type=None)
    out = dict(batch=B, NL=n // B, atom_rows=n, bond_rows=nb, launches=args.launches)
    for mode, init, kw in (("prior", dict(mode="prior"), {}), ("noised", dict(mode="noised", **known), dict(start_step=500))):
        for keyed in (False, True):
            extra = dict(sample_keys=sample_keys(3, range(B))) if keyed else dict(seed=3)
            m.sample_diffusion(num_steps=0, center_pos_mode="protein", init=init, **bd, **kw, **extra)
            s, bufs = m._last
            st = hip_lib.init_struct(mode, bufs["ci_cc"], bufs["ci_std"], None, None, bufs.get("ci_x0c"), bufs.get("ci_v0"), bufs.get("ci_b0"),
                                     m.fixed_step_table().to(dev) if mode == "noised" else None)
            keys = hip_lib.ptr(bufs["sample_keys"]) if keyed else None
            launch = lambda: hip_lib.check(lib.dd_chain_init(ctypes.byref(s), keys, ctypes.byref(st), hip_lib.stream_ptr(dev)), "dd_chain_init")
            for _ in range(20):
                launch()
            torch.cuda.synchronize()
            us = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    launch()
                e1.record()
                torch.cuda.synchronize()
                us.append(1000.0 * e0.elapsed_time(e1) / args.launches)
            out[f"{mode}{'_keyed' if keyed else ''}_us_per_launch"] = round(med(us), 2)
            out[f"{mode}{'_keyed' if keyed else ''}_us_min"] = round(min(us), 2)
    # the host path on the same state: draws in the reference's order, then the upload
    cen, std = b["prior_centers"][b["ligand_decomp_batch"]], b["prior_stds"][b["ligand_decomp_batch"]]
    host = []
    for _ in range(args.reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pos = cen + torch.randn(n, 3) * std
        bond = synth.gumbel_argmax_uniform(nb, 5)
        v = synth.gumbel_argmax_uniform(n, 8)
        t1 = time.perf_counter()
        on_dev = [t.to(dev) for t in (pos, v, bond)]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        host.append((1e6 * (t1 - t0), 1e6 * (t2 - t1)))
    host = host[2:]
    out["host_draws_us"] = round(med([h[0] for h in host]), 1)
    out["host_upload_us"] = round(med([h[1] for h in host]), 1)
    print(json.dumps(out), flush=True)
