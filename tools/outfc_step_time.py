#!/usr/bin/env python
"""Cost of the node output MLPs (x2h_out_fc = True) on C-small pockets (300 + 30 atoms):
  * reverse-step time of the sampler with and without the switch (production noise, calls of --steps steps timed with HIP events
    after a warm-up call of the same length, the two models alternating);
  * duration of the new launch alone (dd_node_out_fc on a [B * 330, 128] problem);
  * the same stage composed from existing launches: six dd_gemm128 launches and a copy, two of them with the LayerNorm + ReLU prologue
    (U_e A_e, + V_e h, the same pair for the bond MLP on all rows, then the two composed second products accumulated into h).
    The composition is built here for the comparison only; it is not shipped.
One JSON line per measurement.  usage: python tools/outfc_step_time.py [--batch 8] [--steps 1000] [--reps 3]"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
from decompdiff_amd import DecompScorePosNet3D, hip_lib, packing, shipped_config, synth  # noqa: E402

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
for out_fc in (False, True):
    cfg = shipped_config(x2h_out_fc=out_fc)
    m = DecompScorePosNet3D(cfg, 29, 10, 8)
    sd = m.state_dict()
    sd.update(synth.synthetic_state_dict(cfg, 0))
    m.load_state_dict(sd)
    models[out_fc] = m.to(dev)
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
for k, v in ms.items():
    print(json.dumps(dict(x2h_out_fc=k, batch=args.batch, NP=300, NL=30, steps=args.steps, ms_per_step=round(min(v), 4),
                          ms_per_step_all=[round(x, 4) for x in v])), flush=True)

# ---- the stage alone: the kernel against the composition from dd_gemm128 launches
lib = hip_lib.load()
B, NP, NL = args.batch, 300, 30
R = B * (NP + NL)
cfg = shipped_config(x2h_out_fc=True)
f = packing.node_out_fc(synth.synthetic_state_dict(cfg, 0), cfg)[0]
blk = packing.node_out_block(f).to(dev)
W = {k: v.to(dev).contiguous() for k, v in f.items()}
U = {m: W["W1_" + m][:, :128].contiguous() for m in "eb"}
V = {m: W["W1_" + m][:, 128:].contiguous() for m in "eb"}
A_e, A_b, h = torch.randn(R, 128, device=dev), torch.randn(B * NL, 128, device=dev), torch.randn(R, 128, device=dev)
A_bf = torch.zeros(B, NP + NL, 128, device=dev)
A_bf[:, NP:] = A_b.view(B, NL, 128)
A_bf = A_bf.view(R, 128).contiguous()
pre = {m: torch.empty(R, 128, device=dev) for m in "eb"}
out_k, out_c = torch.empty_like(h), torch.empty_like(h)
st = hip_lib.stream_ptr(dev)
P = hip_lib.ptr


def gemm(X, Wm, bias, ln, Y, acc):
    hip_lib.check(lib.dd_gemm128(P(X), R, 0, 128, R, P(Wm), P(bias), P(ln), P(Y), R, 0, 128, 128, acc, st), "dd_gemm128")


def kernel():
    hip_lib.check(lib.dd_node_out_fc(P(A_e), P(A_b), P(h), B, NP, NL, P(blk), None, None, P(out_k), st), "dd_node_out_fc")


def composed():
    out_c.copy_(h)
    for m, A in (("e", A_e), ("b", A_bf)):
        gemm(A, U[m], W["b1_" + m], None, pre[m], 0)
        gemm(h, V[m], None, None, pre[m], 1)
    gemm(pre["e"], W["W2_e"], W["c0"], W["ln_e"], out_c, 1)
    gemm(pre["b"], W["W2_b"], None, W["ln_b"], out_c, 1)


def time_us(fn, n=200):
    for _ in range(20):
        fn()
    best = 1e30
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, 1000.0 * e0.elapsed_time(e1) / n)
    return round(best, 2)


kernel()
composed()
torch.cuda.synchronize()
print(json.dumps(dict(stage="k_node_out_fc", rows=R, us=time_us(kernel))), flush=True)
print(json.dumps(dict(stage="composed: 6 dd_gemm128 launches + copy", rows=R, us=time_us(composed),
                      max_abs_diff=float((out_k - out_c).abs().max()))), flush=True)
