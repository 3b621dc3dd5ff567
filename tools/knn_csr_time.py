#!/usr/bin/env python
"""Kernel time of the ragged kNN (dd_knn_csr) against the padded one (dd_knn_masked) on the same batch: B samples of
300-600 protein + 30-60 ligand atoms, K = 32, once as the flat PyG tensor with sample offsets and once padded to the largest
pocket / ligand with real counts; then the flat batch with one 4100-atom sample appended (three chunks of 2048 candidates,
dd_knn_csr only: the padded kernel stops at 2048 atoms per sample).  HIP events around `--iters` back-to-back launches after a
warm-up, `--reps` repeats, the two kernels alternating; one JSON line per case with min / median / max microseconds per launch.
usage: python tools/knn_csr_time.py [--batch 4] [--k 32] [--iters 200] [--reps 7]"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
from decompdiff_amd import hip_lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--k", type=int, default=32)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
dev = torch.device("cuda:0")
lib = hip_lib.load()
g = torch.Generator().manual_seed(0)
B, K = args.batch, args.k
n_p = torch.randint(300, 601, (B,), generator=g).tolist()
n_l = torch.randint(30, 61, (B,), generator=g).tolist()
NP, NL = max(n_p), max(n_l)
padded = torch.zeros(B, NP + NL, 3)
flat = []
for b in range(B):
    xp, xl = torch.randn(n_p[b], 3, generator=g) * 8.0, torch.randn(n_l[b], 3, generator=g) * 3.0
    padded[b, :n_p[b]], padded[b, NP:NP + n_l[b]] = xp, xl
    flat.append(torch.cat([xp, xl]))
st = hip_lib.stream_ptr(dev)


def csr_case(samples):
    x = torch.cat(samples).to(dev).contiguous()
    counts = torch.tensor([s.size(0) for s in samples])
    ptr = torch.zeros(len(samples) + 1, dtype=torch.int32)
    ptr[1:] = counts.cumsum(0)
    off = torch.zeros(len(samples) + 1, dtype=torch.int64)
    off[1:] = (counts * (counts - 1).clamp(max=K)).cumsum(0)
    E = int(off[-1])
    keep = (x, ptr.to(dev), off.to(dev), torch.empty(2, E, dtype=torch.int64, device=dev))
    run = lambda: hip_lib.check(lib.dd_knn_csr(hip_lib.ptr(keep[0]), hip_lib.ptr(keep[1]), len(samples), x.size(0), int(counts.max()), K, 0,
                                               hip_lib.ptr(keep[2]), E, hip_lib.ptr(keep[3]), st), "dd_knn_csr")
    return run, keep, dict(rows=int(x.size(0)), edges=E)


def masked_case():
    keep = (padded.to(dev).contiguous(), torch.tensor(n_p, dtype=torch.int32, device=dev), torch.tensor(n_l, dtype=torch.int32, device=dev),
            torch.empty(B, NP + NL, K, dtype=torch.int32, device=dev))
    run = lambda: hip_lib.check(lib.dd_knn_masked(hip_lib.ptr(keep[0]), B, NP, NL, K, hip_lib.ptr(keep[1]), hip_lib.ptr(keep[2]),
                                                  hip_lib.ptr(keep[3]), st), "dd_knn_masked")
    return run, keep, dict(rows=B * (NP + NL), edges=B * (NP + NL) * K)


def us_per_launch(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / args.iters


cases = {"dd_knn_masked padded": masked_case(), "dd_knn_csr flat": csr_case(flat),
         "dd_knn_csr flat + 4100-atom sample": csr_case(flat + [torch.randn(4100, 3, generator=g) * 12.0])}
# the two layouts hold the same atoms: same neighbours (padded-local ids -> flat rows)
nbr = cases["dd_knn_masked padded"][1][3]
cases["dd_knn_masked padded"][0]()
cases["dd_knn_csr flat"][0]()
torch.cuda.synchronize()
ei = cases["dd_knn_csr flat"][1][3].cpu()
o, e = 0, 0
for b in range(B):
    n = n_p[b] + n_l[b]
    loc = torch.cat([nbr[b, :n_p[b]], nbr[b, NP:NP + n_l[b]]]).long().cpu()
    loc = torch.where(loc >= NP, loc - NP + n_p[b], loc) + o
    assert torch.equal(loc.reshape(-1), ei[0, e:e + n * K]), b
    o, e = o + n, e + n * K
times = {name: [] for name in cases}
for name, (run, _, _) in cases.items():
    us_per_launch(run)                                   # warm-up: code object loaded, clocks up
for _ in range(args.reps):
    for name, (run, _, _) in cases.items():
        times[name].append(us_per_launch(run))
for name, (_, _, info) in cases.items():
    t = sorted(times[name])
    print(json.dumps(dict(case=name, K=K, n_p=n_p, n_l=n_l, **info, iters=args.iters, reps=args.reps, us_min=round(t[0], 2),
                          us_median=round(t[len(t) // 2], 2), us_max=round(t[-1], 2))), flush=True)
