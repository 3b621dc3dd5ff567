#!/usr/bin/env python
"""Time of the triplet lists of the ligand bond graph: functional.triplets (dd_csr_select_count, one host read of the total,
dd_csr_select_fill) against the same lists built by the ATen composition, oracle.ops.bond_triplets called on device tensors
(what a host that got past `import torch_sparse` would run per layer: sorts, cumsums, repeat_interleaves and boolean masks,
several of which synchronise the host).  Shapes: the benchmark's ligands, 30 atoms x 8 samples at node ids 330 b + 300 ...
(6 960 edges, 194 880 triplets), and 60 atoms x 8 (28 320 edges, 1 642 560 triplets).  Both sides end in a host read, so a call
is a round trip: HIP events around `--iters` back-to-back calls after a warm-up, `--reps` repeats, the two sides alternating;
one JSON line per case and side with min / median / max microseconds per call.  The lists are compared first.
usage: python tools/triplets_time.py [--iters 50] [--reps 7]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from decompdiff_amd import functional as F  # noqa: E402
from oracle import ops  # noqa: E402
import triplets_cases as C  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
assert torch.cuda.is_available(), "triplets_time.py measures on the GPU"
dev = torch.device("cuda:0")


def us_per_call(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / args.iters


for name, (n_atoms, n_protein) in {"30 atoms x 8": (30, 300), "60 atoms x 8": (60, 300)}.items():
    ei, n = C.bench_ligands(n_atoms, 8, n_protein)
    d = ei.to(dev)
    sides = {"functional.triplets (HIP)": lambda: F.triplets(d, n), "ATen composition": lambda: ops.bond_triplets(d, n)}
    got, want = sides["functional.triplets (HIP)"](), sides["ATen composition"]()
    assert all(torch.equal(g, w) for g, w in zip(got, want)), name
    times = {s: [] for s in sides}
    for run in sides.values():
        us_per_call(run)                                 # warm-up: code objects loaded, allocator blocks cached
    for _ in range(args.reps):
        for s, run in sides.items():
            times[s].append(us_per_call(run))
    for s in sides:
        t = sorted(times[s])
        print(json.dumps(dict(case=name, side=s, nodes=n, edges=int(ei.size(1)), triplets=int(got[2].numel()), iters=args.iters,
                              reps=args.reps, us_min=round(t[0], 1), us_median=round(t[len(t) // 2], 1), us_max=round(t[-1], 1))), flush=True)
