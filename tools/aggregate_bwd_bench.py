#!/usr/bin/env python
"""Time of the op-level attention backward kernels (dd_attn_aggregate_node_bwd / _pos_bwd) at the training bench shape
(B = 8 C-small pockets: 8 * 330 destinations x 32 kNN members with e_w, node and coordinate form; 8 * 870 bonds x 28 triplet
members, q per segment, no e_w) against their algorithmic bytes (HIP events; under `rocprofv3 --kernel-trace --stats` the same
launches give the per-kernel averages).  Per member the node form reads k, v, e_w and writes dk, dv, d_ew; per segment it
reads q, out, g and writes dq.  The backward reads a segment's k rows (coordinate form: v16, rel_x, e_w too) a second time:
those bytes are stated separately -- they should come from cache.
--mask-fraction F: also time the masked entry points (dd_attn_aggregate_*_masked, *_bwd_masked; forward and backward) at the same
shapes, beside the unmasked ones, with the last round(F * K) members of every segment masked (the prefix pattern of padded
batches).  The option is off by default: a plain run times the unmasked entry points alone, as before.  --mask-fraction 0 times an
all-real mask: the difference to the unmasked time is the price of the mask.
usage: python tools/aggregate_bwd_bench.py [reps] [--mask-fraction F]"""
import argparse, ctypes, sys, torch
sys.path.insert(0, ".")
from decompdiff_amd import hip_lib
ap = argparse.ArgumentParser(); ap.add_argument("reps", nargs="?", type=int, default=20)
ap.add_argument("--mask-fraction", type=float, default=None, help="time the masked entry points too, this fraction of every segment masked (0 = all-real mask)")
args = ap.parse_args()
if args.mask_fraction is not None and not 0.0 <= args.mask_fraction <= 1.0: ap.error("--mask-fraction must lie in [0, 1]")
lib = hip_lib.load(); dev = torch.device("cuda:0")
reps = args.reps
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream); P = hip_lib.ptr
def timed(fn):
    for _ in range(3): fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3
def report(name, n_seg, K, once, again, t):
    print(f"{name}: {n_seg} segments x {K} members, {once/1e6:.1f} MB algorithmic (+ {again/1e6:.1f} MB read a second time), {t*1e6:.1f} us -> "
          f"{once/t/1e12:.2f} TB/s ({once/t/8e12*100:.0f} % of 8 TB/s; {(once+again)/t/1e12:.2f} TB/s with the second read)")
def member_mask(n_seg, K):
    real = K - int(round(args.mask_fraction * K))
    return (torch.arange(K, device=dev) < real).to(torch.uint8).repeat(n_seg).contiguous(), real
def masked_line(name, t_fwd, t_fwd_m, t_bwd, t_bwd_m, real, K):
    print(f"    {name} masked ({real} of {K} members real): forward {t_fwd_m*1e6:.1f} us (unmasked {t_fwd*1e6:.1f} us), "
          f"backward {t_bwd_m*1e6:.1f} us (unmasked {t_bwd*1e6:.1f} us)")
for name, n_seg, K, use_ew in (("node_bwd (kNN, e_w)", 8 * 330, 32, True), ("node_bwd (triplets)", 8 * 870, 28, False)):
    E = n_seg * K
    q, k, v = torch.randn(n_seg, 128, device=dev), torch.randn(E, 128, device=dev), torch.randn(E, 128, device=dev)
    ew = torch.rand(E, device=dev) if use_ew else None
    ptr = (torch.arange(n_seg + 1, device=dev, dtype=torch.int32) * K).contiguous()
    out, g = torch.empty(n_seg, 128, device=dev), torch.randn(n_seg, 128, device=dev)
    hip_lib.check(lib.dd_attn_aggregate_node(P(q), 0, P(k), P(v), P(ew), P(ptr), n_seg, P(out), st))
    dq, dk, dv, dew = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v), (torch.empty_like(ew) if use_ew else None)
    t = timed(lambda: hip_lib.check(lib.dd_attn_aggregate_node_bwd(P(q), 0, P(k), P(v), P(ew), P(ptr), n_seg, P(out), P(g), P(dq), P(dk), P(dv), P(dew), st)))
    report(name, n_seg, K, (2048 + (8 if use_ew else 0)) * E + (2048 + 4) * n_seg, 512 * E, t)
    if args.mask_fraction is not None:
        mk, real = member_mask(n_seg, K)
        tf = timed(lambda: hip_lib.check(lib.dd_attn_aggregate_node(P(q), 0, P(k), P(v), P(ew), P(ptr), n_seg, P(out), st)))
        tfm = timed(lambda: hip_lib.check(lib.dd_attn_aggregate_node_masked(P(q), 0, P(k), P(v), P(ew), P(ptr), n_seg, P(mk), P(out), st)))
        tbm = timed(lambda: hip_lib.check(lib.dd_attn_aggregate_node_bwd_masked(P(q), 0, P(k), P(v), P(ew), P(ptr), n_seg, P(mk), P(out), P(g), P(dq), P(dk), P(dv), P(dew), st)))
        masked_line(name, tf, tfm, t, tbm, real, K)
n_seg, K = 8 * 330, 32
E = n_seg * K
q, k, v16 = torch.randn(n_seg, 128, device=dev), torch.randn(E, 128, device=dev), torch.randn(E, 16, device=dev)
ew, rel, g3 = torch.rand(E, device=dev), torch.randn(E, 3, device=dev), torch.randn(n_seg, 3, device=dev)
ptr = (torch.arange(n_seg + 1, device=dev, dtype=torch.int32) * K).contiguous()
dq, dk, dv, dew, dr = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v16), torch.empty_like(ew), torch.empty_like(rel)
t = timed(lambda: hip_lib.check(lib.dd_attn_aggregate_pos_bwd(P(q), P(k), P(v16), P(ew), P(rel), P(ptr), n_seg, P(g3), P(dq), P(dk), P(dv), P(dew), P(dr), st)))
report("pos_bwd (kNN, e_w)", n_seg, K, 2 * 592 * E + (1036 + 4) * n_seg, 592 * E, t)
if args.mask_fraction is not None:
    mk, real = member_mask(n_seg, K)
    out3 = torch.empty(n_seg, 3, device=dev)
    tf = timed(lambda: hip_lib.check(lib.dd_attn_aggregate_pos(P(q), P(k), P(v16), P(ew), P(rel), P(ptr), n_seg, P(out3), st)))
    tfm = timed(lambda: hip_lib.check(lib.dd_attn_aggregate_pos_masked(P(q), P(k), P(v16), P(ew), P(rel), P(ptr), n_seg, P(mk), P(out3), st)))
    tbm = timed(lambda: hip_lib.check(lib.dd_attn_aggregate_pos_bwd_masked(P(q), P(k), P(v16), P(ew), P(rel), P(ptr), n_seg, P(mk), P(g3), P(dq), P(dk), P(dv), P(dew), P(dr), st)))
    masked_line("pos_bwd (kNN, e_w)", tf, tfm, t, tbm, real, K)
