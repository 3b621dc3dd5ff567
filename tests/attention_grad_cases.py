"""Cases of the attention-gradient tests: functional.scatter_attention / scatter_attention_pos (dd_attn_aggregate_*_bwd) against
torch autograd of the reference expression on the CPU in float64.  A plain helper module (no tests): tests/test_attention_grad_host.py
checks this builder and the closed forms the kernels implement, tests/test_gpu_attention_grad.py holds the ops to `reference`.

Segments.  SIZES: empty segments first (none before it has members), in the middle and last; every tail of the four-in-flight
member loop (1, 2, 3, 5, 31, 33, 65, 127); the kNN limits 32 and 64 and the sizes next to them; one size above 256.  15 segments:
the last workgroup (4 waves) is partly filled.

Inputs.  v, v16 and the cotangent standard normal, rel_x three times that, e_w uniform in [0, 1), q and k standard normal times
SCALES[name]: 1, 2, and 6 ("sharp": scores x 36, most segments are close to one-hot).

d32.  Per case, the largest absolute distance of the reference expression's fp32 CPU result (forward and every input gradient)
from the float64 one: what fp32 arithmetic itself costs on these inputs.  The GPU bound is 2e-5 at scales 1 and 2 (d32 <= 5e-6
there, asserted on the host) and max(2e-5, 4 * d32) at the sharp scale."""
import functools
import math

import torch

SIZES = [0, 1, 31, 32, 33, 0, 64, 65, 300, 1, 0, 2, 3, 5, 127]
SCALES = {"unit": 1.0, "double": 2.0, "sharp": 6.0}
NH, HD = 16, 8
SCALE = 1.0 / math.sqrt(HD)
TOL = 2e-5                                      # the siblings' bound (test_gpu_scatter_ops.py, GRAD_TOL of test_gpu_train_ops.py)
D32_MAX = 5e-6                                  # of the reference's own fp32 run at scales 1 and 2

NODE_CASES = [(scale, use_ew, per_edge) for scale in SCALES for use_ew in (True, False) for per_edge in (False, True)]
POS_CASES = [(scale, use_ew) for scale in SCALES for use_ew in (True, False)]


def layout():
    """(index [E] int64 sorted, seg_ptr [n + 1] int32, n)."""
    n = len(SIZES)
    index = torch.repeat_interleave(torch.arange(n), torch.tensor(SIZES))
    ptr = torch.zeros(n + 1, dtype=torch.int32)
    ptr[1:] = torch.tensor(SIZES).cumsum(0)
    return index, ptr, n


def inputs(form, scale, use_ew, per_edge=False):
    """fp32 CPU inputs of one case; `names`: the tensors that are differentiated, in the ops' argument order."""
    index, ptr, n = layout()
    E = index.numel()
    g = torch.Generator().manual_seed(1000 * (form == "pos") + 100 * list(SCALES).index(scale) + 10 * int(use_ew) + int(per_edge))
    s = SCALES[scale]
    q = torch.randn(n, 128, generator=g) * s
    t = dict(q=q[index].clone() if per_edge else q, k=torch.randn(E, 128, generator=g) * s)
    if form == "pos":
        t.update(v=torch.randn(E, NH, generator=g), rel_x=torch.randn(E, 3, generator=g) * 3.0, cot=torch.randn(n, 3, generator=g))
    else:
        t.update(v=torch.randn(E, 128, generator=g), cot=torch.randn(n, 128, generator=g))
    if use_ew:
        t["e_w"] = torch.rand(E, 1, generator=g)
    names = [k for k in ("q", "k", "v", "rel_x", "e_w") if k in t]
    return dict(t, index=index, ptr=ptr, n=n, names=names, per_edge=per_edge, form=form)


def alpha_of(q, k, index, n):
    """scatter_softmax((q_e * k / sqrt(8)).sum(-1), index, dim=0) -> [E,16] (max-shifted, as torch_scatter's composite)."""
    q_e = q if q.size(0) == index.numel() and q.size(0) != n else q[index]
    score = (q_e.view(-1, NH, HD) * k.view(-1, NH, HD)).sum(-1) * SCALE
    idx = index.unsqueeze(-1).expand_as(score)
    mx = torch.full((n, NH), -math.inf, dtype=score.dtype).scatter_reduce(0, idx, score.detach(), "amax")
    p = (score - mx[index]).exp()
    return p / torch.zeros(n, NH, dtype=score.dtype).index_add(0, index, p)[index]


def expression(form, t):
    """The reference expression (uni_transformer_edge.py:63-68 / 199-211) on the tensors of `t`, differentiable."""
    index, n = t["index"], t["n"]
    alpha = alpha_of(t["q"], t["k"], index, n)
    w = t["e_w"].view(-1, 1) if "e_w" in t else 1.0
    if form == "pos":
        m = (alpha * (t["v"] * w)).unsqueeze(-1) * t["rel_x"].unsqueeze(1)                       # [E,16,3]
        return torch.zeros(n, NH, 3, dtype=m.dtype).index_add(0, index, m).mean(1)
    m = (alpha.unsqueeze(-1) * (t["v"] * w).view(-1, NH, HD)).reshape(-1, 128)
    return torch.zeros(n, 128, dtype=m.dtype).index_add(0, index, m)


def autograd_run(form, t, dtype):
    """(out, {name: gradient}) of <expression, cot> under torch autograd in `dtype`."""
    leaves = {k: t[k].to(dtype).clone().requires_grad_(True) for k in t["names"]}
    out = expression(form, dict(t, **leaves))
    grads = torch.autograd.grad((out * t["cot"].to(dtype)).sum(), [leaves[k] for k in t["names"]])
    return out.detach(), dict(zip(t["names"], grads))


def closed_form(form, t):
    """The formulas the backward kernels implement, evaluated in float64 without autograd -> (out, {name: gradient})."""
    d = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in t.items()}
    index, n, g = d["index"], d["n"], d["cot"]
    E = index.numel()
    q, k, v = d["q"], d["k"], d["v"]
    q_e = q if t["per_edge"] else q[index]
    w = d["e_w"].view(-1) if "e_w" in d else torch.ones(E, dtype=torch.float64)
    alpha = alpha_of(q, k, index, n)
    seg_sum = lambda x: torch.zeros((n,) + x.shape[1:], dtype=x.dtype).index_add(0, index, x)
    per_ch = lambda x: x.repeat_interleave(HD, 1)                                                # [*,16] -> [*,128]
    grads = {}
    if form == "pos":
        rel = d["rel_x"]
        u = (g[index] * rel).sum(-1)                                                             # [E]
        t_eh = w[:, None] * v * u[:, None] / 16
        D = seg_sum(alpha * t_eh)
        av = (alpha * v).sum(-1)                                                                 # sum_h alpha v16
        out = seg_sum((alpha * v * w[:, None]).sum(-1, keepdim=True) * rel) / 16
        grads["v"] = alpha * (w * u / 16)[:, None]
        grads["rel_x"] = g[index] * (w / 16 * av)[:, None]
        d_ew = u / 16 * av
    else:
        out = seg_sum(per_ch(alpha) * v * w[:, None])
        gv = (g[index] * v).view(E, NH, HD).sum(-1)
        t_eh = w[:, None] * gv
        D = (g * out).view(n, NH, HD).sum(-1)
        grads["v"] = per_ch(alpha) * w[:, None] * g[index]
        d_ew = (alpha * gv).sum(-1)
    ds = alpha * (t_eh - D[index])
    grads["k"] = SCALE * per_ch(ds) * q_e
    dq_e = SCALE * per_ch(ds) * k
    grads["q"] = dq_e if t["per_edge"] else seg_sum(dq_e)
    if "e_w" in d:
        grads["e_w"] = d_ew.view(d["e_w"].shape)
    return out, grads


@functools.lru_cache(maxsize=None)
def reference(form, scale, use_ew, per_edge=False):
    """Everything a case needs, computed once per process and left unchanged: the inputs, the float64 output and gradients, and
    d32 (module docstring)."""
    t = inputs(form, scale, use_ew, per_edge)
    out64, g64 = autograd_run(form, t, torch.float64)
    out32, g32 = autograd_run(form, t, torch.float32)
    d32 = max([float((out32.double() - out64).abs().max())] + [float((g32[k].double() - g64[k]).abs().max()) for k in g64])
    return dict(t=t, out64=out64, grad64=g64, d32=d32)


def bound(scale, d32):
    return max(TOL, 4.0 * d32) if scale == "sharp" else TOL
