"""Cases of the member-mask tests: functional.scatter_attention / scatter_attention_pos with `member_mask`
(dd_attn_aggregate_*_masked, dd_attn_aggregate_*_bwd_masked) against torch autograd of the masked reference expression on the CPU
in float64.  A plain helper module (no tests): tests/test_attention_mask_host.py checks this builder and the closed forms,
tests/test_gpu_attention_mask.py holds the ops to `reference`.

Segments, inputs, scales, TOL, D32_MAX and `bound` are those of tests/attention_grad_cases.py (15 segments, 664 members).

Mask.  torch.rand(E, seed 77) < 0.7, then by segment size: 300 -> only the first 200 members are real (the prefix pattern of padded
batches); 64 -> all masked; 33 -> only the last member is real; 5 -> only the first member is masked; 32 -> all real; the first
size-1 segment is masked, the second real.  391 real members of 664, seven segments with both kinds, two non-empty segments
without a real member.

Reference.  A masked member does not exist: the softmax of a segment runs over its real members, a segment without one gives a
zero row.  Masked values are removed with torch.where BEFORE any arithmetic (scores, v, e_w, rel_x, per-edge q), so autograd
gives masked members exact zeros and nothing they hold can reach a result.

d32.  As in attention_grad_cases: per case, the largest distance of the fp32 CPU run of the reference from the float64 one.  Over
all cases it stays within 1.4e-6 (scale 1) and 3.4e-6 (scale 2) -- inside D32_MAX -- and 2.9e-5 at sharp (per-edge q with e_w; the
other sharp cases within 1.2e-5).  Per case it equals, to the digits shown, the d32 of the UNMASKED reference on the arrays
compacted to the real members: the mask adds no error of its own to the yardstick.  So the bounds carry over unchanged: 2e-5 at
scales 1 and 2, max(2e-5, 4 * d32) at sharp, d32 recomputed per case."""
import functools
import math

import torch

import attention_grad_cases as AG

SIZES, SCALES, NH, HD, SCALE = AG.SIZES, AG.SCALES, AG.NH, AG.HD, AG.SCALE
TOL, D32_MAX, bound = AG.TOL, AG.D32_MAX, AG.bound
NODE_CASES, POS_CASES = AG.NODE_CASES, AG.POS_CASES
N_REAL, N_MIXED, N_ALL_MASKED = 391, 7, 2                  # of the mask below (asserted on the host)


@functools.lru_cache(maxsize=None)
def _mask():
    index, ptr, n = AG.layout()
    m = torch.rand(index.numel(), generator=torch.Generator().manual_seed(77)) < 0.7
    seen_one = False
    for s, size in enumerate(SIZES):
        e0 = int(ptr[s])
        seg = m[e0:e0 + size]
        if size == 300:
            seg[:200], seg[200:] = True, False
        elif size == 64:
            seg[:] = False
        elif size == 33:
            seg[:-1], seg[-1] = False, True
        elif size == 5:
            seg[0], seg[1:] = False, True
        elif size == 32:
            seg[:] = True
        elif size == 1:
            seg[:] = seen_one                              # the first size-1 segment is masked, the second real
            seen_one = True
    return m


def mask():
    """bool [E]: True = the member is real (a fresh copy)."""
    return _mask().clone()


def inputs(form, scale, use_ew, per_edge=False):
    """attention_grad_cases.inputs plus `mask`."""
    return dict(AG.inputs(form, scale, use_ew, per_edge), mask=mask())


def alpha_of(q, k, index, n, m, per_edge):
    """Softmax over the real members of each segment -> [E,16]; masked members 0; a segment without real members all 0."""
    mh = m.unsqueeze(-1)
    q_e = torch.where(mh, q, torch.zeros_like(q)) if per_edge else q[index]
    score = (q_e.view(-1, NH, HD) * torch.where(mh, k, torch.zeros_like(k)).view(-1, NH, HD)).sum(-1) * SCALE
    idx = index.unsqueeze(-1).expand_as(score)
    neg = torch.full_like(score, -math.inf)
    mx = torch.full((n, NH), -math.inf, dtype=score.dtype).scatter_reduce(0, idx, torch.where(mh, score.detach(), neg), "amax")
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))                           # (no real member)
    # (a masked member's score is replaced by the maximum before the exponential: exp(0), finite in value and in gradient)
    p = torch.where(mh, (torch.where(mh, score, mx[index]) - mx[index]).exp(), torch.zeros_like(score))
    den = torch.zeros(n, NH, dtype=score.dtype).index_add(0, index, p)
    den = torch.where(den > 0, den, torch.ones_like(den))                                    # guarded: no real member
    return p / den[index]


def _select(t):
    """The tensors of `t` with the masked members' rows replaced by zeros (torch.where: nothing they hold is used)."""
    m = t["mask"].unsqueeze(-1)
    d = dict(t)
    for name in ("k", "v", "rel_x", "e_w") + (("q",) if t["per_edge"] else ()):
        if name in t:
            d[name] = torch.where(m, t[name], torch.zeros_like(t[name]))
    return d


def expression(form, t):
    """The masked reference expression on the tensors of `t`, differentiable."""
    index, n, m = t["index"], t["n"], t["mask"]
    alpha = alpha_of(t["q"], t["k"], index, n, m, t["per_edge"])
    d = _select(t)
    w = d["e_w"].view(-1, 1) if "e_w" in d else 1.0
    if form == "pos":
        x = (alpha * (d["v"] * w)).unsqueeze(-1) * d["rel_x"].unsqueeze(1)
        return torch.zeros(n, NH, 3, dtype=x.dtype).index_add(0, index, x).mean(1)
    x = (alpha.unsqueeze(-1) * (d["v"] * w).view(-1, NH, HD)).reshape(-1, 128)
    return torch.zeros(n, 128, dtype=x.dtype).index_add(0, index, x)


def autograd_run(form, t, dtype):
    """(out, {name: gradient}) of <expression, cot> under torch autograd in `dtype`."""
    leaves = {k: t[k].to(dtype).clone().requires_grad_(True) for k in t["names"]}
    out = expression(form, dict(t, **leaves))
    grads = torch.autograd.grad((out * t["cot"].to(dtype)).sum(), [leaves[k] for k in t["names"]])
    return out.detach(), dict(zip(t["names"], grads))


def closed_form(form, t):
    """attention_grad_cases.closed_form's formulas with alpha = 0 on masked members, in float64 without autograd."""
    d = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in _select(t).items()}
    index, n, g = d["index"], d["n"], d["cot"]
    E = index.numel()
    q, k, v = d["q"], d["k"], d["v"]
    q_e = q if t["per_edge"] else q[index]
    w = d["e_w"].view(-1) if "e_w" in d else torch.ones(E, dtype=torch.float64)
    alpha = alpha_of(q, k, index, n, t["mask"], t["per_edge"])
    seg_sum = lambda x: torch.zeros((n,) + x.shape[1:], dtype=x.dtype).index_add(0, index, x)
    per_ch = lambda x: x.repeat_interleave(HD, 1)
    grads = {}
    if form == "pos":
        rel = d["rel_x"]
        u = (g[index] * rel).sum(-1)
        t_eh = w[:, None] * v * u[:, None] / 16
        D = seg_sum(alpha * t_eh)
        av = (alpha * v).sum(-1)
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
    """Everything a case needs, computed once per process and left unchanged: the inputs with the mask, the float64 output and
    gradients of the masked expression, and d32 (module docstring)."""
    t = inputs(form, scale, use_ew, per_edge)
    out64, g64 = autograd_run(form, t, torch.float64)
    out32, g32 = autograd_run(form, t, torch.float32)
    assert all(bool(torch.isfinite(x).all()) for x in [out32, out64] + list(g32.values()) + list(g64.values()))
    d32 = max([float((out32.double() - out64).abs().max())] + [float((g32[k].double() - g64[k]).abs().max()) for k in g64])
    return dict(t=t, out64=out64, grad64=g64, d32=d32)


def compacted(t):
    """The case restricted to its real members: rows of the per-member tensors selected by the mask, segment pointer and index
    recomputed -- what the masked ops must reproduce bit for bit."""
    m = t["mask"]
    d = dict(t)
    for name in ("k", "v", "rel_x", "e_w") + (("q",) if t["per_edge"] else ()):
        if name in t:
            d[name] = t[name][m].clone()
    d["index"] = t["index"][m].clone()
    ptr = torch.zeros(t["n"] + 1, dtype=torch.int32)
    ptr[1:] = torch.bincount(d["index"], minlength=t["n"]).cumsum(0)
    d["ptr"] = ptr
    del d["mask"]
    return d
