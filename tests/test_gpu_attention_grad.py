"""GPU (-m gpu): functional.scatter_attention / scatter_attention_pos and torch.ops.decompdiff_amd.scatter_attention(_pos) are
differentiable -- forward and every input gradient against torch autograd of the reference expression in float64 on the CPU
(tests/attention_grad_cases.py: the segments, the inputs, the bound and where it comes from), through the HIP backward kernels
dd_attn_aggregate_node_bwd / dd_attn_aggregate_pos_bwd.  Every measured error is printed before it is judged.

Measured on an MI355X (largest error of any case, forward or gradient): see EXPERIMENTS.md, "Differentiable scatter_attention"."""
import ctypes

import pytest
import torch

import attention_grad_cases as AG
import decompdiff_amd.torch_ops  # noqa: F401  (registers torch.ops.decompdiff_amd.*)
from decompdiff_amd import functional as FN
from decompdiff_amd import hip_lib

pytestmark = pytest.mark.gpu

EMPTY = [s for s, m in enumerate(AG.SIZES) if m == 0]


def dev():
    return torch.device("cuda:0")


def _leaves(t, needs=None):
    return {k: t[k].to(dev()).requires_grad_(needs is None or k in needs) for k in t["names"]}


def _call(form, api, x, index, n):
    fn = {("node", "functional"): FN.scatter_attention, ("node", "ops"): torch.ops.decompdiff_amd.scatter_attention,
          ("pos", "functional"): FN.scatter_attention_pos, ("pos", "ops"): torch.ops.decompdiff_amd.scatter_attention_pos}[form, api]
    if form == "pos":
        return fn(x["q"], x["k"], x["v"], x["rel_x"], index, n, x.get("e_w"))
    return fn(x["q"], x["k"], x["v"], index, n, x.get("e_w"))


def _run(form, api, t, index, needs=None):
    """(out, {name: grad or None}) of one differentiable call and its backward on the device."""
    x = _leaves(t, needs)
    out = _call(form, api, x, index, t["n"])
    out.backward(t["cot"].to(dev()))
    torch.cuda.synchronize()
    return out.detach(), {k: x[k].grad for k in t["names"]}


def _judge(tag, form, scale, ref, out, grads):
    t = ref["t"]
    bound = AG.bound(scale, ref["d32"])
    errs = {"out": float((out.cpu().double() - ref["out64"]).abs().max())}
    for name in t["names"]:
        g = grads[name]
        assert g is not None and g.shape == t[name].shape and g.dtype == torch.float32, name
        assert bool(torch.isfinite(g).all()), name
        errs["d" + name] = float((g.cpu().double() - ref["grad64"][name]).abs().max())
    print(f"\nATTNGRAD {tag}: " + " ".join(f"{k}:{v:.3g}" for k, v in errs.items()) + f" bound:{bound:.3g} d32:{ref['d32']:.3g}")
    assert max(errs.values()) <= bound, (errs, bound)
    if not t["per_edge"]:
        assert not bool(grads["q"][EMPTY].any()), "an empty segment's dq row is exactly zero"
    assert not bool(out[EMPTY].any())


@pytest.mark.parametrize("index_kind", ["tensor", "plan"])
@pytest.mark.parametrize("scale,use_ew,per_edge", AG.NODE_CASES)
def test_node_form_gradients_vs_fp64_autograd(scale, use_ew, per_edge, index_kind):
    ref = AG.reference("node", scale, use_ew, per_edge)
    t = ref["t"]
    index = t["index"].to(dev())
    if index_kind == "plan":
        index = FN.SegmentPlan(index, t["n"])
    with torch.no_grad():
        plain = _call("node", "functional", {k: t[k].to(dev()) for k in t["names"]}, index, t["n"])
    apis = ("functional", "ops") if index_kind == "tensor" else ("functional",)     # (the dispatcher ops take an index tensor)
    for api in apis:
        out, grads = _run("node", api, t, index)
        _judge(f"node {scale} ew={use_ew} per_edge={per_edge} {index_kind} {api}", "node", scale, ref, out, grads)
        assert torch.equal(out, plain), "the forward with grad needed is the no-grad forward"
        out2, grads2 = _run("node", api, t, index)
        assert all(torch.equal(grads[k], grads2[k]) for k in grads), "two backward runs agree bit for bit"


@pytest.mark.parametrize("scale,use_ew", AG.POS_CASES)
def test_coordinate_form_gradients_vs_fp64_autograd(scale, use_ew):
    ref = AG.reference("pos", scale, use_ew)
    t = ref["t"]
    for index_kind, apis in (("tensor", ("functional", "ops")), ("plan", ("functional",))):
        index = t["index"].to(dev())
        if index_kind == "plan":
            index = FN.SegmentPlan(index, t["n"])
        with torch.no_grad():
            plain = _call("pos", "functional", {k: t[k].to(dev()) for k in t["names"]}, index, t["n"])
        for api in apis:
            out, grads = _run("pos", api, t, index)
            _judge(f"pos {scale} ew={use_ew} {index_kind} {api}", "pos", scale, ref, out, grads)
            assert torch.equal(out, plain)
            out2, grads2 = _run("pos", api, t, index)
            assert all(torch.equal(grads[k], grads2[k]) for k in grads)


def _p(x):
    return hip_lib.ptr(x)


@pytest.mark.parametrize("use_ew,per_edge", [(True, False), (False, True)])
def test_node_backward_writes_every_element_of_nan_filled_buffers(use_ew, per_edge):
    """The C ABI directly: buffers need no initialisation (and an empty segment writes its zero dq row, nothing else)."""
    ref = AG.reference("node", "double", use_ew, per_edge)
    t = ref["t"]
    lib, st = hip_lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d = {k: t[k].to(dev()).contiguous() for k in t["names"] + ["cot"]}
    ptr, n = t["ptr"].to(dev()), t["n"]
    ew = d["e_w"].reshape(-1) if use_ew else None
    out = torch.full((n, 128), float("nan"), device=dev())
    assert lib.dd_attn_aggregate_node(_p(d["q"]), int(per_edge), _p(d["k"]), _p(d["v"]), _p(ew), _p(ptr), n, _p(out), st) == 0
    nan = lambda x: torch.full_like(x, float("nan"))
    dq, dk, dv, dew = nan(d["q"]), nan(d["k"]), nan(d["v"]), (nan(ew) if use_ew else None)
    rc = lib.dd_attn_aggregate_node_bwd(_p(d["q"]), int(per_edge), _p(d["k"]), _p(d["v"]), _p(ew), _p(ptr), n, _p(out), _p(d["cot"]),
                                        _p(dq), _p(dk), _p(dv), _p(dew), st)
    torch.cuda.synchronize()
    assert rc == 0
    got = dict(q=dq, k=dk, v=dv, **({"e_w": dew.view(-1, 1)} if use_ew else {}))
    errs = {k: float((g.cpu().double() - ref["grad64"][k]).abs().max()) for k, g in got.items()}
    print(f"\nATTNGRAD node C ABI ew={use_ew} per_edge={per_edge}: " + " ".join(f"d{k}:{v:.3g}" for k, v in errs.items()))
    assert all(bool(torch.isfinite(g).all()) for g in got.values())
    assert max(errs.values()) <= AG.TOL, errs


@pytest.mark.parametrize("use_ew", [True, False])
def test_pos_backward_writes_every_element_of_nan_filled_buffers(use_ew):
    ref = AG.reference("pos", "double", use_ew)
    t = ref["t"]
    lib, st = hip_lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d = {k: t[k].to(dev()).contiguous() for k in t["names"] + ["cot"]}
    ptr, n = t["ptr"].to(dev()), t["n"]
    ew = d["e_w"].reshape(-1) if use_ew else None
    nan = lambda x: torch.full_like(x, float("nan"))
    dq, dk, dv, dr, dew = nan(d["q"]), nan(d["k"]), nan(d["v"]), nan(d["rel_x"]), (nan(ew) if use_ew else None)
    rc = lib.dd_attn_aggregate_pos_bwd(_p(d["q"]), _p(d["k"]), _p(d["v"]), _p(ew), _p(d["rel_x"]), _p(ptr), n, _p(d["cot"]),
                                       _p(dq), _p(dk), _p(dv), _p(dew), _p(dr), st)
    torch.cuda.synchronize()
    assert rc == 0
    got = dict(q=dq, k=dk, v=dv, rel_x=dr, **({"e_w": dew.view(-1, 1)} if use_ew else {}))
    errs = {k: float((g.cpu().double() - ref["grad64"][k]).abs().max()) for k, g in got.items()}
    print(f"\nATTNGRAD pos C ABI ew={use_ew}: " + " ".join(f"d{k}:{v:.3g}" for k, v in errs.items()))
    assert all(bool(torch.isfinite(g).all()) for g in got.values())
    assert max(errs.values()) <= AG.TOL, errs


def test_backward_entry_points_reject_bad_arguments():
    lib = hip_lib.load()
    x = torch.zeros(4, 128, device=dev())
    p3 = torch.zeros(4, 3, device=dev())
    v16 = torch.zeros(4, 16, device=dev())
    ew = torch.zeros(4, device=dev())
    ptr = torch.tensor([0, 4], dtype=torch.int32, device=dev())
    P = _p
    assert lib.dd_attn_aggregate_node_bwd(None, 0, None, None, None, None, 4, None, None, None, None, None, None, None) != 0
    assert lib.dd_attn_aggregate_pos_bwd(None, None, None, None, None, None, 4, None, None, None, None, None, None, None) != 0
    # n_seg < 0; e_w without d_ew and d_ew without e_w; a missing output
    assert lib.dd_attn_aggregate_node_bwd(P(x), 0, P(x), P(x), None, P(ptr), -1, P(x), P(x), P(x), P(x), P(x), None, None) != 0
    assert lib.dd_attn_aggregate_node_bwd(P(x), 0, P(x), P(x), P(ew), P(ptr), 1, P(x), P(x), P(x), P(x), P(x), None, None) != 0
    assert lib.dd_attn_aggregate_node_bwd(P(x), 0, P(x), P(x), None, P(ptr), 1, P(x), P(x), P(x), P(x), P(x), P(ew), None) != 0
    assert lib.dd_attn_aggregate_node_bwd(P(x), 0, P(x), P(x), None, P(ptr), 1, P(x), P(x), P(x), None, P(x), None, None) != 0
    assert lib.dd_attn_aggregate_pos_bwd(P(x), P(x), P(v16), None, P(p3), P(ptr), -1, P(p3), P(x), P(x), P(v16), None, P(p3), None) != 0
    assert lib.dd_attn_aggregate_pos_bwd(P(x), P(x), P(v16), P(ew), P(p3), P(ptr), 1, P(p3), P(x), P(x), P(v16), None, P(p3), None) != 0
    assert lib.dd_attn_aggregate_pos_bwd(P(x), P(x), P(v16), None, P(p3), P(ptr), 1, P(p3), P(x), P(x), P(v16), None, None, None) != 0
    # n_seg == 0 is fine and launches nothing
    assert lib.dd_attn_aggregate_node_bwd(P(x), 0, P(x), P(x), None, P(ptr), 0, P(x), P(x), P(x), P(x), P(x), None, None) == 0
    assert lib.dd_attn_aggregate_pos_bwd(P(x), P(x), P(v16), None, P(p3), P(ptr), 0, P(p3), P(x), P(x), P(v16), None, P(p3), None) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("api", ["functional", "ops"])
@pytest.mark.parametrize("form", ["node", "pos"])
def test_inputs_that_need_no_gradient_get_none(form, api):
    ref = AG.reference(form, "unit", True)
    t = ref["t"]
    index = t["index"].to(dev())
    _, full = _run(form, api, t, index)
    for needs in (("k",), ("e_w",), ("q", "v")) + ((("rel_x",),) if form == "pos" else ()):
        out, grads = _run(form, api, t, index, needs=needs)
        for name in t["names"]:
            if name in needs:
                assert torch.equal(grads[name], full[name]), name
            else:
                assert grads[name] is None, name
    # nothing needs a gradient, or grad mode is off: the plain result, no graph
    plain = _call(form, api, _leaves(t, needs=()), index, t["n"])
    assert plain.grad_fn is None and not plain.requires_grad
    with torch.no_grad():
        assert _call(form, api, _leaves(t), index, t["n"]).grad_fn is None


def test_half_and_strided_inputs_get_gradients_of_their_own_dtype_and_shape():
    ref = AG.reference("node", "unit", True)
    t = ref["t"]
    index, n, cot = t["index"].to(dev()), t["n"], t["cot"].to(dev())
    E = index.numel()
    q = t["q"].to(dev()).half().requires_grad_(True)                                      # half
    k_wide = torch.zeros(E, 256, device=dev())
    k_wide[:, ::2] = t["k"].to(dev())
    k_wide.requires_grad_(True)
    k = k_wide[:, ::2]                                                                    # a strided view
    v = t["v"].to(dev()).view(E, 16, 8).requires_grad_(True)                              # heads unflattened
    e_w = t["e_w"].to(dev()).view(-1).requires_grad_(True)                                # [E] instead of [E,1]
    FN.scatter_attention(q, k, v, index, n, e_w).backward(cot)
    assert q.grad.dtype == torch.float16 and q.grad.shape == q.shape
    assert k_wide.grad.shape == (E, 256) and not bool(k_wide.grad[:, 1::2].any())
    assert v.grad.shape == (E, 16, 8) and e_w.grad.shape == (E,)
    # the same values as the fp32 contiguous call on the same numbers, up to the final cast
    x = dict(q=q.detach().float().requires_grad_(True), k=k.detach().contiguous().requires_grad_(True),
             v=v.detach().view(E, 128).requires_grad_(True), e_w=e_w.detach().view(E, 1).requires_grad_(True))
    FN.scatter_attention(x["q"], x["k"], x["v"], index, n, x["e_w"]).backward(cot)
    torch.cuda.synchronize()
    assert torch.equal(q.grad, x["q"].grad.half()) and torch.equal(k_wide.grad[:, ::2], x["k"].grad)
    assert torch.equal(v.grad.view(E, 128), x["v"].grad) and torch.equal(e_w.grad.view(E, 1), x["e_w"].grad)
    # coordinate form: half v16 and rel_x, e_w [E]
    rp = AG.reference("pos", "unit", True)["t"]
    y = dict(q=rp["q"].to(dev()).requires_grad_(True), k=rp["k"].to(dev()).requires_grad_(True),
             v=rp["v"].to(dev()).half().requires_grad_(True), rel_x=rp["rel_x"].to(dev()).half().requires_grad_(True),
             e_w=rp["e_w"].to(dev()).view(-1).requires_grad_(True))
    FN.scatter_attention_pos(y["q"], y["k"], y["v"], y["rel_x"], index, n, y["e_w"]).backward(rp["cot"].to(dev()))
    torch.cuda.synchronize()
    assert y["v"].grad.dtype == torch.float16 and y["v"].grad.shape == (E, 16)
    assert y["rel_x"].grad.dtype == torch.float16 and y["rel_x"].grad.shape == (E, 3) and y["e_w"].grad.shape == (E,)
    assert all(bool(torch.isfinite(g.grad).all()) for g in y.values())


def test_unsorted_index_and_permuted_plan_are_refused():
    t = AG.reference("node", "unit", False)["t"]
    x = _leaves(t)
    bad = t["index"].flip(0).to(dev())
    with pytest.raises(NotImplementedError):
        FN.scatter_attention(x["q"], x["k"], x["v"], bad, t["n"])
    with pytest.raises(NotImplementedError):
        FN.scatter_attention(x["q"], x["k"], x["v"], FN.SegmentPlan(bad, t["n"]), t["n"])
    tp = AG.reference("pos", "unit", False)["t"]
    y = _leaves(tp)
    with pytest.raises(NotImplementedError):
        FN.scatter_attention_pos(y["q"], y["k"], y["v"], y["rel_x"], FN.SegmentPlan(bad, tp["n"]), tp["n"])
    with pytest.raises(NotImplementedError):
        FN.scatter_attention_pos(y["q"], y["k"], y["v"], y["rel_x"], bad, tp["n"])
    # a plan of another table height or member count does not pass either
    plan = FN.SegmentPlan(t["index"].to(dev()), t["n"])
    with pytest.raises(ValueError):
        FN.scatter_attention(x["q"], x["k"], x["v"], plan, t["n"] + 1)
    with pytest.raises(ValueError):
        FN.scatter_attention(x["q"], x["k"][:-1], x["v"][:-1], plan, t["n"])


def test_backward_ops_trace_with_fake_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        E, n = 10, 4
        q, k, v = torch.empty(n, 128, device="cuda"), torch.empty(E, 128, device="cuda"), torch.empty(E, 128, device="cuda")
        idx, ew = torch.empty(E, dtype=torch.long, device="cuda"), torch.empty(E, 1, device="cuda")
        out = torch.ops.decompdiff_amd.scatter_attention_backward(q, k, v, idx, n, ew, q, q)
        assert [tuple(o.shape) for o in out] == [(n, 128), (E, 128), (E, 128), (E, 1)]
        v16, rel, g3 = torch.empty(E, 16, device="cuda"), torch.empty(E, 3, device="cuda"), torch.empty(n, 3, device="cuda")
        out = torch.ops.decompdiff_amd.scatter_attention_pos_backward(q, k, v16, rel, idx, n, None, g3)
        assert [tuple(o.shape) for o in out] == [(n, 128), (E, 128), (E, 16), (E, 3), (0,)]
