"""GPU (-m gpu): member masks of functional.scatter_attention / scatter_attention_pos and of
torch.ops.decompdiff_amd.scatter_attention(_pos) (dd_attn_aggregate_*_masked forward, dd_attn_aggregate_*_bwd_masked backward).
The cases, the mask, the float64 reference and the bound: tests/attention_mask_cases.py (15 segments, 664 members, 391 real).

1. forward and every gradient against float64 autograd of the masked reference, within bound(scale, d32);
2. no tolerance: the masked op on the full arrays equals, bit for bit, the unmasked op on the arrays compacted to the real
   members, and masked members get exact zeros;
3. NaN in every row of a masked member changes no bit of any result;
4. member_mask=None and an all-ones mask give bitwise the unmasked op;
5. argument checks of the C ABI and of `functional`;
6. the two routes of `functional` -- the compiled extension's ops and, without it, the ctypes binding -- give the same bits.
Every measured error is printed before it is judged."""
import ctypes
import os

import pytest
import torch

import attention_mask_cases as AM
import decompdiff_amd.torch_ops  # noqa: F401  (registers torch.ops.decompdiff_amd.*)
from decompdiff_amd import functional as FN
from decompdiff_amd import hip_lib

pytestmark = pytest.mark.gpu

PER_MEMBER = ("k", "v", "rel_x", "e_w")


def dev():
    return torch.device("cuda:0")


def _none_real(t):
    real = torch.zeros(t["n"], dtype=torch.long).index_add(0, t["index"], t["mask"].long())
    return (real == 0).nonzero().view(-1).tolist()


def _call(form, api, x, index, n, mask):
    fn = {("node", "functional"): FN.scatter_attention, ("node", "ops"): torch.ops.decompdiff_amd.scatter_attention,
          ("pos", "functional"): FN.scatter_attention_pos, ("pos", "ops"): torch.ops.decompdiff_amd.scatter_attention_pos}[form, api]
    if form == "pos":
        return fn(x["q"], x["k"], x["v"], x["rel_x"], index, n, x.get("e_w"), member_mask=mask)
    return fn(x["q"], x["k"], x["v"], index, n, x.get("e_w"), member_mask=mask)


def _run(form, api, t, mask="own", index=None):
    """(out, {name: grad}) of one differentiable call and its backward on the device; `mask`: "own" = the case's, else as given."""
    x = {k: t[k].to(dev()).requires_grad_(True) for k in t["names"]}
    m = t["mask"].to(dev()) if isinstance(mask, str) else mask
    out = _call(form, api, x, t["index"].to(dev()) if index is None else index, t["n"], m)
    out.backward(t["cot"].to(dev()))
    torch.cuda.synchronize()
    return out.detach(), {k: x[k].grad for k in t["names"]}


def _judge(tag, scale, ref, out, grads):
    t = ref["t"]
    bound = AM.bound(scale, ref["d32"])
    errs = {"out": float((out.cpu().double() - ref["out64"]).abs().max())}
    for name in t["names"]:
        g = grads[name]
        assert g is not None and g.shape == t[name].shape and g.dtype == torch.float32, name
        assert bool(torch.isfinite(g).all()), name
        errs["d" + name] = float((g.cpu().double() - ref["grad64"][name]).abs().max())
    print(f"\nATTNMASK {tag}: " + " ".join(f"{k}:{v:.3g}" for k, v in errs.items()) + f" bound:{bound:.3g} d32:{ref['d32']:.3g}")
    assert bool(torch.isfinite(out).all())
    assert max(errs.values()) <= bound, (errs, bound)
    _masked_are_zero(t, out, grads)


def _masked_are_zero(t, out, grads):
    masked = (~t["mask"]).to(dev())
    for name in PER_MEMBER + (("q",) if t["per_edge"] else ()):
        if name in grads:
            assert not bool(grads[name][masked].any()), f"d{name} of a masked member is exactly zero"
    none = _none_real(t)
    assert not bool(out[none].any()), "a segment without a real member gives a zero row"
    if not t["per_edge"]:
        assert not bool(grads["q"][none].any()), "a segment without a real member gives a zero dq row"


# ---- 1. against float64
@pytest.mark.parametrize("scale,use_ew,per_edge", AM.NODE_CASES)
def test_masked_node_form_vs_fp64_autograd(scale, use_ew, per_edge):
    ref = AM.reference("node", scale, use_ew, per_edge)
    out, grads = _run("node", "functional", ref["t"])
    _judge(f"node {scale} ew={use_ew} per_edge={per_edge} functional", scale, ref, out, grads)
    plan = FN.SegmentPlan(ref["t"]["index"].to(dev()), ref["t"]["n"])
    out_p, grads_p = _run("node", "functional", ref["t"], index=plan)
    assert torch.equal(out, out_p) and all(torch.equal(grads[k], grads_p[k]) for k in grads), "a SegmentPlan as index: the same bits"


@pytest.mark.parametrize("scale,use_ew", AM.POS_CASES)
def test_masked_coordinate_form_vs_fp64_autograd(scale, use_ew):
    ref = AM.reference("pos", scale, use_ew)
    out, grads = _run("pos", "functional", ref["t"])
    _judge(f"pos {scale} ew={use_ew} functional", scale, ref, out, grads)


@pytest.mark.parametrize("form,case", [("node", ("double", True, True)), ("pos", ("double", True))])
def test_masked_dispatcher_ops_are_differentiable(form, case):
    ref = AM.reference(form, *case)
    t = ref["t"]
    out, grads = _run(form, "ops", t)
    _judge(f"{form} {case} ops", case[0], ref, out, grads)
    out_f, grads_f = _run(form, "functional", t)
    assert torch.equal(out, out_f) and all(torch.equal(grads[k], grads_f[k]) for k in grads)
    # a uint8 mask is the same mask; without grad the plain forward is the same forward
    out_u, grads_u = _run(form, "ops", t, mask=t["mask"].to(dev()).to(torch.uint8))
    assert torch.equal(out, out_u) and all(torch.equal(grads[k], grads_u[k]) for k in grads)
    with torch.no_grad():
        plain = _call(form, "functional", {k: t[k].to(dev()) for k in t["names"]}, t["index"].to(dev()), t["n"], t["mask"].to(dev()))
    assert plain.grad_fn is None and torch.equal(plain, out)


# ---- 2. bitwise compaction identity
@pytest.mark.parametrize("form,use_ew,per_edge", [("node", True, False), ("node", False, False), ("node", True, True),
                                                  ("node", False, True), ("pos", True, False), ("pos", False, False)])
def test_masked_op_equals_the_unmasked_op_on_compacted_arrays_bit_for_bit(form, use_ew, per_edge):
    t = AM.reference(form, "unit", use_ew, *((per_edge,) if form == "node" else ()))["t"]
    c = AM.compacted(t)
    assert c["k"].size(0) == AM.N_REAL and int(c["ptr"][-1]) == AM.N_REAL
    out, grads = _run(form, "functional", t)
    out_c, grads_c = _run(form, "functional", c, mask=None)
    real = t["mask"].to(dev())
    assert torch.equal(out, out_c), "out"
    for name in t["names"]:
        if name == "q" and not per_edge:
            assert torch.equal(grads["q"], grads_c["q"]), "dq"
        else:
            assert torch.equal(grads[name][real], grads_c[name]), f"d{name} at the real members"
    _masked_are_zero(t, out, grads)


# ---- 3. poison
@pytest.mark.parametrize("form,use_ew,per_edge", [("node", True, False), ("node", True, True), ("node", False, True),
                                                  ("pos", True, False), ("pos", False, False)])
def test_nan_in_masked_rows_changes_no_bit(form, use_ew, per_edge):
    t = AM.reference(form, "double", use_ew, *((per_edge,) if form == "node" else ()))["t"]
    poisoned = dict(t)
    masked = ~t["mask"]
    for name in PER_MEMBER + (("q",) if per_edge else ()):
        if name in t:
            poisoned[name] = t[name].clone()
            poisoned[name][masked] = float("nan")
            assert bool(torch.isnan(poisoned[name]).any())
    out, grads = _run(form, "functional", t)
    out_p, grads_p = _run(form, "functional", poisoned)
    assert bool(torch.isfinite(out_p).all()) and torch.equal(out, out_p), "out"
    for name in t["names"]:
        assert bool(torch.isfinite(grads_p[name]).all()), name
        assert torch.equal(grads[name], grads_p[name]), name


# ---- 4. no mask, all-ones mask
@pytest.mark.parametrize("form,use_ew,per_edge", [("node", True, False), ("node", False, True), ("pos", True, False)])
def test_none_and_all_ones_masks_are_the_unmasked_op(form, use_ew, per_edge):
    t = AM.AG.reference(form, "double", use_ew, *((per_edge,) if form == "node" else ()))["t"]
    E = t["index"].numel()
    x = {k: t[k].to(dev()).requires_grad_(True) for k in t["names"]}
    fn = FN.scatter_attention_pos if form == "pos" else FN.scatter_attention
    args = (x["q"], x["k"], x["v"]) + ((x["rel_x"],) if form == "pos" else ()) + (t["index"].to(dev()), t["n"], x.get("e_w"))
    base = fn(*args)                                                     # today's call, no keyword
    base.backward(t["cot"].to(dev()))
    want = {k: x[k].grad for k in t["names"]}
    for tag, m in (("None", None), ("ones bool", torch.ones(E, dtype=torch.bool, device=dev())),
                   ("ones uint8", torch.ones(E, dtype=torch.uint8, device=dev()))):
        out, grads = _run(form, "functional", t, mask=m)
        assert torch.equal(out, base.detach()), tag
        assert all(torch.equal(grads[k], want[k]) for k in want), tag


def test_c_abi_null_mask_is_the_unmasked_entry_point():
    t = AM.AG.reference("node", "unit", True)["t"]
    lib, st, P = hip_lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), hip_lib.ptr
    d = {k: t[k].to(dev()).contiguous() for k in ("q", "k", "v", "cot")}
    ew, ptr, n = t["e_w"].to(dev()).reshape(-1).contiguous(), t["ptr"].to(dev()), t["n"]
    nan = lambda x: torch.full_like(x, float("nan"))
    o1, o2 = nan(d["cot"]), nan(d["cot"])
    assert lib.dd_attn_aggregate_node(P(d["q"]), 0, P(d["k"]), P(d["v"]), P(ew), P(ptr), n, P(o1), st) == 0
    assert lib.dd_attn_aggregate_node_masked(P(d["q"]), 0, P(d["k"]), P(d["v"]), P(ew), P(ptr), n, None, P(o2), st) == 0
    g1 = [nan(d["q"]), nan(d["k"]), nan(d["v"]), nan(ew)]
    g2 = [nan(d["q"]), nan(d["k"]), nan(d["v"]), nan(ew)]
    assert lib.dd_attn_aggregate_node_bwd(P(d["q"]), 0, P(d["k"]), P(d["v"]), P(ew), P(ptr), n, P(o1), P(d["cot"]), *[P(g) for g in g1], st) == 0
    assert lib.dd_attn_aggregate_node_bwd_masked(P(d["q"]), 0, P(d["k"]), P(d["v"]), P(ew), P(ptr), n, None, P(o2), P(d["cot"]),
                                                 *[P(g) for g in g2], st) == 0
    torch.cuda.synchronize()
    assert torch.equal(o1, o2) and all(torch.equal(a, b) for a, b in zip(g1, g2))


# ---- 5. argument checks
def test_masked_entry_points_reject_bad_arguments():
    lib, P = hip_lib.load(), hip_lib.ptr
    x = torch.zeros(4, 128, device=dev())
    p3 = torch.zeros(4, 3, device=dev())
    v16 = torch.zeros(4, 16, device=dev())
    ew = torch.zeros(4, device=dev())
    m = torch.ones(4, dtype=torch.uint8, device=dev())
    ptr = torch.tensor([0, 4], dtype=torch.int32, device=dev())
    # null pointers
    assert lib.dd_attn_aggregate_node_masked(None, 0, None, None, None, None, 1, P(m), None, None) != 0
    assert lib.dd_attn_aggregate_pos_masked(None, None, None, None, None, None, 1, P(m), None, None) != 0
    assert lib.dd_attn_aggregate_node_bwd_masked(None, 0, None, None, None, None, 1, P(m), None, None, None, None, None, None, None) != 0
    assert lib.dd_attn_aggregate_pos_bwd_masked(None, None, None, None, None, None, 1, P(m), None, None, None, None, None, None, None) != 0
    assert lib.dd_attn_aggregate_node_masked(P(x), 0, P(x), P(x), None, P(ptr), 1, P(m), None, None) != 0              # no out
    assert lib.dd_attn_aggregate_pos_masked(P(x), P(x), P(v16), None, None, P(ptr), 1, P(m), P(p3), None) != 0           # no rel_x
    # the same without a mask (NULL = all real: the sibling's checks)
    assert lib.dd_attn_aggregate_node_masked(None, 0, None, None, None, None, 1, None, None, None) != 0
    assert lib.dd_attn_aggregate_pos_bwd_masked(None, None, None, None, None, None, 1, None, None, None, None, None, None, None, None) != 0
    # n_seg < 0; e_w without d_ew
    assert lib.dd_attn_aggregate_node_masked(P(x), 0, P(x), P(x), None, P(ptr), -1, P(m), P(x), None) != 0
    assert lib.dd_attn_aggregate_pos_masked(P(x), P(x), P(v16), None, P(p3), P(ptr), -1, P(m), P(p3), None) != 0
    assert lib.dd_attn_aggregate_node_bwd_masked(P(x), 0, P(x), P(x), None, P(ptr), -1, P(m), P(x), P(x), P(x), P(x), P(x), None, None) != 0
    assert lib.dd_attn_aggregate_pos_bwd_masked(P(x), P(x), P(v16), None, P(p3), P(ptr), -1, P(m), P(p3), P(x), P(x), P(v16), None, P(p3), None) != 0
    assert lib.dd_attn_aggregate_node_bwd_masked(P(x), 0, P(x), P(x), P(ew), P(ptr), 1, P(m), P(x), P(x), P(x), P(x), P(x), None, None) != 0
    assert lib.dd_attn_aggregate_pos_bwd_masked(P(x), P(x), P(v16), P(ew), P(p3), P(ptr), 1, P(m), P(p3), P(x), P(x), P(v16), None, P(p3), None) != 0
    # n_seg == 0 is fine and touches nothing
    out = torch.full((4, 128), 7.0, device=dev())
    assert lib.dd_attn_aggregate_node_masked(P(x), 0, P(x), P(x), None, P(ptr), 0, P(m), P(out), None) == 0
    assert lib.dd_attn_aggregate_pos_masked(P(x), P(x), P(v16), None, P(p3), P(ptr), 0, P(m), P(out), None) == 0
    assert lib.dd_attn_aggregate_node_bwd_masked(P(x), 0, P(x), P(x), None, P(ptr), 0, P(m), P(x), P(x), P(out), P(out), P(out), None, None) == 0
    assert lib.dd_attn_aggregate_pos_bwd_masked(P(x), P(x), P(v16), None, P(p3), P(ptr), 0, P(m), P(p3), P(out), P(out), P(out), None, P(out), None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_functional_refuses_a_wrong_mask():
    t = AM.reference("node", "unit", True)["t"]
    x = {k: t[k].to(dev()) for k in t["names"]}
    index, n, E = t["index"].to(dev()), t["n"], t["index"].numel()
    good = t["mask"].to(dev())
    tp = AM.reference("pos", "unit", True)["t"]
    y = {k: tp[k].to(dev()) for k in tp["names"]}
    for bad in (good[:-1], torch.ones(E + 1, dtype=torch.bool, device=dev()), good.view(-1, 1), good.float(), good.long(), t["mask"]):
        with pytest.raises(ValueError):
            FN.scatter_attention(x["q"], x["k"], x["v"], index, n, x["e_w"], member_mask=bad)
        with pytest.raises(ValueError):
            FN.scatter_attention_pos(y["q"], y["k"], y["v"], y["rel_x"], index, n, y["e_w"], member_mask=bad)
    out = FN.scatter_attention(x["q"], x["k"], x["v"], index, n, x["e_w"])
    with pytest.raises(ValueError):
        FN.scatter_attention_backward(x["q"], x["k"], x["v"], index, n, x["e_w"], out, out, member_mask=good.float())
    with pytest.raises(ValueError):
        FN.scatter_attention_pos_backward(y["q"], y["k"], y["v"], y["rel_x"], index, n, y["e_w"], tp["cot"].to(dev()), member_mask=good[:-1])


# ---- 6. extension route == ctypes route
@pytest.mark.parametrize("form,per_edge", [("node", False), ("node", True), ("pos", False)])
def test_ctypes_route_equals_the_extension_route_bit_for_bit(form, per_edge, monkeypatch):
    """With the extension built every call of functional._attention_* goes through its ops, masked ones included; the ctypes
    branch is what a host without the extension (or with DD_HIP_LIB / DD_TORCH_EXT=0) runs.  Same entry point, same bits:
    the masked case (empty, all-masked and mixed segments) and the unmasked call, forward and every gradient.  The two routes differ
    in the forward alone -- functional._attention_*_bwd always calls over ctypes -- so the gradients compared here show that the
    backward is handed the same inputs (the node form reads the forward's `out`) on both."""
    t = AM.reference(form, "unit", True, *((per_edge,) if form == "node" else ()))["t"]
    # (with DD_HIP_LIB or DD_TORCH_EXT=0 set both halves run over ctypes and the comparison says nothing; a default run sets neither)
    assert FN.torch_ext() is not None or os.environ.get("DD_HIP_LIB") or os.environ.get("DD_TORCH_EXT") == "0", \
        "the compiled torch extension did not load: build it (python -m decompdiff_amd.build)"
    by_ext = [_run(form, "functional", t), _run(form, "functional", t, mask=None)]
    monkeypatch.setitem(FN._ext_state, "ops", None)
    assert FN.torch_ext() is None
    by_ctypes = [_run(form, "functional", t), _run(form, "functional", t, mask=None)]
    for (out_e, grads_e), (out_c, grads_c) in zip(by_ext, by_ctypes):
        assert torch.equal(out_e, out_c), "out"
        for name in t["names"]:
            assert torch.equal(grads_e[name], grads_c[name]), f"d{name}"
    _masked_are_zero(t, *by_ctypes[0])


def test_masked_ops_trace_with_fake_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        E, n = 10, 4
        q, k, v = torch.empty(n, 128, device="cuda"), torch.empty(E, 128, device="cuda"), torch.empty(E, 128, device="cuda")
        idx, ew = torch.empty(E, dtype=torch.long, device="cuda"), torch.empty(E, 1, device="cuda")
        m = torch.empty(E, dtype=torch.bool, device="cuda")
        ops = torch.ops.decompdiff_amd
        assert tuple(ops.scatter_attention(q, k, v, idx, n, ew, m).shape) == (n, 128)
        assert tuple(ops.scatter_attention(q, k, v, idx, n, ew).shape) == (n, 128)                    # positional call sites keep working
        out = ops.scatter_attention_backward(q, k, v, idx, n, ew, q, q, m)
        assert [tuple(o.shape) for o in out] == [(n, 128), (E, 128), (E, 128), (E, 1)]
        v16, rel, g3 = torch.empty(E, 16, device="cuda"), torch.empty(E, 3, device="cuda"), torch.empty(n, 3, device="cuda")
        assert tuple(ops.scatter_attention_pos(q, k, v16, rel, idx, n, None, m).shape) == (n, 3)
        out = ops.scatter_attention_pos_backward(q, k, v16, rel, idx, n, None, g3, m)
        assert [tuple(o.shape) for o in out] == [(n, 128), (E, 128), (E, 16), (E, 3), (0,)]
