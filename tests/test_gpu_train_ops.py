"""GPU (-m gpu): the autograd Functions every layer of training.network goes through -- scatter_sum / gather / scatter_softmax
over a SegmentPlan (sorted, unsorted, and the unchecked plan of kNN sources), _attention with and without member_real,
linear128 / linear_feat with the weight given as the column slices of a wider first Linear that the network passes, and
dd_gemm128_tn(_bias) with accumulate = 1, lda > M, ldx > 128 and ldo > 128 -- each against torch autograd in float64 on the CPU,
forward and every input gradient.  The kernels are deterministic; the bounds are the sibling tests' (test_gpu_scatter_ops.py,
test_gpu_training.py): 1e-6 on softmax values, 2e-5 absolute on gradients at unit-scale inputs, 2e-6 relative (to the largest
expected element) on the GEMM-backed ops.  A segment sum of n fp32 rows is held to 1e-6 of the sum of the absolute terms, element
by element: any summation order is within (n - 1) u of it (u = 6e-8), a lane-then-tree order of 300 rows within ~11 u."""
import ctypes

import pytest
import torch

from decompdiff_amd import hip_lib, training

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 31, 32, 33, 0, 64, 65, 300, 1, 0]          # segment sizes: empty (also first and last), 1, around 32 / 64, above 256
SUM_REL, SOFTMAX_TOL, GRAD_TOL, GEMM_REL = 1e-6, 1e-6, 2e-5, 2e-6


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _index(kind, seed=0):
    """(index on the CPU, dim_size, check flag of seg_plan)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "sorted":
        return torch.repeat_interleave(torch.arange(len(SIZES)), torch.tensor(SIZES)), len(SIZES), True
    if kind == "unsorted":                                   # the same segments in no order: the plan sorts (perm / inv path)
        idx = torch.repeat_interleave(torch.arange(len(SIZES)), torch.tensor(SIZES))
        return idx[torch.randperm(idx.numel(), generator=g)], len(SIZES), True
    assert kind == "knn_src"                                 # like the sources of a kNN graph: every node appears, in no order
    n, k = 70, 32
    idx = torch.cat([torch.arange(n), torch.randint(0, n, (n * k - n,), generator=g)])
    return idx[torch.randperm(idx.numel(), generator=g)], n, False


def _plan(idx, n, check):
    return training.seg_plan(idx.to(_dev()), n, check=check)


def _seg_sum64(x, idx, n):
    return torch.zeros((n,) + tuple(x.shape[1:]), dtype=torch.float64).index_add_(0, idx, x)


def _softmax64(x, idx, n):
    """Segment softmax over dim 0 in float64 (differentiable; the shift by the segment maximum is a constant)."""
    ix = idx.view(-1, 1).expand_as(x)
    mx = torch.full((n, x.size(1)), float("-inf"), dtype=torch.float64).scatter_reduce(0, ix, x.detach(), "amax", include_self=True)
    e = (x - mx[idx]).exp()
    return e / _seg_sum64(e, idx, n)[idx]


KINDS = ("sorted", "unsorted", "knn_src")


@pytest.mark.parametrize("width", [3, 16, 48, 128])
@pytest.mark.parametrize("kind", KINDS)
def test_scatter_sum_and_gather_over_a_plan(kind, width):
    idx, n, check = _index(kind)
    plan = _plan(idx, n, check)
    g = torch.Generator().manual_seed(width)
    E = idx.numel()
    src, table = torch.randn(E, width, generator=g), torch.randn(n, width, generator=g)
    c_n, c_e = torch.randn(n, width, generator=g), torch.randn(E, width, generator=g)
    s = src.to(_dev()).requires_grad_(True)
    t = table.to(_dev()).requires_grad_(True)
    y = training.scatter_sum(s, plan)
    r = training.gather(t, plan)
    ((y * c_n.to(_dev())).sum() + (r * c_e.to(_dev())).sum()).backward()
    want_y, room_y = _seg_sum64(src.double(), idx, n), _seg_sum64(src.double().abs(), idx, n)
    want_dt, room_dt = _seg_sum64(c_e.double(), idx, n), _seg_sum64(c_e.double().abs(), idx, n)
    e_y, e_dt = (y.detach().cpu().double() - want_y).abs(), (t.grad.cpu().double() - want_dt).abs()
    print(f"\nscatter_sum/gather {kind} width={width}: forward {float(e_y.max()):.3g}, gather backward {float(e_dt.max()):.3g}")
    assert y.shape == (n, width) and bool((e_y <= SUM_REL * room_y).all())                   # (empty segments: exactly 0)
    assert torch.equal(r.detach().cpu(), table[idx])                                          # a gather does no arithmetic ...
    assert torch.equal(s.grad.cpu(), c_n[idx])                                                # ... nor does the backward of a sum
    assert bool((e_dt <= SUM_REL * room_dt).all())


@pytest.mark.parametrize("kind,width,scale", [(k, 16, s) for k in KINDS for s in (1.0, 30.0, 1000.0)] + [("sorted", w, 1.0) for w in (3, 48, 128)])
def test_scatter_softmax_over_a_plan(kind, width, scale):
    idx, n, check = _index(kind, seed=1)
    plan = _plan(idx, n, check)
    g = torch.Generator().manual_seed(int(scale) + width)
    x = torch.randn(idx.numel(), width, generator=g) * scale
    c = torch.randn(idx.numel(), width, generator=g)
    xd = x.to(_dev()).requires_grad_(True)
    y = training.scatter_softmax(xd, plan)
    (y * c.to(_dev())).sum().backward()
    x64 = x.double().requires_grad_(True)
    want = _softmax64(x64, idx, n)
    (want * c.double()).sum().backward()
    e_y, e_g = float((y.detach().cpu().double() - want.detach()).abs().max()), float((xd.grad.cpu().double() - x64.grad).abs().max())
    print(f"\nscatter_softmax {kind} width={width} logits x {scale:g}: forward {e_y:.3g}, backward {e_g:.3g}")
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(xd.grad).all())
    assert e_y < SOFTMAX_TOL and e_g < GRAD_TOL


def _member_mask(idx, n, g):
    """Real members of each segment: a random half, but segment 3 without any real member, segment 2 with one and segment 4
    with all (sizes 32, 31, 33 of SIZES)."""
    real = torch.rand(idx.numel(), generator=g) < 0.5
    real[idx == 3] = False
    real[idx == 2] = False
    real[(idx == 2).nonzero()[0]] = True
    real[idx == 4] = True
    return real


@pytest.mark.parametrize("kind", ["sorted", "unsorted"])
def test_scatter_softmax_with_masked_members(kind):
    """Members set to -1e30 as _attention sets padding members, one segment without any real member: the result is finite, and
    after the mask multiply the masked members' forward and gradient are exactly zero; the real members follow the float64
    softmax over the real members alone."""
    idx, n, check = _index(kind, seed=2)
    plan = _plan(idx, n, check)
    g = torch.Generator().manual_seed(7)
    real = _member_mask(idx, n, g)
    x, c = torch.randn(idx.numel(), 16, generator=g) * 3, torch.randn(idx.numel(), 16, generator=g)
    xd, rd = x.to(_dev()).requires_grad_(True), real.to(_dev())
    masked = torch.where(rd.unsqueeze(-1), xd, torch.full_like(xd, -1e30))
    y_raw = training.scatter_softmax(masked, plan)
    y = y_raw * rd.unsqueeze(-1).float()
    (y * c.to(_dev())).sum().backward()
    assert bool(torch.isfinite(y_raw).all()) and bool(torch.isfinite(xd.grad).all())
    assert bool((y.detach().cpu()[~real] == 0).all()) and bool((xd.grad.cpu()[~real] == 0).all())
    x64 = x[real].double().requires_grad_(True)
    want = _softmax64(x64, idx[real], n)
    (want * c[real].double()).sum().backward()
    e_y = float((y.detach().cpu()[real].double() - want.detach()).abs().max())
    e_g = float((xd.grad.cpu()[real].double() - x64.grad).abs().max())
    print(f"\nmasked scatter_softmax {kind}: forward {e_y:.3g}, backward {e_g:.3g}")
    assert e_y < SOFTMAX_TOL and e_g < GRAD_TOL


def test_gather_rejects_a_plan_of_another_table_height():
    idx, n, _ = _index("sorted")
    plan = _plan(idx, n, True)
    t = torch.randn(n + 2, 16, device=_dev(), requires_grad=True)
    rows = training.gather(t, plan)                          # (the forward is a plain index_select: every index is in range)
    with pytest.raises(RuntimeError, match="another table height"):
        rows.sum().backward()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind", ["sorted", "knn_src"])
def test_attention_and_aggregation_as_the_network_forms_them(kind, masked):
    """alpha = _attention(gather(q, plan), k, plan[, member_real]) (16 heads x 8) and out = scatter_sum(alpha . v) against the
    float64 softmax over the real members only: alpha, out and the gradients with respect to q (through q_e), k and v."""
    idx, n, check = _index(kind, seed=3)
    plan = _plan(idx, n, check)
    g = torch.Generator().manual_seed(11)
    E = idx.numel()
    real = _member_mask(idx, n, g) if masked else torch.ones(E, dtype=torch.bool)
    q, k, v = torch.randn(n, 128, generator=g), torch.randn(E, 128, generator=g), torch.randn(E, 128, generator=g)
    c = torch.randn(n, 128, generator=g)
    qd, kd, vd = (t.to(_dev()).requires_grad_(True) for t in (q, k, v))
    alpha = training._attention(training.gather(qd, plan), kd, plan, member_real=real.to(_dev()) if masked else None)
    out = training.scatter_sum((alpha.unsqueeze(-1) * vd.view(-1, 16, 8)).reshape(-1, 128), plan)
    (out * c.to(_dev())).sum().backward()
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    score = (q64[idx].view(-1, 16, 8) * k64.view(-1, 16, 8)).sum(-1) / 8 ** 0.5
    a64 = torch.zeros(E, 16, dtype=torch.float64).index_put((real.nonzero().squeeze(1),), _softmax64(score[real], idx[real], n))
    want = _seg_sum64((a64.unsqueeze(-1) * v64.view(-1, 16, 8)).reshape(-1, 128), idx, n)
    (want * c.double()).sum().backward()
    errs = dict(alpha=float((alpha.detach().cpu().double() - a64.detach()).abs().max()),
                out=float((out.detach().cpu().double() - want.detach()).abs().max()),
                dq=float((qd.grad.cpu().double() - q64.grad).abs().max()), dk=float((kd.grad.cpu().double() - k64.grad).abs().max()),
                dv=float((vd.grad.cpu().double() - v64.grad).abs().max()))
    print(f"\n_attention {kind} masked={masked}:", {a: f"{b:.2g}" for a, b in errs.items()})
    assert all(bool(torch.isfinite(t).all()) for t in (alpha, out, qd.grad, kd.grad, vd.grad))
    if masked:
        assert bool((alpha.detach().cpu()[~real] == 0).all()) and bool((kd.grad.cpu()[~real] == 0).all()) and bool((vd.grad.cpu()[~real] == 0).all())
        assert bool((out.detach().cpu()[3] == 0).all())      # the segment without a real member contributes nothing
    assert errs["alpha"] < SOFTMAX_TOL and max(errs["out"], errs["dq"], errs["dk"], errs["dv"]) < GRAD_TOL, errs


# --------------------------------------------------------------------------------- Linear layers on column slices of a wider weight
WIDE = 437                                                   # the widest first Linear (bond_layer: 128 + 20 + 20 + 13 + 128 + 128)
SLICES_128 = [(84, 212), (212, 340), (128, 256), (256, 384), (0, 128), (181, 309), (309, 437)]
SLICES_FEAT = [(0, 84), (128, 148), (148, 168), (168, 181)]
ROWS = [1, 33, 264, 2640, 3584]
_rel = lambda a, w: float((a.double().cpu() - w).abs().max() / w.abs().max().clamp(min=1e-30))


def _slice_grad_lands(W, a, b, want_dW):
    """W.grad: the float64 gradient in columns [a:b], exactly zero elsewhere."""
    gW = W.grad.cpu()
    outside = torch.ones(WIDE, dtype=torch.bool)
    outside[a:b] = False
    assert bool((gW[:, outside] == 0).all()), (a, b)
    return _rel(gW[:, a:b], want_dW)


@pytest.mark.parametrize("rows", ROWS)
def test_linear128_on_column_slices_of_a_wider_weight(rows):
    g = torch.Generator().manual_seed(rows)
    for a, b in SLICES_128:
        x = torch.randn(rows, 128, generator=g)
        W, bias = torch.randn(128, WIDE, generator=g) * 0.1, torch.randn(128, generator=g)
        dy = torch.randn(rows, 128, generator=g)
        xd, Wd, bd = (t.to(_dev()).requires_grad_(True) for t in (x, W, bias))
        y = training.linear128(xd, Wd[:, a:b], bd)
        y.backward(dy.to(_dev()))
        Ws = W[:, a:b].double()
        errs = dict(y=_rel(y.detach(), x.double() @ Ws.t() + bias.double()), dx=_rel(xd.grad, dy.double() @ Ws),
                    dW=_slice_grad_lands(Wd, a, b, dy.double().t() @ x.double()), db=_rel(bd.grad, dy.double().sum(0)))
        print(f"\nlinear128 rows={rows} W[:, {a}:{b}]:", {k: f"{v:.2g}" for k, v in errs.items()})
        assert max(errs.values()) < GEMM_REL, (a, b, errs)


@pytest.mark.parametrize("rows", ROWS)
def test_linear_feat_on_column_slices_of_a_wider_weight(rows):
    g = torch.Generator().manual_seed(rows + 1)
    for a, b in SLICES_FEAT:
        f = torch.rand(rows, b - a, generator=g)
        W = torch.randn(128, WIDE, generator=g) * 0.1
        dy = torch.randn(rows, 128, generator=g)
        fd, Wd = (t.to(_dev()).requires_grad_(True) for t in (f, W))
        y = training.linear_feat(fd, Wd[:, a:b])
        y.backward(dy.to(_dev()))
        Ws = W[:, a:b].double()
        errs = dict(y=_rel(y.detach(), f.double() @ Ws.t()), df=_rel(fd.grad, dy.double() @ Ws),
                    dW=_slice_grad_lands(Wd, a, b, dy.double().t() @ f.double()))
        print(f"\nlinear_feat rows={rows} W[:, {a}:{b}]:", {k: f"{v:.2g}" for k, v in errs.items()})
        assert max(errs.values()) < GEMM_REL, (a, b, errs)


# --------------------------------------------------------------------------------- dd_gemm128_tn beyond the call of training.py
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("M", [5, 16, 64, 84, 128])
def test_gemm128_tn_accumulates_into_a_strided_output(M, bias):
    """out[M, 128] += A^T X with accumulate = 1 into a non-zero out whose rows lie ldo = 136 apart, A rows lda > M apart (one
    pitch that keeps the 16-byte loads, one that does not; the gap holds NaN: it must never be read) and X rows 132 apart.
    200 rows: four slabs, the last of 8 rows.  The gap columns of out stay as they were, bit for bit."""
    lib, d = hip_lib.load(), _dev()
    rows, ldx, ldo = 200, 132, 136
    g = torch.Generator().manual_seed(M)
    for lda in (M + 3, (M + 3) // 4 * 4 + 4):
        A = torch.full((rows, lda), float("nan"))
        A[:, :M] = torch.randn(rows, M, generator=g)
        X = torch.randn(rows, ldx, generator=g)
        out0 = torch.randn(M, ldo, generator=g)
        Ad, Xd, out = A.to(d), X.to(d), out0.to(d)
        n_scratch = int(lib.dd_gemm128_tn_scratch_floats(rows, M))
        assert n_scratch >= 4 * 32 * 128
        scratch = torch.zeros(n_scratch, device=d)
        st = hip_lib.stream_ptr(d)
        if bias:
            db = torch.full((M,), float("nan"), device=d)
            rc = lib.dd_gemm128_tn_bias(hip_lib.ptr(Ad), lda, M, hip_lib.ptr(Xd), ldx, rows, hip_lib.ptr(scratch), hip_lib.ptr(out), ldo, 1,
                                        hip_lib.ptr(db), st)
        else:
            rc = lib.dd_gemm128_tn(hip_lib.ptr(Ad), lda, M, hip_lib.ptr(Xd), ldx, rows, hip_lib.ptr(scratch), hip_lib.ptr(out), ldo, 1, st)
        hip_lib.check(rc, "dd_gemm128_tn")
        torch.cuda.synchronize()
        got = out.cpu()
        want = out0[:, :128].double() + A[:, :M].double().t() @ X[:, :128].double()
        err = _rel(got[:, :128], want)
        print(f"\ndd_gemm128_tn{'_bias' if bias else ''} M={M} lda={lda}: {err:.2g}")
        assert torch.equal(got[:, 128:], out0[:, 128:]), "the gap columns of out were written"
        assert err < GEMM_REL, (M, lda, err)
        if bias:
            assert _rel(db, A[:, :M].double().sum(0)) < GEMM_REL
        # accumulate = 0 over the same buffer: the product alone, the gap columns still untouched
        rc = lib.dd_gemm128_tn(hip_lib.ptr(Ad), lda, M, hip_lib.ptr(Xd), ldx, rows, hip_lib.ptr(scratch), hip_lib.ptr(out), ldo, 0, st)
        hip_lib.check(rc, "dd_gemm128_tn")
        torch.cuda.synchronize()
        got = out.cpu()
        assert torch.equal(got[:, 128:], out0[:, 128:]) and _rel(got[:, :128], A[:, :M].double().t() @ X[:, :128].double()) < GEMM_REL
