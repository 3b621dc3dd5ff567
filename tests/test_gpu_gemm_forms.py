"""GPU (-m gpu): every job form of the batched projection GEMM (launch_gemm128_batch, through dd_debug_gemm128_batch) at op level.
Jobs without the LayerNorm prologue must reproduce gemm_cases.expected_bits BIT FOR BIT -- a wrong row, column or addend, a
swapped bias / accumulate order or another summation order all fail it; LayerNorm jobs are held to float64 at the kernel's
project bound.  Around that: memory outside a job's window stays untouched, a NaN / Inf row stays in its row, a batch equals its
jobs launched alone, what the tile cannot address is refused, and the measurement build's tile variants give the same bits.
Every test prints what it measured (run with -s)."""
import numpy as np
import pytest
import torch

import gemm_cases as GC
from decompdiff_amd import hip_lib

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def upload(case, override=None):
    T = dict(case["tensors"], **(override or {}))
    d = {n: torch.from_numpy(t).to(dev()) for n, t in T.items()}
    return d, {n: t.data_ptr() for n, t in d.items()}


def outputs_of(jobs):
    return sorted({j["Y"][0] for j in jobs} | {j["acc_src"] for j in jobs if j["acc_src"]})


def launch(case, jobs=None, override=None, expect_ok=True, single_entry=False):
    """Fresh upload, ONE launch of `jobs` (default: all of the case's), download of every Y / acc_src tensor of the CASE."""
    lib = hip_lib.load()
    jobs = case["jobs"] if jobs is None else jobs
    d, base = upload(case, override)
    if single_entry:
        (job,) = jobs
        rc = lib.dd_gemm128(*GC.dd_gemm128_args(job, base), hip_lib.stream_ptr())
    else:
        rc = lib.dd_debug_gemm128_batch(GC.job_array(jobs, base), len(jobs), hip_lib.stream_ptr())
    torch.cuda.synchronize()
    if expect_ok:
        hip_lib.check(rc, "gemm launch")
    return rc, {n: d[n].cpu().numpy() for n in outputs_of(case["jobs"])}


_RUNS = {}


def run(case):
    if case["name"] not in _RUNS:
        _RUNS[case["name"]] = launch(case)[1]
    return _RUNS[case["name"]]


def same_bits(a, b):
    return torch.equal(torch.tensor(np.ascontiguousarray(a).view(np.int32)), torch.tensor(np.ascontiguousarray(b).view(np.int32)))


def check_bits(case, ji, out, tag=""):
    job, ref = case["jobs"][ji], GC.reference(case, ji)
    got = GC.read_window(out[job["Y"][0]], job)
    frac = float((np.abs(got.astype(np.float64) - ref["y64"]) / ref["bound"]).max())
    n_bad = int((got.view(np.int32) != ref["bits"].view(np.int32)).sum())
    print(f"\n{case['name']}{tag} job {ji}: {got.size} elements compared, {n_bad} differ in a bit, worst |y - y64| / bound {frac:.3f}")
    assert same_bits(got, ref["bits"]), f"{n_bad} of {got.size} elements differ from the fma chain"


def check_ln(case, ji, out, tag=""):
    job, ref = case["jobs"][ji], GC.reference(case, ji)
    got = GC.read_window(out[job["Y"][0]], job)
    err = float(np.abs(got.astype(np.float64) - ref["y64"]).max())
    bound = GC.ln_bound(ref["d32"])
    print(f"\n{case['name']}{tag} job {ji}: {got.size} elements, max |y - y64| {err:.3g}, fp32 torch is {ref['d32']:.3g} from float64, bound {bound:.3g}")
    assert err <= bound


def check_untouched(case, out, launched=None):
    """Everything outside the launched jobs' windows is bit-identical to what was uploaded; acc_src buffers are unchanged."""
    launched = case["jobs"] if launched is None else launched
    for name in outputs_of(case["jobs"]):
        m = np.zeros(case["tensors"][name].shape, bool)
        for job in launched:
            if job["Y"][0] == name:
                m |= GC.written_mask(case, job)
        assert same_bits(out[name][~m], case["tensors"][name][~m]), f"{case['name']}: {name} changed outside the written windows"


def _groups():
    return [pytest.param(GC.plain_group(*gk), id="plain-r%d-c%d-%s" % gk) for gk in GC.plain_groups()] + \
           [pytest.param([n], id=n) for n in GC.other_bit_cases()]


@pytest.mark.parametrize("names", _groups())
def test_bits_of_every_form(names):
    for name in names:
        case = GC.cases()[name]
        check_bits(case, 0, run(case))


@pytest.mark.parametrize("name", GC.ln_cases())
def test_layernorm_forms(name):
    case = GC.cases()[name]
    check_ln(case, 0, run(case))


@pytest.mark.parametrize("names", _groups() + [pytest.param([n], id=n) for n in GC.ln_cases()])
def test_untouched_memory(names):
    """Random canaries in Y and acc_src: the gaps between Y row blocks, the columns beside the window and past ncols in a
    partial tile, and all of acc_src keep their bits."""
    for name in names:
        case = GC.cases()[name]
        check_untouched(case, run(case))
        job = case["jobs"][0]
        assert GC.written_mask(case, job).sum() == job["rows"] * job["ncols"] <= case["tensors"][job["Y"][0]].size


# ------------------------------------------------------------------------------------------------ batches
@pytest.mark.parametrize("njobs", [1, 2, 3, 4, 5, 6])
def test_batch_prefix(njobs):
    """The first njobs of the six-job batch in one launch: each against its reference, the buffers of the others untouched."""
    full = GC.batch_case()
    case = GC.batch_prefix(njobs)
    _, out = launch(full, jobs=case["jobs"])
    for ji, job in enumerate(case["jobs"]):
        (check_bits if job["ln"] is None else check_ln)(full, ji, out, tag=f"[:{njobs}]")
    check_untouched(full, out, launched=case["jobs"])


def test_launch_independence():
    """The six-job batch == six single-job launches == dd_gemm128 where it can express the job, bit for bit; and twice the same."""
    full = GC.batch_case()
    _, a = launch(full)
    _, b = launch(full)
    for name in a:
        assert same_bits(a[name], b[name]), name
    n_single = 0
    for ji, job in enumerate(full["jobs"]):
        _, alone = launch(full, jobs=[job])
        assert same_bits(GC.read_window(alone[job["Y"][0]], job), GC.read_window(a[job["Y"][0]], job)), f"job {ji} alone"
        check_untouched(full, alone, launched=[job])
        if GC.dd_gemm128_args(job, {n: 0 for n in full["tensors"]}) is not None:
            _, one = launch(full, jobs=[job], single_entry=True)
            assert same_bits(GC.read_window(one[job["Y"][0]], job), GC.read_window(a[job["Y"][0]], job)), f"job {ji} through dd_gemm128"
            n_single += 1
    print(f"\nbatch of 6 == 6 launches of one job; {n_single} of them also through dd_gemm128")
    assert n_single == 3


# ------------------------------------------------------------------------------------------------ isolation
def _poisoned_rows(case, job, tensor, start):
    """Output rows whose input (X or X2 row) starts at `start` of `tensor`."""
    hit = np.zeros(job["rows"], bool)
    if job["X"][0] == tensor:
        hit |= GC.x_starts(job) == start
    if job["X2"] is not None and job["X2"][0] == tensor:
        hit |= GC.x2_starts(job) == start
    return hit


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
@pytest.mark.parametrize("name,which,row", [("ln-plain-near1", "X", 40), ("ln-rowblock-xy-mixed", "X", 300), ("x2-ligand-s1", "X2", 7),
                                            ("x2-all-nodes-s1", "X2", 20), ("ln-bond-nl9-near1", "X2", 11)])
def test_poison_stays_in_its_row(name, which, row, value):
    """One input row (of X, or of the addend X2 -- a bond-form addend row feeds NL - 1 output rows) set to NaN / Inf: those
    output rows are non-finite, every other output bit is what the clean run gave."""
    case = GC.cases()[name]
    job = case["jobs"][0]
    clean = run(case)
    tensor = job[which][0]
    starts = GC.x_starts(job) if which == "X" else GC.x2_starts(job)
    start = int(starts[starts >= 0][row]) if which == "X" else int(np.unique(starts[starts >= 0])[row])
    bad = case["tensors"][tensor].copy()
    bad[start:start + 128] = value
    _, out = launch(case, override={tensor: bad})
    hit = _poisoned_rows(case, job, tensor, start)
    got, ref = GC.read_window(out[job["Y"][0]], job), GC.read_window(clean[job["Y"][0]], job)
    print(f"\n{name} {which} row {row} = {value}: {int(hit.sum())} output rows poisoned, non-finite there: {int((~np.isfinite(got[hit])).sum())} of {got[hit].size}")
    assert hit.sum() == (job["x2_NLm1"] if job["x2_Eb"] > 0 and which == "X2" else 1)
    assert not np.isfinite(got[hit]).any()
    assert same_bits(got[~hit], ref[~hit])
    check_untouched(case, out)


# ------------------------------------------------------------------------------------------------ refusals
def _refusals():
    P, L, N2, BD = "plain-r65-c70-b1-src-s1", "ln-plain-near1", "x2-all-nodes-s1", "ln-bond-nl9-near1"

    def field(name, value):
        return lambda j: setattr(j, name, value)

    def shift(name, nbytes=4):
        return lambda j: setattr(j, name, getattr(j, name) + nbytes)
    return [("njobs 0", P, None, 0), ("njobs 7", P, None, 7),
            ("X null", P, field("X", None), 1), ("W null", P, field("W", None), 1), ("Y null", P, field("Y", None), 1),
            ("X misaligned", P, shift("X"), 1), ("W misaligned", P, shift("W"), 1), ("ln misaligned", L, shift("ln"), 1),
            ("X2 misaligned", N2, shift("X2"), 1), ("bias misaligned", P, shift("bias"), 1), ("acc_src misaligned", P, shift("acc_src"), 1),
            ("ldx % 4", P, field("ldx", 258), 1), ("x_stride_b % 4", P, field("x_stride_b", 2), 1), ("x2_ld % 4", BD, field("x2_ld", 1282), 1),
            ("rows 0", P, field("rows", 0), 1), ("rows < 0", P, field("rows", -1), 1), ("ncols 0", P, field("ncols", 0), 1),
            ("x_rows_per_b 0", P, field("x_rows_per_b", 0), 1), ("y_rows_per_b 0", P, field("y_rows_per_b", 0), 1),
            ("node form x2_N == x2_NP", N2, field("x2_NP", GC.N5), 1), ("node form x2_NP < 0", N2, field("x2_NP", -1), 1),
            ("bond form x2_NLm1 0", BD, field("x2_NLm1", 0), 1), ("bond form x2_Eb % x2_NLm1", BD, field("x2_NLm1", 7), 1)]


def test_refusals():
    """What the tile cannot address comes back as a negative status before anything is launched: Y keeps its bits."""
    lib = hip_lib.load()
    for what, name, mutate, njobs in _refusals():
        case = GC.cases()[name]
        d, base = upload(case)
        good = GC.to_ctypes(case["jobs"][0], base)
        arr = (hip_lib.DDGemmJob * 7)(*[good] * 7)
        if mutate is not None:
            mutate(arr[0])
        rc = lib.dd_debug_gemm128_batch(arr, njobs, hip_lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc < 0, what
        for n in outputs_of(case["jobs"]):
            assert same_bits(d[n].cpu().numpy(), case["tensors"][n]), what
    assert lib.dd_debug_gemm128_batch(None, 1, hip_lib.stream_ptr()) < 0
    print(f"\n{len(_refusals()) + 1} malformed calls refused, Y untouched")


# ------------------------------------------------------------------------------------------------ measurement build
@pytest.mark.parametrize("key", [1, 21])
def test_tile_variants_reproduce_the_bits(debug_options, key):
    """dd_debug_set_option(1, 0): the unsplit tile; (21, 0): no XCD-aware tile order.  Every case the variant supports gives the
    bits of the default path (jobs without LayerNorm: the fma chain itself; LayerNorm jobs: the default path's run in this
    process); the unsplit tile has no bond-form addend and the entry point refuses it."""
    if not debug_options:
        return
    lib = hip_lib.load()
    bond = [n for n, c in GC.cases().items() if c["jobs"][0]["x2_Eb"] > 0]
    names = [n for n in GC.cases() if not (key == 1 and n in bond)]
    ln_default = {n: run(GC.cases()[n]) for n in GC.ln_cases()}
    batch_default = launch(GC.batch_case())[1] if key == 21 else None
    compared = 0
    assert lib.dd_debug_set_option(key, 0) == 0
    try:
        for name in names:
            case = GC.cases()[name]
            job = case["jobs"][0]
            _, out = launch(case)
            got = GC.read_window(out[job["Y"][0]], job)
            want = GC.reference(case)["bits"] if job["ln"] is None else GC.read_window(ln_default[name][job["Y"][0]], job)
            assert same_bits(got, want), name
            check_untouched(case, out)
            compared += got.size
        if key == 1:
            for name in bond:
                rc, out = launch(GC.cases()[name], expect_ok=False)
                assert rc < 0, name
                check_untouched(GC.cases()[name], out, launched=[])
        else:
            _, out = launch(GC.batch_case())
            for n in out:
                assert same_bits(out[n], batch_default[n]), n
    finally:
        assert lib.dd_debug_set_option(key, 1) == 0
    print(f"\noption {key} = 0: {len(names)} cases, {compared} elements bit-identical" + (f", {len(bond)} bond-form jobs refused" if key == 1 else ""))
