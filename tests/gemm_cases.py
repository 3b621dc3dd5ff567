"""Every job form of the batched projection GEMM (csrc/dd_gemm.hip: launch_gemm128_batch, reached through
dd_debug_gemm128_batch) as data, with two restatements of what a job computes.  A plain helper module (no tests):
tests/test_gemm_cases_host.py checks the restatements and the case builder on the CPU, tests/test_gpu_gemm_forms.py runs
the kernel.

A CASE is {"name", "tensors": {name: flat float32 numpy array}, "jobs": [job, ...]}.  A JOB names tensors and windows into them
(all offsets and strides in floats):
    X  = (tensor, offset), x_rows_per_b, x_stride_b, ldx, rows       W, bias, ln = tensor names (bias / ln may be None)
    Y  = (tensor, offset), y_rows_per_b, y_stride_b, ldy, ncols      accumulate, acc_src = tensor name or None (Y's window)
    X2 = (tensor, offset) or None, x2_N, x2_NP, x2_Eb, x2_NLm1, x2_ld
Row maps are written out as nested loops over samples and rows (x_starts, y_starts, x2_starts), not as the kernel's
div / mod arithmetic.

expected_bits(case, job): the bits the kernel must produce for a job without the LayerNorm prologue.  The tile multiplies
with v_mfma_f32_32x32x2_f32, which is bitwise a chain of fp32 fmaf in the order of its two k slots; the tile feeds the k slots of
one instruction from the columns (4 i, 4 i + 2) and of the next from (4 i + 1, 4 i + 3) (lane half hh reads the float2 at column
4 i + 2 hh), so the chain of an output element runs over K_ORDER = 0, 2, 1, 3, 4, 6, 5, 7, ... -- the same for the unsplit and the
K-split tile, for every job, launch order and position in a batch:
    x = X row (+ X2 row: one fp32 add);  acc = 0;  acc = fma32(x[k], w[k], acc) for k in K_ORDER;  + bias;  + old   (fp32 adds)
expected64(case, job): the same expression in float64, the LayerNorm + ReLU prologue (eps 1e-5, biased variance, the X2 sum taken
first) included, and the per-element bound  g (|x| . |w| + |bias| + |old|),  g = n u / (1 - n u), u = 2^-24, n = 130: the textbook
bound of a 128-term fma chain plus the two adds behind it (the X2 add of a job that has one is a 131st rounding, 0.8 % of the
bound, which the measured fractions -- a few per cent of it -- do not come near)."""
import ctypes
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

K = 128
K_ORDER = tuple(4 * (k // 4) + (0, 2, 1, 3)[k % 4] for k in range(K))
U = 2.0 ** -24
N_ROUNDINGS = 130
GAMMA = N_ROUNDINGS * U / (1.0 - N_ROUNDINGS * U)
LN_EPS = 1e-5
LN_TOL = 2e-5            # the project's bound for this kernel at X ~ N(0,1), W ~ N(0,1)/11.3 (test_gpu_parity.test_gemm128)
F32_MIN_NORMAL = 2.0 ** -126


# ================================================================================================== exact fp32 FMA
def fma32(a, b, c):
    """round_to_fp32(a * b + c) with ONE rounding, for float32 arrays (results in the normal range or 0; finite inputs).
    The product of two fp32 is exact in float64; s = fl64(p + c) with its rounding error e (TwoSum); fp32(s) is the answer
    unless s sits exactly on the midpoint of two neighbouring fp32 (low 29 mantissa bits 1 0...0) with e != 0, where the
    sign of e says on which side of the midpoint the true sum lies."""
    a, b, c = np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32)
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    s = p + c64
    p, c64 = np.broadcast_to(p, s.shape), np.broadcast_to(c64, s.shape)
    r = s.astype(np.float32)
    tie = (s.view(np.int64) & 0x1FFFFFFF) == 0x10000000
    if tie.any():
        bb = s - p
        e = (p - (s - bb)) + (c64 - bb)
        idx = np.nonzero(tie & (e != 0.0))
        if idx[0].size:
            st, et = s[idx], e[idx]
            r = r.copy()
            r0 = r[idx]
            lo = np.where(r0.astype(np.float64) < st, r0, np.nextafter(r0, np.float32(-np.inf)))
            hi = np.where(r0.astype(np.float64) > st, r0, np.nextafter(r0, np.float32(np.inf)))
            r[idx] = np.where(et > 0.0, hi, lo)
    mag = np.abs(s)
    assert not ((mag < F32_MIN_NORMAL) & (mag > 0.0)).any(), "fma32: subnormal result (outside what the cases cover)"
    return r


# ================================================================================================== row maps, written out
def x_starts(job):
    """Offset (floats, into the X tensor) of the first input column of every logical row."""
    out, off = [], job["X"][1]
    b = 0
    while len(out) < job["rows"]:
        for i in range(job["x_rows_per_b"]):
            if len(out) == job["rows"]:
                break
            out.append(off + b * job["x_stride_b"] + i * job["ldx"])
        b += 1
    return np.asarray(out, np.int64)


def y_starts(job):
    out, off = [], job["Y"][1]
    b = 0
    while len(out) < job["rows"]:
        for i in range(job["y_rows_per_b"]):
            if len(out) == job["rows"]:
                break
            out.append(off + b * job["y_stride_b"] + i * job["ldy"])
        b += 1
    return np.asarray(out, np.int64)


def x2_starts(job):
    """Offset into the X2 tensor of the addend of every logical row, -1 where a row has none."""
    if job.get("X2") is None:
        return None
    out, off = [], job["X2"][1]
    rows = job["rows"]
    if job["x2_Eb"] > 0:                       # bond rows, grouped by sample, then by destination atom (x2_NLm1 bonds each)
        sample = 0
        while len(out) < rows:
            for atom in range(job["x2_Eb"] // job["x2_NLm1"]):
                for _ in range(job["x2_NLm1"]):
                    if len(out) < rows:
                        out.append(off + (sample * job["x2_N"] + atom) * job["x2_ld"])
            sample += 1
    else:                                      # node rows: the x2_N - x2_NP last nodes of every sample, X2 rows packed, 128 apart
        packed = 0
        while len(out) < rows:
            for n in range(job["x2_N"]):
                if len(out) == rows:
                    break
                if n >= job["x2_NP"]:
                    out.append(off + packed * K)
                    packed += 1
                else:
                    out.append(-1)
    return np.asarray(out, np.int64)


def _gather(flat, starts, width):
    return flat[starts[:, None] + np.arange(width)[None, :]]


def inputs(case, job):
    """(X rows [rows,128], X2 rows or None (zeros where a row has no addend), W [ncols,128], bias or None, ln or None, old or None)."""
    T = case["tensors"]
    X = _gather(T[job["X"][0]], x_starts(job), K)
    X2 = None
    s2 = x2_starts(job)
    if s2 is not None:
        X2 = np.where((s2 >= 0)[:, None], _gather(T[job["X2"][0]], np.maximum(s2, 0), K), np.float32(0.0))
    W = T[job["W"]].reshape(-1, K)[:job["ncols"]]
    bias = None if job["bias"] is None else T[job["bias"]][:job["ncols"]]
    ln = None if job["ln"] is None else T[job["ln"]].reshape(2, K)
    old = None
    if job["accumulate"]:
        old = _gather(T[job["acc_src"] if job["acc_src"] else job["Y"][0]], y_starts(job), job["ncols"])
    return X, X2, W, bias, ln, old


def expected_bits(case, job, k_order=K_ORDER):
    assert job["ln"] is None, "bit-exact restatement exists for jobs without the LayerNorm prologue"
    X, X2, W, bias, _, old = inputs(case, job)
    x = X if X2 is None else np.where(x2_starts(job)[:, None] >= 0, X + X2, X)        # (float32 + float32: one fp32 add)
    assert x.dtype == np.float32
    acc = np.zeros((job["rows"], job["ncols"]), np.float32)
    Wt = np.ascontiguousarray(W.T)

    def chain(r0):                                            # (row chunks: the working set of a chain stays in cache)
        a = acc[r0:r0 + 64]
        for k in k_order:
            a = fma32(x[r0:r0 + 64, k, None], Wt[None, k, :], a)
        acc[r0:r0 + 64] = a
    with ThreadPoolExecutor(max_workers=8) as ex:             # (numpy releases the GIL: the chunks of a large case run side by side)
        list(ex.map(chain, range(0, job["rows"], 64)))
    if bias is not None:
        acc = acc + bias[None, :]
    if old is not None:
        acc = acc + old
    assert acc.dtype == np.float32
    return acc


def prologue64(case, job):
    X, X2, _, _, ln, _ = inputs(case, job)
    x = X.astype(np.float64)
    if X2 is not None:
        x = x + X2.astype(np.float64)
    if ln is not None:
        mean = x.mean(1, keepdims=True)
        var = ((x - mean) ** 2).mean(1, keepdims=True)
        x = np.maximum((x - mean) / np.sqrt(var + LN_EPS) * ln[0].astype(np.float64) + ln[1].astype(np.float64), 0.0)
    return x


def expected64(case, job):
    """(float64 result [rows, ncols], per-element bound of the GEMM part)."""
    _, _, W, bias, _, old = inputs(case, job)
    x = prologue64(case, job)
    w = W.astype(np.float64)
    y = x @ w.T
    mag = np.abs(x) @ np.abs(w).T
    if bias is not None:
        y = y + bias.astype(np.float64)
        mag = mag + np.abs(bias.astype(np.float64))
    if old is not None:
        y = y + old.astype(np.float64)
        mag = mag + np.abs(old.astype(np.float64))
    return y, GAMMA * mag


def torch32(case, job):
    """The expression of expected64 as plain fp32 torch statements on the CPU (for the distance fp32 itself keeps from float64)."""
    import torch
    X, X2, W, bias, ln, old = inputs(case, job)
    x = torch.from_numpy(np.ascontiguousarray(X))
    if X2 is not None:
        x = x + torch.from_numpy(np.ascontiguousarray(X2))
    if ln is not None:
        lnt = torch.from_numpy(np.ascontiguousarray(ln))
        x = torch.relu(torch.nn.functional.layer_norm(x, (K,), lnt[0], lnt[1], LN_EPS))
    y = x @ torch.from_numpy(np.ascontiguousarray(W)).t()
    if bias is not None:
        y = y + torch.from_numpy(np.ascontiguousarray(bias))
    if old is not None:
        y = y + torch.from_numpy(np.ascontiguousarray(old))
    return y.numpy()


def ln_bound(d32):
    """stress_weights.bound: the flat project tolerance while fp32 torch itself stays within a quarter of it, else twice its distance."""
    return LN_TOL if d32 <= 0.25 * LN_TOL else max(LN_TOL, 2.0 * d32)


def written_mask(case, job):
    """Boolean mask over the Y tensor: the elements the job writes."""
    m = np.zeros(case["tensors"][job["Y"][0]].shape, bool)
    m[y_starts(job)[:, None] + np.arange(job["ncols"])[None, :]] = True
    return m


def read_window(flat, job):
    return _gather(np.asarray(flat), y_starts(job), job["ncols"])


# ================================================================================================== ctypes side
_PTR_BYTES = 4


def to_ctypes(job, base):
    """The dd_gemm_job of a job; base: tensor name -> device address of its first float."""
    from decompdiff_amd import hip_lib
    j = hip_lib.DDGemmJob()

    def at(ref):
        return None if ref is None else base[ref[0]] + _PTR_BYTES * ref[1]
    j.X, j.x_rows_per_b, j.x_stride_b, j.ldx, j.rows = at(job["X"]), job["x_rows_per_b"], job["x_stride_b"], job["ldx"], job["rows"]
    j.W = base[job["W"]]
    j.bias = None if job["bias"] is None else base[job["bias"]]
    j.ln = None if job["ln"] is None else base[job["ln"]]
    j.Y, j.y_rows_per_b, j.y_stride_b, j.ldy, j.ncols = at(job["Y"]), job["y_rows_per_b"], job["y_stride_b"], job["ldy"], job["ncols"]
    j.accumulate = int(job["accumulate"])
    j.acc_src = None if not job["acc_src"] else at((job["acc_src"], job["Y"][1]))
    j.X2 = at(job.get("X2"))
    j.x2_N, j.x2_NP, j.x2_Eb, j.x2_NLm1, j.x2_ld = (job.get(k, 0) for k in ("x2_N", "x2_NP", "x2_Eb", "x2_NLm1", "x2_ld"))
    return j


def job_array(jobs, base):
    from decompdiff_amd import hip_lib
    arr = (hip_lib.DDGemmJob * len(jobs))()
    for i, job in enumerate(jobs):
        arr[i] = to_ctypes(job, base)
    return arr


def dd_gemm128_args(job, base):
    """Argument list of the single-job entry point dd_gemm128 for a job it can express (no X2, no acc_src), else None."""
    if job.get("X2") is not None or job["acc_src"]:
        return None
    c = to_ctypes(job, base)
    return [ctypes.c_void_p(c.X), c.x_rows_per_b, c.x_stride_b, c.ldx, c.rows, ctypes.c_void_p(c.W), ctypes.c_void_p(c.bias),
            ctypes.c_void_p(c.ln), ctypes.c_void_p(c.Y), c.y_rows_per_b, c.y_stride_b, c.ldy, c.ncols, c.accumulate]


# ================================================================================================== the cases
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _randn(g, n, scale=1.0):
    return (g.standard_normal(n) * scale).astype(np.float32)


def _job(**kw):
    job = dict(bias=None, ln=None, accumulate=0, acc_src=None, X2=None, x2_N=0, x2_NP=0, x2_Eb=0, x2_NLm1=0, x2_ld=0)
    job.update(kw)
    return job


def _weights(g, T, pre, ncols, bias, sw=1.0):
    T[pre + "W"] = _randn(g, ncols * K, sw / 11.3)
    if bias:
        T[pre + "bias"] = _randn(g, ncols)
    return pre + "W", (pre + "bias" if bias else None)


def ln_params(g, family, T, pre):
    """[2,128] gamma / beta: family "near1": gamma = 1 +- 0.1;  "mixed": 40 channels negated, 5 exactly zero."""
    gam, bet = 1.0 + 0.1 * g.standard_normal(K), 0.1 * g.standard_normal(K)
    if family == "mixed":
        perm = g.permutation(K)
        gam[perm[:40]] *= -1.0
        gam[perm[40:45]] = 0.0
        assert int((gam < 0).sum()) == 40 and int((gam == 0).sum()) == 5
    T[pre + "ln"] = np.concatenate([gam, bet]).astype(np.float32)
    return pre + "ln"


def _const_rows(case, job, family):
    """mixed family: the first quarter of the rows (at least one) constant over the 128 input channels -- variance 0.  With an
    addend, the addend rows of those X rows are made constant too."""
    if family != "mixed":
        return
    T = case["tensors"]
    n = max(1, job["rows"] // 4)
    xs, s2 = x_starts(job)[:n], x2_starts(job)
    X = T[job["X"][0]]
    for s in xs:
        X[s:s + K] = X[s]
    if s2 is not None:
        X2 = T[job["X2"][0]]
        for s in s2[:n]:
            if s >= 0:
                X2[s:s + K] = X2[s]


def plain_job(g, T, pre, rows, ncols, bias=True, acc="none", ln=None, sx=1.0, sw=1.0, ldy_extra=0, y_off=32):
    """X: columns 64..191 of a 256-wide table; Y: columns y_off.. of a table ncols (rounded up to 4) + 64 (+ ldy_extra) wide."""
    ldy = (ncols + 3) // 4 * 4 + 64 + ldy_extra
    T[pre + "X"] = _randn(g, rows * 256, sx)
    T[pre + "Y"] = _randn(g, rows * ldy)
    W, b = _weights(g, T, pre, ncols, bias, sw)
    if acc == "src":
        T[pre + "S"] = _randn(g, rows * ldy)
    return _job(X=(pre + "X", 64), x_rows_per_b=rows, x_stride_b=0, ldx=256, rows=rows, W=W, bias=b,
                ln=None if ln is None else ln_params(g, ln, T, pre),
                Y=(pre + "Y", y_off), y_rows_per_b=rows, y_stride_b=0, ldy=ldy, ncols=ncols,
                accumulate=int(acc != "none"), acc_src=pre + "S" if acc == "src" else None)


PLAIN_ROWS = (1, 63, 64, 65)
PLAIN_NCOLS = (4, 61, 64, 70, 128)
PLAIN_BIAS = (True, False)
PLAIN_ACC = ("none", "y", "src")
SCALES = {"s1": (1.0, 1.0), "s1e3": (1e3, 1e-3)}
LN_FAMILIES = ("near1", "mixed")
B5, NP5, NL5 = 5, 197, 9
N5 = NP5 + NL5


def _single(name, build):
    g = _rng(name)
    T = {}
    job = build(g, T)
    return {"name": name, "tensors": T, "jobs": [job]}


def xcd_job(g, T, pre, ncols, sx=1.0, sw=1.0, rows=1030):
    """The n1 form: all rows, Y a column window (P + col0) of a 640-wide table."""
    col0 = 640 - ncols if ncols < 640 else 0
    T[pre + "X"] = _randn(g, rows * K, sx)
    T[pre + "Y"] = _randn(g, rows * 640)
    W, b = _weights(g, T, pre, ncols, True, sw)
    return _job(X=(pre + "X", 0), x_rows_per_b=rows, x_stride_b=0, ldx=K, rows=rows, W=W, bias=b,
                Y=(pre + "Y", col0), y_rows_per_b=rows, y_stride_b=0, ldy=640, ncols=ncols)


def rowblock_x_job(g, T, pre, sx=1.0, sw=1.0, x2=False, B=B5, NP=NP5, NL=NL5):
    """The l1 / v_head1 form: the ligand rows h[:, NP:] of every sample -> columns 0..191 of a 1280-wide table; x2: + the
    ligand-only addend (x2_N = NL, x2_NP = 0)."""
    N = NP + NL
    T[pre + "h"] = _randn(g, B * N * K, sx)
    T[pre + "PL"] = _randn(g, B * NL * 1280)
    W, b = _weights(g, T, pre, 192, True, sw)
    job = _job(X=(pre + "h", NP * K), x_rows_per_b=NL, x_stride_b=N * K, ldx=K, rows=B * NL, W=W, bias=b,
               Y=(pre + "PL", 0), y_rows_per_b=B * NL, y_stride_b=0, ldy=1280, ncols=192)
    if x2:
        T[pre + "Anb"] = _randn(g, B * NL * K, sx)
        job.update(X2=(pre + "Anb", 0), x2_N=NL, x2_NP=0)
    return job


def rowblock_y_job(g, T, pre, sx=1.0, sw=1.0, B=B5, NP=NP5, NL=NL5):
    """The n1_l0_protein form: protein rows -> the protein rows of a [B, N, 640] table (the ligand rows are gaps)."""
    N = NP + NL
    T[pre + "ph"] = _randn(g, B * NP * K, sx)
    T[pre + "P"] = _randn(g, B * N * 640)
    W, b = _weights(g, T, pre, 640, True, sw)
    return _job(X=(pre + "ph", 0), x_rows_per_b=NP, x_stride_b=NP * K, ldx=K, rows=B * NP, W=W, bias=b,
                Y=(pre + "P", 0), y_rows_per_b=NP, y_stride_b=N * 640, ldy=640, ncols=640)


def rowblock_xy_ln_job(g, T, pre, family, B=B5, NP=NP5, NL=NL5):
    """The q_ne_l0_protein form: column 512 of the protein rows of a [B, N, 640] table -> the protein rows of [B, N, 128]."""
    N = NP + NL
    T[pre + "P"] = _randn(g, B * N * 640)
    T[pre + "qn"] = _randn(g, B * N * K)
    W, b = _weights(g, T, pre, K, True)
    return _job(X=(pre + "P", 512), x_rows_per_b=NP, x_stride_b=N * 640, ldx=640, rows=B * NP, W=W, bias=b,
                ln=ln_params(g, family, T, pre),
                Y=(pre + "qn", 0), y_rows_per_b=NP, y_stride_b=N * K, ldy=K, ncols=K)


def x2_all_nodes_job(g, T, pre, sx=1.0, sw=1.0, B=B5, NP=NP5, NL=NL5):
    """The lin_node form: every node row, the addend on the ligand rows (x2_N = N, x2_NP = NP), accumulate from the other h."""
    N = NP + NL
    T[pre + "A"] = _randn(g, B * N * K, sx)
    T[pre + "Anb"] = _randn(g, B * NL * K, sx)
    T[pre + "h1"] = _randn(g, B * N * K)
    T[pre + "h0"] = _randn(g, B * N * K)
    W, b = _weights(g, T, pre, K, True, sw)
    return _job(X=(pre + "A", 0), x_rows_per_b=B * N, x_stride_b=0, ldx=K, rows=B * N, W=W, bias=b,
                Y=(pre + "h1", 0), y_rows_per_b=B * N, y_stride_b=0, ldy=K, ncols=K, accumulate=1, acc_src=pre + "h0",
                X2=(pre + "Anb", 0), x2_N=N, x2_NP=NP)


def bond_job(g, T, pre, family, B=3, NL=9, sx=1.0, sw=1.0):
    """The q_bl form: bond rows at column 512 of a 640-wide table + the destination atom's row at column 1152 of a 1280-wide
    one, through the LayerNorm prologue (family None: without it -- not a job of the forward, but the addressing bit for bit)."""
    Eb = NL * (NL - 1)
    T[pre + "PB"] = _randn(g, B * Eb * 640, sx)
    T[pre + "PL"] = _randn(g, B * NL * 1280, sx)
    T[pre + "qb"] = _randn(g, B * Eb * K)
    W, b = _weights(g, T, pre, K, True, sw)
    return _job(X=(pre + "PB", 512), x_rows_per_b=B * Eb, x_stride_b=0, ldx=640, rows=B * Eb, W=W, bias=b,
                ln=None if family is None else ln_params(g, family, T, pre),
                Y=(pre + "qb", 0), y_rows_per_b=B * Eb, y_stride_b=0, ldy=K, ncols=K,
                X2=(pre + "PL", 1152), x2_N=NL, x2_Eb=Eb, x2_NLm1=NL - 1, x2_ld=1280)


def _build():
    cases = {}

    def add(name, build, family=None):
        c = _single(name, build)
        _const_rows(c, c["jobs"][0], family)
        cases[name] = c
    for sc, (sx, sw) in SCALES.items():
        for rows in PLAIN_ROWS:
            for ncols in PLAIN_NCOLS:
                for bias in PLAIN_BIAS:
                    for acc in PLAIN_ACC:
                        add(f"plain-r{rows}-c{ncols}-b{int(bias)}-{acc}-{sc}",
                            lambda g, T, r=rows, c=ncols, b=bias, a=acc, x=sx, w=sw: plain_job(g, T, "", r, c, b, a, None, x, w))
        # the scalar epilogue (!vec_ok): ldy % 4 != 0, and Y one float off 16-byte alignment
        add(f"scalar-ldy-{sc}", lambda g, T, x=sx, w=sw: plain_job(g, T, "", 65, 70, True, "src", None, x, w, ldy_extra=1))
        add(f"scalar-yoff-{sc}", lambda g, T, x=sx, w=sw: plain_job(g, T, "", 65, 70, True, "y", None, x, w, y_off=33))
        for ncols in (128, 640, 64):
            add(f"xcd-c{ncols}-{sc}", lambda g, T, c=ncols, x=sx, w=sw: xcd_job(g, T, "", c, x, w))
        add(f"rowblock-x-{sc}", lambda g, T, x=sx, w=sw: rowblock_x_job(g, T, "", x, w))
        add(f"rowblock-y-{sc}", lambda g, T, x=sx, w=sw: rowblock_y_job(g, T, "", x, w))
        add(f"x2-all-nodes-{sc}", lambda g, T, x=sx, w=sw: x2_all_nodes_job(g, T, "", x, w))
        add(f"x2-ligand-{sc}", lambda g, T, x=sx, w=sw: rowblock_x_job(g, T, "", x, w, x2=True))
        for nl in (9, 2):
            add(f"bond-noln-nl{nl}-{sc}", lambda g, T, n=nl, x=sx, w=sw: bond_job(g, T, "", None, NL=n, sx=x, sw=w))
    for fam in LN_FAMILIES:
        add(f"ln-plain-{fam}", lambda g, T, f=fam: plain_job(g, T, "", 65, 70, True, "y", f), fam)
        add(f"ln-rowblock-xy-{fam}", lambda g, T, f=fam: rowblock_xy_ln_job(g, T, "", f), fam)
        for nl in (9, 2):
            add(f"ln-bond-nl{nl}-{fam}", lambda g, T, f=fam, n=nl: bond_job(g, T, "", f, NL=n), fam)
    return cases


_CASES = None


def cases():
    """name -> single-job case (built once, tensors shared: treat them as read-only)."""
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


def plain_groups():
    return [(rows, ncols, sc) for sc in SCALES for rows in PLAIN_ROWS for ncols in PLAIN_NCOLS]


def plain_group(rows, ncols, sc):
    return [f"plain-r{rows}-c{ncols}-b{int(b)}-{a}-{sc}" for b in PLAIN_BIAS for a in PLAIN_ACC]


def other_bit_cases():
    return [n for n, c in cases().items() if c["jobs"][0]["ln"] is None and not n.startswith("plain-")]


def bit_cases():
    return [n for n, c in cases().items() if c["jobs"][0]["ln"] is None]


def ln_cases():
    return [n for n, c in cases().items() if c["jobs"][0]["ln"] is not None]


_BATCH = None


def batch_case():
    """Six jobs of different forms in one launch, writing disjoint buffers: XCD-ordered, a single tile, LN, bond form (LN),
    row-blocked X with the ligand addend, a partial column tile accumulating from another buffer."""
    global _BATCH
    if _BATCH is None:
        g = _rng("batch6")
        T = {}
        jobs = [xcd_job(g, T, "j0.", 128),
                plain_job(g, T, "j1.", 63, 61, True, "none"),
                plain_job(g, T, "j2.", 65, 70, True, "y", "mixed"),
                bond_job(g, T, "j3.", "near1"),
                rowblock_x_job(g, T, "j4.", x2=True),
                plain_job(g, T, "j5.", 65, 70, False, "src")]
        _BATCH = {"name": "batch6", "tensors": T, "jobs": jobs}
        _const_rows(_BATCH, jobs[2], "mixed")
    return _BATCH


def batch_prefix(n):
    c = batch_case()
    return {"name": f"batch6[:{n}]", "tensors": c["tensors"], "jobs": c["jobs"][:n]}


_REF = {}


def reference(case, ji=0):
    """Cached {"bits" (non-LN jobs), "y64", "bound", "d32" (max |torch fp32 - float64|)} of job ji of a case."""
    key = (case["name"].split("[")[0], ji)
    if key not in _REF:
        job = case["jobs"][ji]
        y64, bound = expected64(case, job)
        ref = {"y64": y64, "bound": bound, "d32": float(np.abs(torch32(case, job).astype(np.float64) - y64).max())}
        if job["ln"] is None:
            ref["bits"] = expected_bits(case, job)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = ref
    return _REF[key]
