"""CPU: the restatements and the case builder of tests/gemm_cases.py, which tests/test_gpu_gemm_forms.py holds the projection
GEMM to -- the fp32 FMA emulation against exact integer arithmetic, the bit-exact restatement against the float64 one within the
derived bound, and every window and row map of the cases against a brute-force enumeration."""
import math

import numpy as np
import pytest

import gemm_cases as GC


# ------------------------------------------------------------------------------------------------ fma32 vs exact integers
def _decompose(x):
    """float32 value -> (integer mantissa, exponent): x = m * 2^e exactly."""
    m, e = math.frexp(float(x))
    mi = int(math.ldexp(m, 24))
    assert math.ldexp(mi, e - 24) == float(x)
    return mi, e - 24


def _round_f32(num, e):
    """num * 2^e (Python ints) rounded to the nearest fp32, ties to even, written out; normal range only."""
    if num == 0:
        return 0.0
    sign, n = (-1.0 if num < 0 else 1.0), abs(num)
    drop = n.bit_length() - 24
    if drop <= 0:
        mant, exp = n << -drop, e + drop
    else:
        mant, rem, half = n >> drop, n & ((1 << drop) - 1), 1 << (drop - 1)
        if rem > half or (rem == half and (mant & 1)):
            mant += 1
        exp = e + drop
    if mant == 1 << 24:
        mant, exp = mant >> 1, exp + 1
    assert -149 <= exp and exp + 23 >= -126 and exp + 23 <= 127, "outside the normal range"
    return sign * math.ldexp(mant, exp)


def fma_exact(a, b, c):
    (ma, ea), (mb, eb), (mc, ec) = _decompose(a), _decompose(b), _decompose(c)
    e = min(ea + eb, ec)
    return _round_f32(((ma * mb) << (ea + eb - e)) + (mc << (ec - e)), e)


def _check(a, b, c):
    got = GC.fma32(a, b, c)
    want = np.array([fma_exact(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    bad = np.nonzero(got.view(np.int32) != want.view(np.int32))[0]
    assert bad.size == 0, [(a[i], b[i], c[i], got[i], want[i]) for i in bad[:5]]
    return want


def test_fma32_random_triples():
    g = np.random.default_rng(7)
    n = 6000
    a = (g.standard_normal(n) * 10.0 ** g.integers(-3, 4, n)).astype(np.float32)
    b = (g.standard_normal(n) * 10.0 ** g.integers(-3, 4, n)).astype(np.float32)
    c = (g.standard_normal(n) * 10.0 ** g.integers(-3, 4, n)).astype(np.float32)
    # a third of them with a * b + c cancelling to a few ulps, a third with c = 0 (the first link of a chain)
    c[: n // 3] = -(a[: n // 3].astype(np.float64) * b[: n // 3]).astype(np.float32)
    c[n // 3: 2 * n // 3] = 0.0
    keep = np.array([x == 0.0 or abs(x) > 1e-30 for x in (a.astype(np.float64) * b + c)])   # (stay clear of subnormal results)
    _check(a[keep], b[keep], c[keep])


def midpoint_triples():
    """a * b + c exactly on an fp32 midpoint, and one float64-invisible unit above / below it.
    p = a * b is 2^46, 2^46 + 1 = 8384513 * 8392705 or 2^46 - 1 = (2^23 + 1)(2^23 - 1); c = 2^70 + j 2^47 has the fp32 spacing
    2^47, so c + 2^46 is a midpoint and the +-1 lies 2^-52 of the sum below float64's resolution; powers of two and signs varied."""
    assert 8384513 * 8392705 == 2 ** 46 + 1 and 8384513 < 2 ** 24 and 8392705 < 2 ** 24
    out = []
    for j in (0, 1, 2, 5, 2 ** 23 - 2, 2 ** 23 - 1):
        for a, b in ((2.0 ** 23, 2.0 ** 23), (8384513.0, 8392705.0), (2.0 ** 23 + 1, 2.0 ** 23 - 1)):
            for sa, sc, sign in ((0, 0, 1.0), (-40, -35, 1.0), (11, -90, -1.0)):
                out.append((sign * math.ldexp(a, sa), math.ldexp(b, sc), sign * math.ldexp(2.0 ** 70 + j * 2.0 ** 47, sa + sc)))
    return tuple(np.array(v, np.float32) for v in zip(*out))


def test_fma32_midpoints_and_near_misses():
    a, b, c = midpoint_triples()
    assert (a.astype(np.float64) == np.array([float(x) for x in a])).all()
    want = _check(a, b, c)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    wrong = int((naive.view(np.int32) != want.view(np.int32)).sum())
    print(f"\nconstructed triples: {a.size}, double rounding through float64 wrong on {wrong}")
    assert wrong >= 1
    # each of the three kinds decides differently somewhere: up, down and to even
    up = want.astype(np.float64) > c.astype(np.float64)
    assert up.any() and (~up).any()


def test_k_order_is_a_permutation():
    assert sorted(GC.K_ORDER) == list(range(128)) and GC.K_ORDER[:8] == (0, 2, 1, 3, 4, 6, 5, 7)


# ------------------------------------------------------------------------------------------------ bits vs float64
def _bit_groups():
    return [pytest.param(GC.plain_group(*gk), id="plain-r%d-c%d-%s" % gk) for gk in GC.plain_groups()] + \
           [pytest.param([n], id=n) for n in GC.other_bit_cases()]


@pytest.mark.parametrize("names", _bit_groups())
def test_expected_bits_within_derived_bound(names):
    for name in names:
        case = GC.cases()[name]
        ref = GC.reference(case)
        err = np.abs(ref["bits"].astype(np.float64) - ref["y64"])
        frac = float((err / ref["bound"]).max())
        scale = float(np.sqrt((ref["y64"] ** 2).mean()))
        med = float(np.median(ref["bound"]))
        print(f"\n{name}: {err.size} elements, worst err/bound {frac:.3f}, median bound {med:.3g} = {med / scale:.3g} of the output rms")
        assert (err <= ref["bound"]).all()
        assert frac > 0.0 or err.size <= 4                  # (fp32 does round: a restatement in float64 by accident would show)
        assert med < 1e-4 * scale


def test_summation_order_is_visible():
    """The restatement is sharp enough for its purpose: the ascending chain differs from the tile's order in some bit."""
    case = GC.cases()["xcd-c128-s1"]
    job = dict(case["jobs"][0], rows=64)
    a, b = GC.expected_bits(case, job), GC.expected_bits(case, job, tuple(range(128)))
    assert (a.view(np.int32) != b.view(np.int32)).any()


# ------------------------------------------------------------------------------------------------ the case builder
def _all_cases():
    return list(GC.cases().values()) + [GC.batch_case()]


def test_every_address_inside_its_tensor():
    n_jobs = 0
    for case in _all_cases():
        T = case["tensors"]
        for job in case["jobs"]:
            n_jobs += 1
            xs, ys, s2 = GC.x_starts(job), GC.y_starts(job), GC.x2_starts(job)
            assert len(xs) == len(ys) == job["rows"] > 0
            assert xs.min() >= 0 and xs.max() + 128 <= T[job["X"][0]].size and (xs % 4 == 0).all()
            assert ys.min() >= 0 and ys.max() + job["ncols"] <= T[job["Y"][0]].size
            assert len(np.unique(ys)) == len(ys) and np.diff(np.sort(ys)).min(initial=job["ncols"]) >= job["ncols"]
            assert T[job["W"]].size == job["ncols"] * 128
            assert job["bias"] is None or T[job["bias"]].size == job["ncols"]
            assert job["ln"] is None or T[job["ln"]].size == 256
            if job["acc_src"]:
                assert job["accumulate"] and T[job["acc_src"]].size == T[job["Y"][0]].size and job["acc_src"] != job["Y"][0]
            if s2 is not None:
                assert len(s2) == job["rows"] and (s2 >= 0).any()
                assert s2.max() + 128 <= T[job["X2"][0]].size and (s2[s2 >= 0] % 4 == 0).all()
            for t in T.values():
                assert t.dtype == np.float32 and t.ndim == 1 and np.isfinite(t).all()
    assert n_jobs > 250


def test_batch_jobs_write_disjoint_buffers():
    case = GC.batch_case()
    assert len(case["jobs"]) == 6
    written = {}
    for job in case["jobs"]:
        m = GC.written_mask(case, job)
        prev = written.setdefault(job["Y"][0], np.zeros_like(m))
        assert not (prev & m).any()
        prev |= m
    for job in case["jobs"]:                                 # ... and nothing a job reads is written by any job of the batch but itself
        reads = {job["X"][0], job["W"], job["bias"], job["ln"], job["acc_src"], job["X2"][0] if job["X2"] else None} - {None}
        assert not (reads & set(written))
    forms = case["jobs"]
    assert forms[0]["rows"] >= 16 * 64 and forms[0]["ncols"] > 64                      # XCD-ordered
    assert forms[1]["rows"] <= 64 and forms[1]["ncols"] <= 64                          # a single tile
    assert forms[2]["ln"] and forms[3]["ln"] and forms[3]["x2_Eb"] > 0                 # LN, bond form


def _view_starts(shape, index):
    """Flat offsets picked by plain array indexing of a [B, rows, ld] table."""
    return np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)[index].ravel()


def test_row_maps_agree_with_brute_force():
    C = GC.cases()
    B, NP, NL, N = GC.B5, GC.NP5, GC.NL5, GC.N5
    job = C["rowblock-x-s1"]["jobs"][0]                                           # X rows: h[:, NP:]
    assert np.array_equal(GC.x_starts(job), _view_starts((B, N, 128), np.s_[:, NP:, 0]))
    assert np.array_equal(GC.y_starts(job), _view_starts((B * NL, 1280), np.s_[:, 0]))
    job = C["rowblock-y-s1"]["jobs"][0]                                           # Y rows: P[:, :NP] of [B, N, 640]
    assert np.array_equal(GC.y_starts(job), _view_starts((B, N, 640), np.s_[:, :NP, 0]))
    assert np.array_equal(GC.x_starts(job), _view_starts((B * NP, 128), np.s_[:, 0]))
    job = C["ln-rowblock-xy-near1"]["jobs"][0]                                    # both: column 512 of P[:, :NP] -> qn[:, :NP]
    assert np.array_equal(GC.x_starts(job), _view_starts((B, N, 640), np.s_[:, :NP, 512]))
    assert np.array_equal(GC.y_starts(job), _view_starts((B, N, 128), np.s_[:, :NP, 0]))
    job = C["x2-all-nodes-s1"]["jobs"][0]                                         # addend of node (b, n >= NP): Anb[b, n - NP]
    want = np.full((B, N), -1, np.int64)
    want[:, NP:] = _view_starts((B, NL, 128), np.s_[:, :, 0]).reshape(B, NL)
    assert np.array_equal(GC.x2_starts(job), want.ravel()) and (want >= 0).sum() == B * NL
    job = C["x2-ligand-s1"]["jobs"][0]                                            # ligand rows only: row r <-> Anb row r
    assert np.array_equal(GC.x2_starts(job), 128 * np.arange(B * NL))
    for nl in (9, 2):                                                             # bond (b, dst, j) <- PL[b, dst, 1152:]
        job = C[f"bond-noln-nl{nl}-s1"]["jobs"][0]
        atoms = _view_starts((3, nl, 1280), np.s_[:, :, 1152]).reshape(3, nl)
        assert np.array_equal(GC.x2_starts(job), np.repeat(atoms, nl - 1, axis=1).ravel())
        assert job["rows"] == 3 * nl * (nl - 1)
        assert np.array_equal(GC.x_starts(job), _view_starts((job["rows"], 640), np.s_[:, 512]))
    # the same maps in closed form, for every job of every case
    for case in _all_cases():
        for job in case["jobs"]:
            r = np.arange(job["rows"])
            assert np.array_equal(GC.x_starts(job), job["X"][1] + r // job["x_rows_per_b"] * job["x_stride_b"] + r % job["x_rows_per_b"] * job["ldx"])
            assert np.array_equal(GC.y_starts(job), job["Y"][1] + r // job["y_rows_per_b"] * job["y_stride_b"] + r % job["y_rows_per_b"] * job["ldy"])


def test_case_list_covers_the_paths():
    C = GC.cases()
    assert len(GC.bit_cases()) == 2 * (120 + 2 + 3 + 4 + 2) and len(GC.ln_cases()) == 8
    for sc in GC.SCALES:
        a, b = C[f"scalar-ldy-{sc}"]["jobs"][0], C[f"scalar-yoff-{sc}"]["jobs"][0]
        assert a["ldy"] % 4 != 0 and a["Y"][1] % 4 == 0 and b["ldy"] % 4 == 0 and b["Y"][1] % 4 == 1
        for ncols, xcd in ((128, True), (640, True), (64, False)):
            j = C[f"xcd-c{ncols}-{sc}"]["jobs"][0]
            nbx, nby = -(-j["rows"] // 64), -(-ncols // 64)
            assert nbx == 17 and (nbx >= 16 and nby >= 2) == xcd
    for fam in GC.LN_FAMILIES:                                                    # mixed: variance 0 on the first quarter of the rows
        for name in (f"ln-plain-{fam}", f"ln-rowblock-xy-{fam}", f"ln-bond-nl9-{fam}", f"ln-bond-nl2-{fam}"):
            case = C[name]
            job = case["jobs"][0]
            X, X2, _, _, ln, _ = GC.inputs(case, job)
            x = X if X2 is None else X + X2
            n = max(1, job["rows"] // 4)
            assert ((x[:n].max(1) == x[:n].min(1)).all()) == (fam == "mixed")
            assert (int((ln[0] < 0).sum()), int((ln[0] == 0).sum())) == ((40, 5) if fam == "mixed" else (int((ln[0] < 0).sum()), 0))
