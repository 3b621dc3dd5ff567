"""GPU (-m gpu): the device's production noise held to tests/philox_ref.py, the host restatement of the documented contract
(Philox4x32-10, key = the seed's halves, counter = (row, row >> 32, time word, stream | class block << 8), uniforms from the top
24 bits, Box-Muller normals with the clamp of u1 and the fp32 angle).

(a) The exposed draws (dd_debug_philox, the device functions every production kernel draws through) equal the reference:
    uniforms bit for bit; normals within 4 x d32a of the reference's z64a, d32a = max |z32 - z64a| of the reference itself over
    these very draws (philox_ref.contract_d32a; 4.7e-7 -> bound 1.9e-6).  The factor 4 leaves the device's logf / sqrtf / cosf a
    few ulp each against numpy's.  The measured worst distance is printed next to the bound.
(b) The plain, unfixed reverse step (k_step_rows<NC, false>, k_step_pos) under production noise draws at the documented addresses
    on streams 1 / 2 / 7: tests/philox_step_cases.py, run in a process of its own (it builds four further models; see
    tests/test_gpu_knn_wide.py and tests/test_gpu_stress.py for the shape); the wrapper asserts every verdict and the case count.
(c) Every other production path already recomputes its result from the exposed draws; with (a) those draws are the contract's:

    path                          carried back to (a) by
    FIXED steps, replace          test_gpu_fixed_atoms.py::test_replace_with_device_noise_draws_level_l_at_time_l_plus_one
    resampling jumps              test_gpu_resample.py::test_the_jump_alone_against_float64
    chain init                    test_gpu_chain_init.py::test_prior_state_is_the_exposed_draws, ::test_noised_state_*
    keyed and padded addressing   test_gpu_sample_keys.py::test_anchor_one_sample_keyed_is_that_sample_seeded and the
                                  "equals each sample alone" tests (a keyed sample is the sample alone with seed = key)
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_utils as GU
import philox_ref as PR
from decompdiff_amd import hip_lib
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STEP_CASES = 4                                         # philox_step_cases.CASES, six transitions each


def draw(seed, word, rows, kind, nc=0):
    """dd_debug_philox -> numpy float32 [rows, classes] (kinds 1-6) or [rows] (kinds 7-9); `nc` rides in bits 8-15 of kind."""
    cols = 1 if kind in PR.NORMAL_KINDS else (PR.NUM_BOND_CLASSES if kind in PR.BOND_KINDS else (nc or 8))
    out = torch.full((rows * cols,), float("nan"), device=dev())
    hip_lib.check(hip_lib.load().dd_debug_philox(seed, PR.as_c_int(word), rows, kind | (nc << 8), hip_lib.ptr(out), hip_lib.stream_ptr()),
                  "dd_debug_philox")
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    return a.reshape(rows, cols) if cols > 1 else a


@pytest.mark.parametrize("kind", PR.ATOM_KINDS + PR.BOND_KINDS)
def test_exposed_uniforms_equal_the_reference_bit_for_bit(kind):
    """300 atom rows x {8 (as 0), 8, 13, 23} classes / 1000 bond rows x 5 classes: the class counts that are no power of two cross
    the 256-thread blocks of the launch; five seeds (both key halves, all ones) x six time words (the last two with bit 30 / bit 31
    set: the word is `step` cast to uint32)."""
    atoms = kind in PR.ATOM_KINDS
    rows = PR.ATOM_ROWS if atoms else PR.BOND_ROWS
    bad, n = [], 0
    for nc in (PR.CONTRACT_CLASS_COUNTS if atoms else (0,)):
        for seed in PR.CONTRACT_SEEDS:
            for word in PR.CONTRACT_WORDS:
                got = draw(seed, word, rows, kind, nc)
                want = PR.uniforms(seed, rows, word, kind, (nc or 8) if atoms else PR.NUM_BOND_CLASSES)
                n += want.size
                if got.dtype != np.float32 or got.shape != want.shape or not np.array_equal(got, want):
                    bad.append((nc, hex(seed), hex(word), int((got != want).sum()) if got.shape == want.shape else got.shape))
    print(f"\nPHILOX kind={kind} uniforms: {n} draws, {len(bad)} of the (class count, seed, word) sets differ")
    GU.note_parity(f"dd_debug_philox kind {kind} vs the host Philox reference: {n} uniforms, " + ("bit-equal" if not bad else f"{len(bad)} sets DIFFER"))
    assert not bad, bad[:8]


@pytest.mark.parametrize("kind", PR.NORMAL_KINDS)
def test_exposed_normals_within_the_fp32_distance_of_the_reference(kind):
    bound = 4.0 * PR.contract_d32a()
    worst, where, n = 0.0, None, 0
    for seed in PR.CONTRACT_SEEDS:
        for word in PR.CONTRACT_WORDS:
            got = draw(seed, word, PR.N_NORMALS, kind)
            assert got.dtype == np.float32 and got.shape == (PR.N_NORMALS,) and np.isfinite(got).all(), (hex(seed), hex(word))
            d = np.abs(got.astype(np.float64) - PR.normals(seed, PR.N_NORMALS, word, kind)["z64a"])
            n += d.size
            if float(d.max()) > worst:
                worst, where = float(d.max()), (hex(seed), hex(word), int(d.argmax()))
    print(f"\nPHILOX kind={kind} normals: {n} draws, max |device - z64a| = {worst:.3g} at {where}, bound 4 x d32a = {bound:.3g} "
          f"(d32a {PR.contract_d32a():.3g})")
    GU.note_parity(f"dd_debug_philox kind {kind} vs the host Philox reference: {n} normals, max |device - z64a| {worst:.2g} "
                   f"(bound 4 x d32a = {bound:.2g})")
    assert worst <= bound, (worst, bound, where)


def test_edge_draws():
    """The clamp of u1 (a draw whose u1 bits are all zero: log(0) without it) on each normal stream, and the two ends of the uniform
    range, at the draws tests/test_philox_ref_host.py re-derives."""
    bound = 4.0 * PR.contract_d32a()
    for seed, stream, idx in PR.EDGE_NORMALS:
        got = float(draw(seed, PR.EDGE_WORD, idx + 1, stream)[idx])
        want = float(PR.normals(seed, np.array([idx]), PR.EDGE_WORD, stream)["z64a"][0])
        print(f"\nPHILOX edge normal seed={seed} stream={stream} idx={idx}: device {got!r}, z64a {want!r}, |d| = {abs(got - want):.3g}, bound {bound:.3g}")
        assert np.isfinite(got) and abs(got - want) <= bound, (seed, stream, idx, got, want)
    for seed, stream, row, c, value in PR.EDGE_UNIFORMS:
        got = draw(seed, PR.EDGE_WORD, row + 1, stream)[row, c]
        assert got.dtype == np.float32 and float(got) == value, (seed, row, c, float(got))
        assert np.array_equal(draw(seed, PR.EDGE_WORD, row + 1, stream), PR.uniforms(seed, row + 1, PR.EDGE_WORD, stream, 8))


# ------------------------------------------------------------------------------------------------ (b), in a process of its own
@pytest.fixture(scope="module")
def step_case_results():
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "-rA", "-s",
                        "tests/philox_step_cases.py"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    verdicts, cases = {}, {}
    for line in r.stdout.splitlines():
        m = re.match(r"^(PASSED|FAILED|ERROR|SKIPPED) tests/philox_step_cases.py::(\S+)", line)
        if m:
            verdicts[m.group(2)] = m.group(1)
        m = re.match(r"^PHILOXSTEP nc=(\d+) NL=(\d+) \S+ \S+ worst=(\S+) err=(\S+) bound=(\S+) d32=(\S+) type-mismatches=(\d+)\+(\d+)", line)
        if m:
            err, bound = float(m.group(4)), float(m.group(5))
            rec = cases.setdefault(f"{m.group(1)} atom classes, NL = {m.group(2)}", dict(n=0, ratio=-1.0, mism=0))
            rec["n"] += 1
            rec["mism"] += int(m.group(7)) + int(m.group(8))
            if err / bound > rec["ratio"]:
                rec.update(ratio=err / bound, text=f"{m.group(3)} {err:.2g} (bound {bound:.2g}, fp32 torch vs fp64 {float(m.group(6)):.2g})")
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith("PHILOXSTEP")))
    for key, rec in sorted(cases.items()):
        GU.note_parity(f"unfixed step under device noise vs fp64 on the host reference's draws, {key} ({rec['n']} transitions): "
                       f"{rec['mism']} type mismatches, closest to its bound {rec['text']}")
    return r, verdicts, cases


def test_unfixed_step_cases_pass(step_case_results):
    r, verdicts, cases = step_case_results
    bad = {k: v for k, v in verdicts.items() if v != "PASSED"}
    assert r.returncode == 0 and not bad and len(verdicts) == N_STEP_CASES, (r.returncode, bad, len(verdicts), r.stdout[-6000:], r.stderr[-2000:])
    assert len(cases) == N_STEP_CASES and all(rec["n"] == 6 and rec["mism"] == 0 for rec in cases.values()), cases
