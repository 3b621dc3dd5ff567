"""GPU (-m gpu): the forward under the weight regimes of tests/stress_weights.py against the float64 oracle, and
dd_reverse_step at its edges against the float64 restatement of tests/stress_steps.py -- the cases of tests/stress_cases.py,
run in a process of their own: they build 26 further models (one per weight regime, eight, and one per step case, 18) with
their own packed weights and buffers (see tests/test_gpu_knn_wide.py for why such cases do not share the suite's process).
The wrapper asserts every verdict and the case count, and hands one line per regime and one per (class count, logit scale)
of the step cases -- the measured error next to its bound and fp32's own distance d32 to float64 -- to the terminal summary."""
import os
import re
import subprocess
import sys

import pytest

import golden_utils as GU

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 21 forwards: 7 regimes x (bench shape, tiny graph) + 2 x (NL = 34, NL = 66) + 1 padded batch + 2 lattice geometries;
# 18 step cases: (8, 13, 23 atom classes) x (uniform, skewed, zero-probability-class priors) x (NL = 30, 66), 12 transitions each
N_CASES = 21 + 18


@pytest.fixture(scope="module")
def case_results():
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "-rA", "-s",
                        "tests/stress_cases.py"], cwd=ROOT, capture_output=True, text=True, timeout=1500)
    verdicts, worst, steps = {}, {}, {}
    for line in r.stdout.splitlines():
        m = re.match(r"^(PASSED|FAILED|ERROR|SKIPPED) tests/stress_cases.py::(\S+)", line)
        if m:
            verdicts[m.group(2)] = m.group(1)
        m = re.match(r"^STRESS (\S+) (\S+) worst=(\S+) err=(\S+) bound=(\S+) d32=(\S+)", line)
        if m:
            regime, shape, name, err, bound, d32 = m.group(1), m.group(2), m.group(3), float(m.group(4)), float(m.group(5)), float(m.group(6))
            rec = worst.setdefault(regime, dict(n=0, ratio=-1.0))
            rec["n"] += 1
            if err / bound > rec["ratio"]:
                rec.update(ratio=err / bound, text=f"{name} at {shape}: {err:.2g} (bound {bound:.2g}, fp32 oracle vs fp64 {d32:.2g})")
        m = re.match(r"^STEP nc=(\d+) \S+ \S+ \S+ scale=(\S+) \S+ worst=(\S+) err=(\S+) bound=(\S+) d32=(\S+) type-mismatches=(\d+)\+(\d+)", line)
        if m:
            key = f"dd_reverse_step, {m.group(1)} atom classes, logits x {m.group(2)}"
            err, bound = float(m.group(4)), float(m.group(5))
            rec = steps.setdefault(key, dict(n=0, ratio=-1.0, mism=0))
            rec["n"] += 1
            rec["mism"] += int(m.group(7)) + int(m.group(8))
            if err / bound > rec["ratio"]:
                rec.update(ratio=err / bound, text=f"{m.group(3)} {err:.2g} (bound {bound:.2g}, fp32 torch vs fp64 {float(m.group(6)):.2g})")
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith(("STRESS", "STEP"))))
    for key, rec in sorted(steps.items()):
        GU.note_parity(f"{key} vs fp64 ({rec['n']} transitions): {rec['mism']} type mismatches, closest to its bound {rec['text']}")
    for regime, rec in sorted(worst.items()):
        GU.note_parity(f"forward vs fp64 oracle, weights '{regime}' ({rec['n']} shapes): closest to its bound {rec['text']}")
    return r, verdicts


def test_stress_cases_pass(case_results):
    r, verdicts = case_results
    bad = {k: v for k, v in verdicts.items() if v != "PASSED"}
    assert r.returncode == 0 and not bad and len(verdicts) == N_CASES, (r.returncode, bad, len(verdicts), r.stdout[-6000:], r.stderr[-2000:])
