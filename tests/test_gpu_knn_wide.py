"""GPU (-m gpu): kNN graphs wider than the shipped knn = 32 -- the cases of tests/knn_wide_cases.py, run in a process of their
own.  They capture and park step graphs of two more models (knn 48 / 64) with their own buffers; run inside the suite's process
they change the graph population every later test captures and destroys against, and the HIP runtime's graph lifecycle is
what the suite already has to order with care (model.py, _drop_cached_graphs).  A fresh process leaves the suite's own graph
history exactly as it was."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CASES = 26


@pytest.fixture(scope="module")
def case_results():
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "-rA", "-s",
                        "tests/knn_wide_cases.py"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    verdicts = {}
    for line in r.stdout.splitlines():
        m = re.match(r"^(PASSED|FAILED|ERROR|SKIPPED) tests/knn_wide_cases.py::(\S+)", line)
        if m:
            verdicts[m.group(2)] = m.group(1)
    print("\n".join(l for l in r.stdout.splitlines() if "knn=" in l or "padded vs groups" in l))
    return r, verdicts


def test_wide_knn_cases_pass(case_results):
    r, verdicts = case_results
    bad = {k: v for k, v in verdicts.items() if v != "PASSED"}
    assert r.returncode == 0 and not bad and len(verdicts) == N_CASES, (r.returncode, bad, len(verdicts), r.stdout[-4000:], r.stderr[-2000:])
