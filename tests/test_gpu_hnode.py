"""GPU (-m gpu): the narrow bond layer (h_node_in_bond_net = False) end to end -- the cases of tests/hnode_cases.py, run in a process
of their own, as tests/test_gpu_out_fc.py runs its cases: they capture and park step graphs of further models; a fresh process
leaves the suite's own graph history exactly as it was."""
import os
import re
import subprocess
import sys

import pytest

import golden_utils as GU

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CASES = 34


@pytest.fixture(scope="module")
def case_results():
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "-rA", "-s",
                        "tests/hnode_cases.py"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    verdicts = {}
    for line in r.stdout.splitlines():
        m = re.match(r"^(PASSED|FAILED|ERROR|SKIPPED) tests/hnode_cases.py::(\S+)", line)
        if m:
            verdicts[m.group(2)] = m.group(1)
    lines = (l.lstrip(".") for l in r.stdout.splitlines())            # (-s: the progress dots share the printed lines)
    parity = list(dict.fromkeys(l for l in lines if l.startswith("hnode ")))
    print("\n".join(parity))
    for line in parity:
        GU.note_parity(line)
    return r, verdicts


def test_hnode_cases_pass(case_results):
    r, verdicts = case_results
    bad = {k: v for k, v in verdicts.items() if v != "PASSED"}
    assert r.returncode == 0 and not bad and len(verdicts) == N_CASES, (r.returncode, bad, len(verdicts), r.stdout[-4000:], r.stderr[-2000:])
