"""GPU (-m gpu): training with the narrow bond layer (h_node_in_bond_net = False) -- the cases of tests/hnode_train_cases.py, run in a
process of their own, as tests/test_gpu_out_fc_training.py runs its cases: they capture and park training graphs of further
models; a fresh process leaves the suite's own graph history exactly as it was."""
import os
import re
import subprocess
import sys

import pytest

import golden_utils as GU

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CASES = 13


@pytest.fixture(scope="module")
def case_results():
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "-rA", "-s",
                        "tests/hnode_train_cases.py"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    verdicts = {}
    for line in r.stdout.splitlines():
        m = re.match(r"^(PASSED|FAILED|ERROR|SKIPPED) tests/hnode_train_cases.py::(\S+)", line)
        if m:
            verdicts[m.group(2)] = m.group(1)
    lines = (l.lstrip(".") for l in r.stdout.splitlines())            # (-s: the progress dots share the printed lines)
    parity = list(dict.fromkeys(l for l in lines if l.startswith(("hnode ", "eager hnode", "no_grad hnode", "graphed hnode"))))
    print("\n".join(parity))
    for line in parity:
        GU.note_parity(line)
    return r, verdicts


IDENTITY = "test_hnode_loss_equals_the_zero_extended_wide_model"


def test_hnode_training_cases_pass(case_results):
    r, verdicts = case_results
    bad = {k: v for k, v in verdicts.items() if v != "PASSED"}
    assert r.returncode == 0 and not bad and len(verdicts) == N_CASES, (r.returncode, bad, len(verdicts), r.stdout[-4000:], r.stderr[-2000:])


def test_hnode_training_loss_is_bit_identical_to_the_zero_extended_wide_model(case_results):
    """The four zero-extension cases: losses bit for bit, gradients on the shared slices within the run-to-run bound."""
    r, verdicts = case_results
    mine = {k: v for k, v in verdicts.items() if k.startswith(IDENTITY)}
    assert len(mine) == 4 and all(v == "PASSED" for v in mine.values()), (mine, r.stdout[-4000:])
