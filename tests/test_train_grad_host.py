"""CPU: the oracle side of the training-gradient cases (tests/train_grad_cases.py).  For every (regime, shape): the float64 and
the fp32 oracle run see the same kNN edges (asserted inside train_grad_cases.reference), every one of the 572 learnable tensors
receives a gradient, the number of tensors whose float64 gradient is exactly zero is the pinned one, every d32_t is within
D32_MAX -- so that stress_weights.bound() judges the case at all -- and the fp32 oracle itself has no tensor above its bound:
the GPU cases may exempt up to five tensors, the reference's own fp32 arithmetic needs none."""
import pytest
import torch

import stress_weights as SW
import train_grad_cases as TG

def test_case_list():
    assert len(TG.cases()) == 11 and len(TG.cases(TG.DENSE)) == 10
    assert "sharp6" not in TG.REGIMES and set(TG.REGIMES) <= set(SW.REGIMES) | {"synthetic"}


@pytest.mark.parametrize("regime,shape", sorted(TG.cases()))
def test_oracle_gradients_are_a_usable_yardstick(regime, shape):
    ref = TG.reference(regime, shape)
    d32 = ref["d32"]
    vals = sorted(d32.values())
    worst = max(d32, key=d32.get)
    zero = TG.zero_tensors(ref)
    print(f"\nTRAINGRAD-HOST {regime} {shape} worst d32={d32[worst]:.3g} ({worst}) median d32={vals[len(vals) // 2]:.3g} "
          f"zero-gradient tensors={len(zero)} d32 of the outputs: " + " ".join(f"{k}:{v:.2g}" for k, v in ref["d32_out"].items()))
    assert len(ref["grad64"]) == TG.N_LEARNABLE and set(ref["grad64"]) == {k for k, v in ref["sd"].items() if v.is_floating_point()}
    assert not ref["unused"], ref["unused"]
    assert all(v.dtype == torch.float64 and bool(torch.isfinite(v).all()) for v in ref["grad64"].values())
    assert len(zero) == TG.expected_zero_tensors(regime, shape), zero
    assert d32[worst] <= SW.D32_MAX, (worst, d32[worst])
    out_bound, bnd = TG.bounds(ref)                          # (bound() asserts d32 <= D32_MAX for every tensor and output)
    assert not [n for n in d32 if not d32[n] <= bnd[n]]
    assert all(v == SW.TOL for v in out_bound.values())      # the outputs: fp32 is within 2.5e-5 of float64 in every case
