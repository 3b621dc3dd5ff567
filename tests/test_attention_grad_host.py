"""CPU: the yardstick of the attention-gradient tests (tests/attention_grad_cases.py).  The closed forms that
dd_attn_aggregate_node_bwd / dd_attn_aggregate_pos_bwd implement equal torch autograd of the reference expression in float64;
the reference's own fp32 run stays within D32_MAX of float64 at scales 1 and 2 (so the GPU bound leaves room for the kernels and
is no gift); the new entry points are declared in the header and exported by the binding."""
import os
import re

import pytest
import torch

import attention_grad_cases as AG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("node",) + c for c in AG.NODE_CASES] + [("pos",) + c for c in AG.POS_CASES]


def test_layout_covers_the_edges_of_the_member_loop():
    index, ptr, n = AG.layout()
    assert n == 15 and n % 4 != 0                                             # the last workgroup is partly filled
    assert AG.SIZES[0] == 0 and AG.SIZES[-1] != 0 and 0 in AG.SIZES[1:-1]
    assert {s % 4 for s in AG.SIZES if s} == {0, 1, 2, 3} and max(AG.SIZES) > 256
    assert {31, 32, 33, 64, 65} <= set(AG.SIZES)
    assert ptr.tolist() == [0] + torch.tensor(AG.SIZES).cumsum(0).tolist() and index.numel() == sum(AG.SIZES)
    assert bool((index[1:] >= index[:-1]).all()) and torch.bincount(index, minlength=n).tolist() == AG.SIZES


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_closed_forms_equal_float64_autograd(case):
    form, rest = case[0], case[1:]
    ref = AG.reference(form, *rest)
    out, grads = AG.closed_form(form, ref["t"])
    errs = {"out": float((out - ref["out64"]).abs().max())}
    assert set(grads) == set(ref["grad64"]) == set(ref["t"]["names"])
    for name, g in grads.items():
        assert g.shape == ref["grad64"][name].shape == ref["t"][name].shape, name
        errs[name] = float((g - ref["grad64"][name]).abs().max())
    print(f"\nATTNGRAD closed form {case}: " + " ".join(f"{k}:{v:.2g}" for k, v in errs.items()) + f" d32:{ref['d32']:.2g}")
    assert max(errs.values()) <= 1e-12, errs
    if rest[0] != "sharp":
        assert ref["d32"] <= AG.D32_MAX, ref["d32"]
    assert AG.bound(rest[0], ref["d32"]) >= AG.TOL
    # empty segments: a zero output row and (q per segment) a zero dq row
    empty = [s for s, m in enumerate(AG.SIZES) if m == 0]
    assert not bool(ref["out64"][empty].any())
    if not ref["t"]["per_edge"]:
        assert not bool(ref["grad64"]["q"][empty].any())


def test_per_edge_cases_have_equal_rows_in_a_segment():
    t = AG.inputs("node", "unit", True, per_edge=True)
    assert t["q"].shape == (sum(AG.SIZES), 128)
    first = t["ptr"][:-1].long()[t["index"]]
    assert torch.equal(t["q"], t["q"][first])


def test_backward_entry_points_are_declared_and_exported():
    from decompdiff_amd import hip_lib
    header = open(os.path.join(ROOT, "include", "decompdiff_hip.h")).read()
    for name in ("dd_attn_aggregate_node_bwd", "dd_attn_aggregate_pos_bwd"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in hip_lib.EXPORTED_SYMBOLS
    assert hip_lib.ABI_VERSION == 9                                           # additive entry points: the ABI version stays
    lib = hip_lib.load()
    assert lib.dd_abi_version() == 9 and all(hasattr(lib, n) for n in ("dd_attn_aggregate_node_bwd", "dd_attn_aggregate_pos_bwd"))
