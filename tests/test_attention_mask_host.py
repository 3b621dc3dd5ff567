"""CPU: the yardstick of the member-mask tests (tests/attention_mask_cases.py).  The mask has the members it is documented to have;
the closed forms the masked kernels implement (the unmasked formulas with alpha = 0 on masked members) equal torch autograd of the
masked reference expression in float64; masked members get exact zeros; the reference's own fp32 run stays within D32_MAX of
float64 at scales 1 and 2; the four masked entry points are declared, exported and bound, and the public ops take the keyword."""
import inspect
import os
import re

import pytest
import torch

import attention_mask_cases as AM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("node",) + c for c in AM.NODE_CASES] + [("pos",) + c for c in AM.POS_CASES]
MASKED_SYMBOLS = ("dd_attn_aggregate_node_masked", "dd_attn_aggregate_pos_masked", "dd_attn_aggregate_node_bwd_masked",
                  "dd_attn_aggregate_pos_bwd_masked")


def test_mask_has_the_documented_members():
    m = AM.mask()
    index, ptr, n = AM.AG.layout()
    assert m.dtype == torch.bool and m.numel() == sum(AM.SIZES) == 664
    assert int(m.sum()) == AM.N_REAL == 391
    real = torch.zeros(n, dtype=torch.long).index_add(0, index, m.long()).tolist()
    by_size = {}
    for s, size in enumerate(AM.SIZES):
        by_size.setdefault(size, []).append((s, real[s]))
    assert by_size[300][0][1] == 200 and bool(m[int(ptr[by_size[300][0][0]]):][:200].all())           # the padded prefix
    assert by_size[64][0][1] == 0 and by_size[32][0][1] == 32
    s33 = by_size[33][0][0]
    assert by_size[33][0][1] == 1 and bool(m[int(ptr[s33 + 1]) - 1])                                  # only the last member
    s5 = by_size[5][0][0]
    assert by_size[5][0][1] == 4 and not bool(m[int(ptr[s5])])                                        # only the first is masked
    assert [r for _, r in by_size[1]] == [0, 1]
    mixed = sum(1 for size, r in zip(AM.SIZES, real) if 0 < r < size)
    none_real = sum(1 for size, r in zip(AM.SIZES, real) if size > 0 and r == 0)
    assert (mixed, none_real) == (AM.N_MIXED, AM.N_ALL_MASKED) == (7, 2)
    assert torch.equal(m, AM.mask())                                                                  # the same mask every time


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_masked_closed_forms_equal_float64_autograd(case):
    form, rest = case[0], case[1:]
    ref = AM.reference(form, *rest)
    t = ref["t"]
    out, grads = AM.closed_form(form, t)
    errs = {"out": float((out - ref["out64"]).abs().max())}
    assert set(grads) == set(ref["grad64"]) == set(t["names"])
    for name, g in grads.items():
        assert g.shape == ref["grad64"][name].shape == t[name].shape, name
        errs[name] = float((g - ref["grad64"][name]).abs().max())
    print(f"\nATTNMASK closed form {case}: " + " ".join(f"{k}:{v:.2g}" for k, v in errs.items()) + f" d32:{ref['d32']:.2g}")
    assert max(errs.values()) <= 1e-12, errs
    if rest[0] != "sharp":
        assert ref["d32"] <= AM.D32_MAX, ref["d32"]
    assert AM.bound(rest[0], ref["d32"]) >= AM.TOL
    # masked members: exact zeros in every per-member gradient, from autograd and from the closed form
    masked = ~t["mask"]
    for name in ("k", "v", "rel_x", "e_w") + (("q",) if t["per_edge"] else ()):
        if name in grads:
            assert not bool(ref["grad64"][name][masked].any()), name
            assert not bool(grads[name][masked].any()), name
    # segments without a real member (empty or all masked): a zero output row and (q per segment) a zero dq row
    real = torch.zeros(t["n"], dtype=torch.long).index_add(0, t["index"], t["mask"].long())
    none = (real == 0).nonzero().view(-1)
    assert none.numel() == AM.SIZES.count(0) + AM.N_ALL_MASKED
    assert not bool(ref["out64"][none].any())
    if not t["per_edge"]:
        assert not bool(ref["grad64"]["q"][none].any())


def test_masked_reference_is_the_unmasked_reference_of_the_compacted_case():
    """The yardstick itself: a masked member does not exist -- float64 results on the full arrays equal those on the real members."""
    for form, case in (("node", ("double", True, True)), ("pos", ("double", True))):
        ref = AM.reference(form, *case)
        t = ref["t"]
        c = AM.compacted(t)
        out, grads = AM.AG.autograd_run(form, c, torch.float64)
        assert float((out - ref["out64"]).abs().max()) <= 1e-12
        for name in t["names"]:
            full = ref["grad64"][name]
            sel = full[t["mask"]] if full.size(0) == t["mask"].numel() else full
            assert float((grads[name] - sel).abs().max()) <= 1e-12, name


def test_masked_entry_points_are_declared_exported_and_bound():
    from decompdiff_amd import hip_lib
    header = open(os.path.join(ROOT, "include", "decompdiff_hip.h")).read()
    for name in MASKED_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in hip_lib.EXPORTED_SYMBOLS, name
    assert hip_lib.ABI_VERSION == 9                                           # additive entry points: the ABI version stays
    lib = hip_lib.load()
    assert lib.dd_abi_version() == 9
    for name in MASKED_SYMBOLS:
        assert hasattr(lib, name), name
        sibling = getattr(lib, name.replace("_masked", ""))
        assert len(getattr(lib, name).argtypes) == len(sibling.argtypes) + 1, name      # the sibling's list plus member_mask


def test_public_ops_take_the_member_mask_keyword():
    from decompdiff_amd import functional as FN
    for fn in (FN.scatter_attention, FN.scatter_attention_pos, FN.scatter_attention_backward, FN.scatter_attention_pos_backward):
        params = inspect.signature(fn).parameters
        assert list(params)[-1] == "member_mask" and params["member_mask"].default is None, fn.__name__
