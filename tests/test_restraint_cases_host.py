"""CPU checks for the distance-restraint term: every case of tests/restraint_cases.py is what it says it is (margins, winners, the
fp32 oracle taking the float64 oracle's branches), the validation of the ``restraint`` entry of ``energy_drift_opt``, and the
collation / placement of restraints in the dense, padded and grouped chain layouts (explicit-atom remap, ``ptr`` rebuild)."""
import ctypes
import math
import os
import re

import pytest
import torch

import restraint_cases as RC
from decompdiff_amd import RESTRAINT_ANY, batch_layout as BL, harness, hip_lib
from decompdiff_amd import model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = RC.all_cases()


# ------------------------------------------------------------------------------------------------ the cases
def test_the_constant_collides_with_no_decomp_value():
    import decompdiff_amd
    assert RESTRAINT_ANY == hip_lib.RESTRAINT_ANY == -3 and RESTRAINT_ANY not in (-1, -2) and RESTRAINT_ANY < 0
    assert "RESTRAINT_ANY" in decompdiff_amd.__all__
    hdr = open(os.path.join(ROOT, "include", "decompdiff_hip.h")).read()
    assert re.search(r"DD_RESTRAINT_ANY\s*=\s*-3\b", hdr)


@pytest.mark.parametrize("name", RC.NAMES)
def test_case_is_what_it_says(name):
    case = CASES[name]
    ref = RC.reference(name)
    B, NL, R = case["B"], case["NL"], case["R"]
    assert case["pos"].shape == (B * NL, 3) and case["pos"].dtype == torch.float32
    assert case["ptr"].tolist() == [int((case["sample"] < b).sum()) for b in range(B + 1)] and int(case["ptr"][-1]) == R
    assert bool((case["min_d"] <= case["max_d"]).all()) and bool((case["weight"] >= 0).all())
    assert bool(torch.isfinite(ref["g64"]).all()) and bool(torch.isfinite(ref["g32"]).all())
    assert RC.same_branches(case), name
    assert ref["bound"] >= RC.FLAT * float(case["weight"].max())
    if case["random"]:
        h, w = RC.margins(case)
        assert h >= RC.HINGE_MARGIN and w >= RC.WINNER_MARGIN, (name, h, w)
        kinds = {(int(a) >= 0, int(g)) for a, g in zip(case["atom"], case["group"])}
        assert any(k[0] for k in kinds) and {RC.ANY, RC.SCA, RC.ABSENT_ARM} <= {k[1] for k in kinds}
        counts = torch.bincount(case["sample"], minlength=B).tolist()
        assert counts == list(RC.COUNTS[B]) and max(counts) > 64
        assert float(ref["g64"].abs().max()) > 0.1                                   # hinges are active
        if case["nl_real"] is not None:
            assert all(n < NL for n in case["nl_real"])
            assert all(w < case["nl_real"][int(b)] for w, b in zip(ref["winner"].tolist(), case["sample"]))
    if "winners" in case:
        assert ref["winner"].tolist() == case["winners"], name
    if "expect" in case:
        assert torch.equal(ref["g64"], torch.tensor(case["expect"], dtype=torch.float64)), name
    if "expect_rows" in case:
        want = torch.zeros(B * NL, 3, dtype=torch.float64)
        for row, v in case["expect_rows"].items():
            want[row] = torch.tensor(v, dtype=torch.float64)
        assert torch.equal(ref["g64"], want), name


def test_the_constructed_cases_hold_their_edges():
    c = CASES["hinge_values"]
    d = RC.reference("hinge_values")["dist"]
    for r, which in c["eq"].items():                                                 # exact equality with a bound
        assert (which in ("min", "both")) == (float(d[r]) == float(c["min_d"][r]))
        assert (which in ("max", "both")) == (float(d[r]) == float(c["max_d"][r]))
    assert all(float(d[r]) == 0.0 and float(c["min_d"][r]) > 0 for r in c["zero_d"])
    assert math.isinf(float(c["max_d"].max())) and float(c["weight"].min()) == 0.0
    for name, rows in (("tie_in_wave_nl64", (10, 20)), ("tie_across_waves_nl128", (40, 100))):
        c = CASES[name]
        p = c["point"][0].double()
        da, db = (((c["pos"][r].double() - p) ** 2).sum() for r in rows)
        assert float(da) == float(db) == 9.0 and RC.reference(name)["winner"][0] == rows[0]
    assert rows[0] < 64 <= rows[1]                                                   # the tie is across the two waves
    c = CASES["padded_nearest_is_padding"]
    assert torch.equal(c["pos"][6], c["point"][0]) and c["nl_real"][0] <= 6          # the nearest row of all is padding
    c = CASES["groups_b3"]
    arms = set(c["decomp"][c["decomp"] >= 0].tolist())
    assert arms == {0, 2, 5} and RC.ABSENT_ARM not in arms and int((c["sample"] == c["empty_sample"]).sum()) == 0
    assert {RC.ANY, RC.SCA, 1, 2, 5, RC.ABSENT_ARM} <= set(c["group"].tolist()) and int(c["atom"].max()) >= 0


# ------------------------------------------------------------------------------------------------ the C boundary
def test_entry_points_are_declared_bound_and_refuse_null():
    import __graft_entry__
    __graft_entry__.build()
    lib = hip_lib.load()
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "decompdiff_hip.h")).read(), flags=re.S)
    for name in ("dd_drift_restraint", "dd_sample_steps_guided", "dd_graph_create_guided"):
        assert name in hip_lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    S, O, V, F, Rs, Q = (ctypes.POINTER(hip_lib.DDSampler), ctypes.POINTER(hip_lib.DDModelOpts), ctypes.c_void_p,
                         ctypes.POINTER(hip_lib.DDFixed), ctypes.POINTER(hip_lib.DDResample), ctypes.POINTER(hip_lib.DDRestraints))
    assert lib.dd_sample_steps_guided.argtypes == [S, O, V, F, Rs, Q, ctypes.c_int, V]
    assert lib.dd_graph_create_guided.argtypes == [S, O, V, F, Rs, Q, ctypes.c_int, V, ctypes.POINTER(V)]
    # the pair is the _resample pair with one more NULL-able struct
    assert lib.dd_sample_steps_guided.argtypes[:5] + lib.dd_sample_steps_guided.argtypes[6:] == lib.dd_sample_steps_resample.argtypes
    fields = [f[0] for f in hip_lib.DDRestraints._fields_]
    body = re.search(r"typedef struct dd_restraints \{(.*?)\} dd_restraints;", hdr, re.S).group(1)
    assert fields == re.findall(r"(\w+)\s*[;,]", body.replace("*", " ")), body
    assert lib.dd_abi_version() == 9
    assert lib.dd_sample_steps_guided(None, None, None, None, None, None, 1, None) == -1
    assert lib.dd_graph_create_guided(None, None, None, None, None, None, 1, None, None) == -1
    r = hip_lib.restraints_struct(0, None, None, None, None, None, None, None, False, 0, 999)
    assert r.size == ctypes.sizeof(hip_lib.DDRestraints) and r.scale == 0 and (r.t_min, r.t_max) == (0, 999)
    assert lib.dd_drift_restraint(None, None, None, 1, 4, ctypes.byref(r), None, None, 0, None, None, None) == -1


# ------------------------------------------------------------------------------------------------ validation
N_L = [4, 3, 5]                                                # ligand sizes of the three samples
BATCH_L = torch.tensor([0] * 4 + [1] * 3 + [2] * 5)
DECOMP = torch.tensor([0, -1, 1, -1, -1, 0, 0, 2, 2, -1, 0, -1])


def entry(**kw):
    e = dict(type="restraint", sample=torch.tensor([2, 0, 2, 1]), point=torch.arange(12.0).reshape(4, 3), min_d=1.0, max_d=2.5,
             atom=torch.tensor([-1, 2, 9, -1]), group=torch.tensor([RESTRAINT_ANY, 0, 0, -1]))
    e.update(kw)
    return {k: v for k, v in e.items() if v is not ...}


def valid(e, decomp=DECOMP, T=1000):
    return M._as_restraints(e, BATCH_L, decomp, T)


def test_a_valid_entry_is_normalised():
    rs = valid(entry(weight=torch.tensor([1.0, 2.0, 0.0, 0.5]), max_d=torch.tensor([2.5, math.inf, 3.0, 2.5]), scale=True, t_min=10, t_max=400))
    assert rs["R"] == 4 and rs["sample"].tolist() == [2, 0, 2, 1] and rs["first"].tolist() == [0, 4, 7]
    assert rs["atom"].tolist() == [-1, 2, 2, -1] and rs["atom"].dtype == torch.int32        # flat rows 2 and 9 -> rows within the sample
    assert rs["group"].tolist() == [RESTRAINT_ANY, RESTRAINT_ANY, RESTRAINT_ANY, -1]        # (not read for an explicit atom)
    assert rs["min_d"].tolist() == [1.0] * 4 and math.isinf(float(rs["max_d"][1])) and rs["weight"].tolist() == [1.0, 2.0, 0.0, 0.5]
    assert (rs["scale"], rs["t_min"], rs["t_max"]) == (True, 10, 400)
    d = valid(entry(atom=None, group=None))
    assert d["atom"].tolist() == [-1] * 4 and d["group"].tolist() == [RESTRAINT_ANY] * 4 and (d["t_min"], d["t_max"], d["scale"]) == (0, 999, False)
    assert d["weight"].tolist() == [1.0] * 4
    e0 = valid(dict(type="restraint", sample=torch.zeros(0, dtype=torch.long), point=torch.zeros(0, 3), min_d=0.0, max_d=1.0))
    assert e0["R"] == 0
    assert valid(entry(atom=None, group=None), decomp=None)["R"] == 4                        # ANY needs no decomposition


@pytest.mark.parametrize("bad", [
    dict(sample=torch.tensor([2, 0, 2, 3])), dict(sample=torch.tensor([2, 0, 2, -1])), dict(sample=torch.tensor([2.0, 0, 2, 1])),
    dict(sample=torch.tensor([[2, 0, 2, 1]])), dict(point=torch.zeros(4, 2)), dict(point=torch.zeros(3, 3)),
    dict(point=torch.zeros(4, 3, dtype=torch.long)), dict(point=torch.full((4, 3), math.nan)), dict(point=torch.full((4, 3), math.inf)),
    dict(min_d=...), dict(max_d=...), dict(min_d=3.0), dict(min_d=-0.5), dict(min_d=math.inf), dict(max_d=math.nan),
    dict(min_d=torch.tensor([1.0, 1.0])), dict(max_d=torch.tensor([2.5, 2.5, 0.5, 2.5])), dict(weight=-1.0), dict(weight=math.inf),
    dict(weight=torch.ones(3)), dict(atom=torch.tensor([-1, 5, 9, -1])), dict(atom=torch.tensor([-1, 2, 12, -1])),
    dict(atom=torch.tensor([-2, 2, 9, -1])), dict(atom=torch.tensor([-1.0, 2, 9, -1])), dict(atom=torch.tensor([-1, 2, 9])),
    dict(group=torch.tensor([-2, 0, 0, -1])), dict(group=torch.tensor([RESTRAINT_ANY, 0, 0])), dict(group=torch.tensor([0.0, 0, 0, -1])),
    dict(t_min=-1), dict(t_max=1000), dict(t_min=5, t_max=4), dict(t_min=1.0), dict(scale="yes"), dict(colour="red"), dict(sample=...)])
def test_bad_entries_raise_value_error(bad):
    with pytest.raises(ValueError):
        valid(entry(**bad))


def test_more_refusals():
    with pytest.raises(ValueError):                            # a scaffold / arm group without ligand_decomp_index
        valid(entry(), decomp=None)
    with pytest.raises(ValueError):                            # the term listed twice
        M._split_restraints([entry(), dict(type="clash", sigma=2, gamma=4), entry()])
    rest, mine = M._split_restraints([dict(type="clash", sigma=2, gamma=4), entry()])
    assert [d["type"] for d in rest] == ["clash"] and mine["type"] == "restraint"
    assert M._split_restraints(None) == (None, None) and M._split_restraints([]) == ([], None)
    M._drift_fields(rest, True)                                # the three old terms go where they went
    with pytest.raises(ValueError):
        M._drift_fields([entry()], True)                       # ... and `_drift_fields` itself still knows only those


# ------------------------------------------------------------------------------------------------ placement
def placed(rs, ids, B):
    off = torch.arange(3.0 * B).reshape(B, 3) * 0.25
    return M._place_restraints(rs, ids, B, off), off


def test_dense_and_padded_placement_sort_by_sample_and_keep_the_callers_order_within_one():
    rs = valid(entry(min_d=torch.tensor([1.0, 1.1, 1.2, 1.3]), max_d=9.0))
    p, off = placed(rs, None, 3)
    assert p["order"].tolist() == [1, 3, 0, 2] and p["ptr"].tolist() == [0, 1, 2, 4] and p["ptr"].dtype == torch.int32
    assert p["min_d"].tolist() == pytest.approx([1.1, 1.3, 1.0, 1.2]) and p["atom"].tolist() == [2, -1, -1, 2]
    want = torch.arange(12.0).reshape(4, 3)[p["order"]] - off[torch.tensor([0, 1, 2, 2])]
    assert torch.equal(p["point"], want) and p["point"].dtype == torch.float32       # the fp32 p - offset[b]
    assert p["first"].tolist() == [0, 4, 7, 7]                                       # the way back to the caller's flat rows
    # padded chain: the explicit atom's padded row is slot * NLmax + row within the sample = where padded_rows() puts its flat row
    rows_l = BL.BatchLayout([10, 10, 10], N_L).padded_rows()[1]
    for r in range(4):
        if int(p["atom"][r]) >= 0:
            flat = int(p["first"][r]) + int(p["atom"][r])
            assert int(rows_l[flat]) == int(p["slot"][r]) * max(N_L) + int(p["atom"][r])
    assert sorted(int(p["first"][r]) + int(p["atom"][r]) for r in range(4) if int(p["atom"][r]) >= 0) == [2, 9]


def test_group_placement_takes_the_restraints_of_its_samples_and_rebuilds_ptr():
    rs = valid(entry())
    p, off = placed(rs, [2, 0], 2)                             # a size group holding the call's samples 2 and 0, in that order
    assert p["order"].tolist() == [0, 2, 1] and p["slot"].tolist() == [0, 0, 1] and p["ptr"].tolist() == [0, 2, 3]
    assert p["atom"].tolist() == [-1, 2, 2] and torch.equal(p["point"][2], torch.tensor([3.0, 4.0, 5.0]) - off[1])
    q, _ = placed(rs, [1], 1)                                  # sample 1 alone
    assert q["order"].tolist() == [3] and q["ptr"].tolist() == [0, 1] and q["group"].tolist() == [-1]
    e, _ = placed(valid(entry(sample=torch.tensor([0, 0, 0, 0]), atom=None, group=None)), [1, 2], 2)
    assert e["R"] == 0 and e["ptr"].tolist() == [0, 0, 0]      # a chain whose samples carry nothing


def test_harness_collation():
    def fn(g, dec):
        if g == 11:
            return None
        n = int(dec.numel())
        return dict(point=torch.full((2, 3), float(g)), min_d=1.0, max_d=torch.tensor([2.0, math.inf]), atom=torch.tensor([n - 1, -1]),
                    group=torch.tensor([RESTRAINT_ANY, -1]))
    e = harness.collate_restraints(fn, 10, N_L, DECOMP, scale=True, t_max=300)
    assert e["type"] == "restraint" and e["sample"].tolist() == [0, 0, 2, 2] and e["atom"].tolist() == [3, -1, 11, -1]
    assert e["point"][:, 0].tolist() == [10.0, 10.0, 12.0, 12.0] and e["weight"].tolist() == [1.0] * 4 and e["scale"] and e["t_max"] == 300
    rs = valid(e)
    assert rs["atom"].tolist() == [3, -1, 4, -1] and rs["t_max"] == 300
    none = harness.collate_restraints(lambda g, dec: None, 0, N_L, DECOMP)
    assert valid(none)["R"] == 0
    with pytest.raises(ValueError):
        harness.collate_restraints(lambda g, dec: dict(point=torch.zeros(1, 3), min_d=0.0, max_d=1.0, atom=torch.tensor([7])), 0, N_L, DECOMP)
