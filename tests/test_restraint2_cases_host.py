"""CPU checks for the general distance restraints (typed atoms, ligand-ligand pairs, the harmonic form, per-step distances): every
case of tests/restraint2_cases.py is what it says it is (margins, winners, the fp32 oracle taking the float64 oracle's branches), the
validation of the new keys of the ``restraint`` entry, their placement and collation, and the C boundary's struct."""
import ctypes
import math
import os
import re

import pytest
import torch

import restraint2_cases as C
from decompdiff_amd import RESTRAINT_ANY, RESTRAINT_NONE, harness, hip_lib
from decompdiff_amd import model as M
from test_restraint_cases_host import BATCH_L, DECOMP, N_L, entry, placed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = C.all_cases()
NUM_CLASSES = 13


# ------------------------------------------------------------------------------------------------ the cases
def test_the_sentinel_collides_with_nothing():
    import decompdiff_amd
    assert RESTRAINT_NONE == hip_lib.RESTRAINT_NONE == C.NONE and RESTRAINT_NONE not in (-1, -2, RESTRAINT_ANY) and RESTRAINT_NONE < 0
    assert "RESTRAINT_NONE" in decompdiff_amd.__all__
    hdr = open(os.path.join(ROOT, "include", "decompdiff_hip.h")).read()
    assert re.search(r"DD_RESTRAINT_NONE\s*=\s*%d\b" % RESTRAINT_NONE, hdr)


def test_the_case_table_covers_what_it_must():
    for NL in (2, 3, 63, 64, 65, 128):
        for B in (1, 3):
            assert f"random_nl{NL}_b{B}" in CASES
    assert CASES["random_nl64_b3_padded"]["nl_real"][1] == 2 and CASES["random_nl128_b3_padded"]["nl_real"][1] == 2
    for name in ("pair_tie_in_wave_nl64", "pair_tie_across_waves_nl128", "pair_hinge_values", "sets_and_classes_b3", "sets_no_decomp",
                 "one_atom_many_roles", "padded_pair_skips_padding"):
        assert name in CASES


@pytest.mark.parametrize("name", C.NAMES)
def test_case_is_what_it_says(name):
    case = CASES[name]
    ref = C.reference(name)
    B, NL, R = case["B"], case["NL"], case["R"]
    assert case["pos"].shape == (B * NL, 3) and case["pos"].dtype == torch.float32
    assert case["ptr"].tolist() == [int((case["sample"] < b).sum()) for b in range(B + 1)] and int(case["ptr"][-1]) == R
    assert bool((case["min_d"] <= case["max_d"]).all()) and bool((case["weight"] >= 0).all())
    assert bool(torch.isfinite(ref["g64"]).all()) and bool(torch.isfinite(ref["g32"]).all())
    assert C.same_branches(case), name
    assert ref["bound"] >= C.FLAT * ref["cmax"] and ref["cmax"] == max(C.coefficients(case, ref["dist"].tolist()))
    assert bool(((ref["winner2"] >= 0) <= case["pair"]).all()) and bool(((ref["winner"] >= 0) | (ref["winner2"] < 0)).all())
    if case["random"]:
        h, w = C.margins(case)
        assert h >= C.HINGE_MARGIN and w >= C.WINNER_MARGIN, (name, h, w)
        counts = torch.bincount(case["sample"], minlength=B).tolist()
        assert counts == list(C.COUNTS[B]) and max(counts) > 64
        assert bool(case["pair"].any()) and not bool(case["pair"].all()) and set(case["form"].tolist()) == {0, 1}
        assert float(ref["g64"].abs().max()) > 0.1                                   # hinges are active
        found = ref["winner"] >= 0
        assert bool(found.any()) and bool((~found).any())                            # ... and some sets are empty
        if NL > 3:
            assert bool((found & case["pair"] & (case["form"] == 1)).any()) and bool((found & case["pair"] & (case["form"] == 0)).any())
            assert bool((case["cls"] != C.ALL).any()) and bool((case["cls2"] != C.ALL).any())
        if case["nl_real"] is not None:
            assert all(n < NL for n in case["nl_real"]) and 2 in case["nl_real"]
            for w_, b in zip(ref["winner"].tolist() + ref["winner2"].tolist(), case["sample"].tolist() * 2):
                assert w_ < case["nl_real"][b]
    if "winners" in case:
        assert list(zip(ref["winner"].tolist(), ref["winner2"].tolist())) == [tuple(w) for w in case["winners"]], name
    if "expect_rows" in case:
        want = torch.zeros(B * NL, 3, dtype=torch.float64)
        for row, v in case["expect_rows"].items():
            want[row] = torch.tensor(v, dtype=torch.float64)
        assert torch.equal(ref["g64"], want), name


def test_the_constructed_cases_hold_their_edges():
    c = CASES["pair_tie_in_wave_nl64"]
    d = lambda c_, i, j: float(((c_["pos"][i].double() - c_["pos"][j].double()) ** 2).sum())
    assert d(c, 5, 9) == d(c, 7, 20) == 9.0
    c = CASES["pair_tie_across_waves_nl128"]
    assert d(c, 40, 100) == d(c, 10, 110) == 9.0
    w, w2 = C.reference("pair_tie_across_waves_nl128")["winner"], C.reference("pair_tie_across_waves_nl128")["winner2"]
    assert int(w[0]) < 64 <= int(w2[0]) and int(w2[2]) < 64 <= int(w[2]) and (int(w[1]), int(w2[1])) == (63, 64)   # ends in different waves
    c = CASES["pair_hinge_values"]
    dist = C.reference("pair_hinge_values")["dist"]
    assert all(float(dist[r]) == 0.0 and float(c["min_d"][r]) > 0 for r in c["zero_d"]) and {int(c["form"][r]) for r in c["zero_d"]} == {0, 1}
    both = [r for r in range(c["R"]) if float(c["min_d"][r]) == float(c["max_d"][r]) == float(dist[r])]
    assert {int(c["form"][r]) for r in both} == {0, 1}                                # min_d == max_d == d, for both forms
    c = CASES["sets_and_classes_b3"]
    assert int(c["v"].max()) >= 32 and int(c["v"].min()) < 0 and int((c["sample"] == c["empty_sample"]).sum()) == 0
    same = (c["atom"] >= 0) & (c["atom"] == c["atom2"])
    assert bool(same.any())                                                           # set 1 == set 2 == one atom
    no_atom_has = [r for r in range(c["R"]) if not any((int(c["cls"][r]) >> int(v)) & 1 for v in c["v"] if 0 <= int(v) < 32)]
    assert no_atom_has
    c = CASES["one_atom_many_roles"]
    w, w2 = C.reference("one_atom_many_roles")["winner"], C.reference("one_atom_many_roles")["winner2"]
    assert int((w == 0).sum()) >= 3 and int((w2 == 0).sum()) >= 3 and float(C.reference("one_atom_many_roles")["g64"][0].abs().max()) > 0.1
    c = CASES["padded_pair_skips_padding"]
    assert c["nl_real"] == [5, 2] and float((c["pos"][0] - c["pos"][6]).norm()) < float((c["pos"][0] - c["pos"][4]).norm())   # padding is nearer


def test_the_sampler_case_has_the_margins():
    for kw in (dict(), dict(scale=True, weight=(0.05, 0.15))):
        b, e, case = C.sampler_case(**kw)
        h, w = C.margins(case)
        assert h >= C.HINGE_MARGIN and w >= C.WINNER_MARGIN and C.same_branches(case)
        ref = C._reference(case)
        found = ref["winner"] >= 0
        assert bool((found & case["pair"] & (case["form"] == 1) & (case["cls2"] != C.ALL)).any())      # a typed harmonic pair acts
        assert float(ref["g64"].abs().max()) > 0.03


# ------------------------------------------------------------------------------------------------ the C boundary
def test_entry_point_is_declared_bound_and_refuses_null():
    import __graft_entry__
    __graft_entry__.build()
    lib = hip_lib.load()
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "decompdiff_hip.h")).read(), flags=re.S)
    name = "dd_drift_restraint2"
    assert name in hip_lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r"\bint\s+" + name + r"\s*\(", hdr)
    V = ctypes.c_void_p
    old = lib.dd_drift_restraint.argtypes
    assert lib.dd_drift_restraint2.argtypes == [V, V] + old[1:11] + [V, V]            # lig_v after lig_pos, winner2 after winner
    assert lib.dd_abi_version() == 9
    r = hip_lib.restraints_struct(0, None, None, None, None, None, None, None, False, 0, 999)
    assert lib.dd_drift_restraint2(None, None, None, None, 1, 4, ctypes.byref(r), None, None, 0, None, None, None, None) == -1


def test_the_struct_round_trips_the_new_fields_and_keeps_the_old_layout():
    S = hip_lib.DDRestraints
    fields = [f[0] for f in S._fields_]
    old = ["size", "R", "ptr", "point", "min_d", "max_d", "weight", "atom", "group", "scale", "t_min", "t_max"]
    new = list(hip_lib.RESTRAINT_GENERAL_FIELDS) + ["traj_positions"]
    assert fields == old + new
    assert S.t_max.offset == 72 and S.cls.offset == 80 and ctypes.sizeof(S) == 80 + 8 * 9 + 8      # today's callers pass size = 80
    ts = {k: torch.zeros(4, dtype=torch.float32 if k == "dist_traj" else torch.int32) for k in hip_lib.RESTRAINT_GENERAL_FIELDS}
    r = hip_lib.restraints_struct(4, None, None, None, None, None, None, None, True, 3, 7, traj_positions=5, **ts)
    assert r.size == ctypes.sizeof(S) and (r.R, r.scale, r.t_min, r.t_max, r.traj_positions) == (4, 1, 3, 7, 5)
    for k, t in ts.items():
        assert getattr(r, k) == t.data_ptr(), k
    r = hip_lib.restraints_struct(4, None, None, None, None, None, None, None, False, 0, 9, pair=ts["pair"], cls=None)
    assert r.pair == ts["pair"].data_ptr() and all(getattr(r, k) is None for k in hip_lib.RESTRAINT_GENERAL_FIELDS if k != "pair")
    assert r.traj_positions == 0
    with pytest.raises(TypeError):
        hip_lib.restraints_struct(4, None, None, None, None, None, None, None, False, 0, 9, colour=ts["pair"])


# ------------------------------------------------------------------------------------------------ validation
def valid(e, decomp=DECOMP, T=1000, nc=NUM_CLASSES):
    return M._as_restraints(e, BATCH_L, decomp, T, nc)


def test_an_entry_without_the_new_keys_is_a_point_entry():
    rs = valid(entry())
    assert rs["general"] is False and rs["traj"] is False and rs["cls"] is None and rs["cls2"] is None
    assert not bool(rs["pair"].any()) and rs["form"].tolist() == [0] * 4 and rs["group2"].tolist() == [RESTRAINT_NONE] * 4
    assert M._as_restraints(entry(), BATCH_L, DECOMP, 1000)["general"] is False       # (the class count has a default)
    p, _ = placed(rs, None, 3)
    assert p["general"] is False and "pair" not in p
    # every new key at its neutral spelling is still a point entry
    rs = valid(entry(classes=None, classes2=None, atom2=None, group2=None, form="linear", traj=False))
    assert rs["general"] is False
    assert valid(entry(form=["linear"] * 4))["general"] is False
    assert valid(entry(group2=[None] * 4, atom2=torch.full((4,), -1)))["general"] is False


def test_every_spelling_of_the_new_keys_is_accepted():
    # samples [2, 0, 2, 1]: flat rows 7 .. 11, 0 .. 3, 7 .. 11, 4 .. 6
    rs = valid(entry(atom2=torch.tensor([8, -1, -1, -1]), group2=torch.tensor([RESTRAINT_NONE, 1, RESTRAINT_NONE, RESTRAINT_ANY])))
    assert rs["pair"].tolist() == [True, True, False, True] and rs["general"]
    assert rs["atom2"].tolist() == [1, -1, -1, -1] and rs["atom2"].dtype == torch.int32          # flat row 8 -> row 1 of sample 2
    assert rs["group2"].tolist() == [RESTRAINT_ANY, 1, RESTRAINT_NONE, RESTRAINT_ANY]            # (not read for an explicit atom)
    rs = valid(entry(group2=[None, -1, None, 0]))
    assert rs["pair"].tolist() == [False, True, False, True] and rs["group2"].tolist() == [RESTRAINT_NONE, -1, RESTRAINT_NONE, 0]
    ids = [None, [0, 12], (3,), torch.tensor([1, 2])]
    rs = valid(entry(classes=ids))
    assert rs["cls"].tolist() == [0xFFFFFFFF, 1 | 1 << 12, 8, 6] and rs["cls2"] is None and rs["general"]
    m = torch.zeros(4, NUM_CLASSES, dtype=torch.bool)
    m[0, :] = True
    m[1, [0, 12]] = True
    m[2, 3] = True
    m[3, [1, 2]] = True
    rs2 = valid(entry(classes2=m, group2=-torch.ones(4, dtype=torch.long)))
    assert rs2["cls2"].tolist() == [(1 << NUM_CLASSES) - 1, 1 | 1 << 12, 8, 6] and rs2["cls"] is None
    assert valid(entry(classes=[[22]] * 4), nc=23)["cls"].tolist() == [1 << 22] * 4              # the widest vocabulary
    rs = valid(entry(form="harmonic"))
    assert rs["form"].tolist() == [1] * 4 and rs["form"].dtype == torch.int32 and rs["general"]
    assert valid(entry(form=["linear", "harmonic", "linear", "harmonic"]))["form"].tolist() == [0, 1, 0, 1]
    rs = valid(entry(traj=True))
    assert rs["traj"] is True and rs["general"] and not bool(rs["pair"].any())
    # point may be None (or left out) when every restraint is a pair; a pair's point is ignored but must be finite
    for e in (entry(point=None, group2=[0, 0, 0, 0]), entry(point=..., atom2=torch.tensor([8, 0, 8, 5]))):
        rs = valid(e)
        assert bool(rs["pair"].all()) and torch.equal(rs["point"], torch.zeros(4, 3))
    with pytest.raises(ValueError):
        valid(entry(point=torch.full((4, 3), math.nan), group2=[0, 0, 0, 0]))
    # ANY needs no decomposition at the second endpoint either
    rs = valid(entry(atom=None, group=None, group2=[RESTRAINT_ANY] * 4), decomp=None)
    assert bool(rs["pair"].all())


@pytest.mark.parametrize("bad", [
    dict(classes=[[0], [1], [2]]), dict(classes=[[0], [1], [2], [NUM_CLASSES]]), dict(classes=[[0], [1], [2], [-1]]),
    dict(classes=[[0], [1], [2], []]), dict(classes=[[0], [1], [2], [1.0]]), dict(classes=[[0], [1], [2], [True]]), dict(classes=5),
    dict(classes=torch.ones(4, NUM_CLASSES)), dict(classes=torch.ones(4, NUM_CLASSES + 1, dtype=torch.bool)),
    dict(classes=torch.zeros(4, NUM_CLASSES, dtype=torch.bool)), dict(classes2=[[0], [1], [2], [99]]), dict(classes2=[[0], [1], [2], 7]),
    dict(atom2=torch.tensor([0, -1, -1, -1])),                 # a row of another sample (restraint 0 belongs to sample 2)
    dict(atom2=torch.tensor([-1, 2, -1, -1])),                 # atom2 == atom
    dict(atom2=torch.tensor([-2, -1, -1, -1])), dict(atom2=torch.tensor([12, -1, -1, -1])), dict(atom2=torch.tensor([8.0, -1, -1, -1])),
    dict(atom2=torch.tensor([8, -1, -1])), dict(group2=torch.tensor([-2, 0, 0, 0])), dict(group2=torch.tensor([0, 0, 0])),
    dict(group2=torch.tensor([0.0, 0, 0, 0])), dict(group2=7.5),
    dict(point=None), dict(point=None, group2=[0, None, 0, 0]),    # a pair without a second endpoint
    dict(form="cubic"), dict(form=["linear"] * 3), dict(form=1), dict(form=["linear", "harmonic", "linear", 2]),
    dict(traj=1), dict(traj="yes"), dict(classes3=[[0]] * 4)])
def test_bad_new_keys_raise_value_error(bad):
    with pytest.raises(ValueError):
        valid(entry(**bad))


def test_a_second_arm_or_scaffold_group_needs_the_decomposition():
    e = entry(atom=None, group=None)
    assert valid(dict(e, group2=[RESTRAINT_ANY, None, None, None]), decomp=None)["R"] == 4
    for g2 in ([-1, None, None, None], [None, None, 0, None]):
        with pytest.raises(ValueError):
            valid(dict(e, group2=g2), decomp=None)


# ------------------------------------------------------------------------------------------------ placement
def test_placement_keeps_every_new_array_with_its_restraint_through_the_sort():
    rs = valid(entry(atom2=torch.tensor([8, -1, 11, -1]), group2=[None, 1, None, None], classes=[[0], [1], [2], [3]],
                     classes2=[None, [4], [5, 6], None], form=["linear", "harmonic", "harmonic", "linear"], traj=True))
    p, _ = placed(rs, None, 3)
    assert p["order"].tolist() == [1, 3, 0, 2] and p["general"] and p["traj"]
    assert p["atom2"].tolist() == [-1, -1, 1, 4] and p["atom"].tolist() == [2, -1, -1, 2]        # rows within the sample, with their restraint
    assert p["pair"].tolist() == [True, False, True, True] and p["group2"].tolist() == [1, RESTRAINT_NONE, RESTRAINT_ANY, RESTRAINT_ANY]
    assert p["cls"].tolist() == [2, 8, 1, 4] and p["cls2"].tolist() == [16, 0xFFFFFFFF, 0xFFFFFFFF, 96] and p["form"].tolist() == [1, 0, 0, 1]
    # the way back: first + atom2 is the caller's flat row
    assert [int(p["first"][r]) + int(p["atom2"][r]) for r in (2, 3)] == [8, 11]
    q, _ = placed(rs, [2, 0], 2)                               # a size group holding the call's samples 2 and 0
    assert q["order"].tolist() == [0, 2, 1] and q["atom2"].tolist() == [1, 4, -1] and q["form"].tolist() == [0, 1, 1]
    assert q["cls"].tolist() == [1, 4, 2] and q["pair"].tolist() == [True, True, True]
    u, _ = placed(valid(entry(form="harmonic")), None, 3)      # untyped: every class at both ends
    assert u["cls"].tolist() == [0xFFFFFFFF] * 4 and u["cls2"].tolist() == [0xFFFFFFFF] * 4 and not bool(u["pair"].any())


def test_harness_collation_passes_the_new_keys_through():
    def fn(g, dec):
        if g == 11:
            return None
        n = int(dec.numel())
        if g == 10:
            return dict(point=torch.full((2, 3), 1.0), min_d=1.0, max_d=2.0, atom=torch.tensor([n - 1, -1]), atom2=torch.tensor([0, -1]),
                        group2=[None, -1], classes=[[1, 2], None], form=["harmonic", "linear"])
        return dict(min_d=0.5, max_d=math.inf, atom2=torch.tensor([1, 2]), atom=torch.tensor([0, 0]), classes2=torch.eye(2, NUM_CLASSES, dtype=torch.bool),
                    form="harmonic")
    e = harness.collate_restraints(fn, 10, N_L, DECOMP, scale=True, traj=True)
    assert e["sample"].tolist() == [0, 0, 2, 2] and e["atom"].tolist() == [3, -1, 7, 7] and e["atom2"].tolist() == [0, -1, 8, 9]
    assert e["group2"].tolist() == [RESTRAINT_NONE, -1, RESTRAINT_NONE, RESTRAINT_NONE] and e["traj"] is True
    assert e["classes"] == [[1, 2], None, None, None] and e["classes2"] == [None, None, [0], [1]] and e["form"] == ["harmonic", "linear", "harmonic", "harmonic"]
    rs = valid(e)
    assert rs["pair"].tolist() == [True, True, True, True] and rs["atom2"].tolist() == [0, -1, 1, 2] and rs["cls2"].tolist()[2:] == [1, 2]
    # a call none of whose samples uses a new key stays a point entry
    old = harness.collate_restraints(lambda g, dec: dict(point=torch.zeros(1, 3), min_d=0.0, max_d=1.0), 0, N_L, DECOMP)
    assert not set(old) & {"atom2", "group2", "classes", "classes2", "form", "traj"} and valid(old)["general"] is False
    with pytest.raises(ValueError):
        harness.collate_restraints(lambda g, dec: dict(min_d=0.0, max_d=1.0), 0, N_L, DECOMP)                     # neither point nor a second end
    with pytest.raises(ValueError):
        harness.collate_restraints(lambda g, dec: dict(point=torch.zeros(2, 3), min_d=0.0, max_d=1.0, atom2=torch.tensor([1])), 0, N_L, DECOMP)
