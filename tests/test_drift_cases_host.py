"""CPU checks of tests/drift_cases.py: every random case has the margins its seed was chosen for, every constructed case is what
it says it is (in float64 and in fp32), the fp32 oracle stays close enough to the float64 one for the bounds to mean something,
and the oracle itself has the conventions the drift kernels are held to (zero subgradient at distance 0, inclusive hinges,
empty arm ids pass no gradient)."""
import math

import pytest
import torch

import drift_cases as DC
from oracle import diffusion as OD
from oracle import ops as OO

CASES = DC.all_cases()
RANDOM = [n for n in DC.NAMES if CASES[n]["random"]]
F64, F32 = torch.float64, torch.float32


def test_the_case_list_covers_the_sizes_at_which_the_kernels_change_path():
    for NL in (2, 3, 63, 64, 65, 127, 128):
        for B in (1, 3):
            assert f"armsca/random_nl{NL}_b{B}" in CASES
    for NF in (1, 63, 255, 256, 257, 600):
        for NL in (1, 3, 30):
            c = CASES[f"clash/random_nf{NF}_nl{NL}_s2"]
            assert (c["B"], c["NF"], c["NL"], c["sigma"], c["gamma"]) == (2, NF, NL, 2.0, 4.0)
    assert sum(1 for n in DC.NAMES if n.startswith("clash/") and CASES[n]["sigma"] != 2.0) >= 1
    for NL in (2, 64, 65, 128):
        for mode in ("min", "all"):
            assert CASES[f"repul_{mode}/random_nl{NL}"]["mode"] == mode
    for c in CASES.values():                                    # the same fp32 inputs feed both precisions and the kernels
        assert c["pos"].dtype == F32 and c["pos"].shape == (c["B"] * c["NL"], 3)
        assert c["NL"] <= 128


@pytest.mark.parametrize("name", RANDOM)
def test_random_cases_have_their_margins_and_fp32_agrees_on_every_branch(name):
    c = CASES[name]
    h, w = DC.MARGINS[c["kind"]](c, F64)
    assert h >= DC.HINGE_MARGIN, (name, h)
    assert w >= DC.WINNER_MARGIN, (name, w)
    assert DC.same_branches(c), name


def test_random_armsca_cases_reach_both_hinges_on_both_reduction_paths():
    for sizes in ((2, 3, 63, 64), (65, 127, 128)):
        lo = hi = 0
        for NL in sizes:
            for B in (1, 3):
                c = CASES[f"armsca/random_nl{NL}_b{B}"]
                ds = [v[2] for v in DC.armsca_winners(c, F64).values()]
                lo += sum(d < c["min_d"] for d in ds)
                hi += sum(d > c["max_d"] for d in ds)
        assert lo >= 3 and hi >= 3, (sizes, lo, hi)


def test_random_clash_and_repul_cases_have_active_and_inactive_terms():
    act = tot = 0
    for n in RANDOM:
        c = CASES[n]
        if c["kind"] == "clash":
            G, _ = DC.clash_G(c, F64)
            act, tot = act + int((G < c["gamma"]).sum()), tot + G.numel()
            if c["NL"] == 30:
                assert 0 < int((G < c["gamma"]).sum()) < G.numel(), n
        if c["kind"] == "repul" and c["NL"] > 2:
            a, m = DC.repul_pairs(c, F64)
            assert 0 < int((a <= c["max_d"]).sum()) < a.numel(), n
            assert any(v[2] <= c["max_d"] for v in m.values()), n
    assert 0 < act < tot


@pytest.mark.parametrize("name", DC.NAMES)
def test_fp32_oracle_is_close_enough_for_the_bound_to_mean_something(name):
    c = CASES[name]
    g64, g32, d32, bnd = DC.reference(name)
    flat = DC.FLAT[c["kind"]]
    assert bool(torch.isfinite(g64).all()) and bool(torch.isfinite(g32).all()), name
    assert d32 <= DC.D32_MAX_FACTOR * flat
    assert bnd == (flat if d32 <= 0.25 * flat else max(flat, 2 * d32))
    # these are well-conditioned by construction: the fp32 oracle is inside the flat tolerance everywhere, so no case runs on a widened bound
    assert bnd == flat, (name, d32)
    if "expect" in c:
        assert float((g64 - torch.tensor(c["expect"], dtype=F64)).abs().max()) < 1e-15, (name, g64)
        assert float((g32.double() - torch.tensor(c["expect"], dtype=F64)).abs().max()) < 1e-7, (name, g32)
    elif not c["random"] or c["NL"] > 1:
        assert float(g64.abs().max()) > 0, name


# ------------------------------------------------------------------------------------------------ constructed: armsca
@pytest.mark.parametrize("dtype", [F64, F32])
def test_two_wave_case_has_a_winner_in_each_wave_and_an_exact_tie_across_them(dtype):
    c = CASES["armsca/two_wave_winners_nl128"]
    assert c["NL"] == 128 and c["B"] == 1
    w = DC.armsca_winners(c, dtype)
    assert w[(0, 0)][1] < 64 and w[(0, 0)][2] == 1.0 and w[(0, 0)][2] < c["min_d"]
    assert w[(0, 1)][1] >= 64 and w[(0, 1)][2] == 3.0 and w[(0, 1)][2] > c["max_d"]
    a, s_lo, s_hi = c["tie"]
    assert s_lo < 64 <= s_hi and c["decomp"][s_lo] == -1 and c["decomp"][s_hi] == -1 and c["decomp"][a] == 2
    pos = c["pos"].to(dtype)
    d_lo, d_hi = torch.norm(pos[a] - pos[s_lo]), torch.norm(pos[a] - pos[s_hi])
    assert float(d_lo) == float(d_hi) == 3.0                      # exact in both precisions: integer squared distances
    assert w[(0, 2)][2] == 3.0 and w[(0, 2)][3] == 3.0            # winner and runner-up tie
    for k, pair in c["winners"].items():
        assert w[(0, k)][:2] == pair
    # which pair the ORACLE's autograd picks: the gradient sits on the arm atom and on one of the two tied scaffold atoms
    g = DC.armsca_grad(c, dtype)
    assert float(g[s_lo].abs().max()) > 0 and float(g[s_hi].abs().max()) == 0, "the oracle takes the first scaffold atom of a tie"
    assert torch.equal(g[a], -g[s_lo])
    for l in range(128):                                          # nothing anywhere else
        if l not in (5, 55, 25, 100, a, s_lo):
            assert float(g[l].abs().max()) == 0


@pytest.mark.parametrize("dtype", [F64, F32])
def test_hinge_cases_sit_at_exact_equality(dtype):
    for name in ("armsca/hinge_eq_both", "armsca/hinge_eq_cancel"):
        c = CASES[name]
        w = DC.armsca_winners(c, dtype)
        for arm, d in c["eq"].items():
            assert w[(0, arm)][2] == d and (d == c["min_d"] or d == c["max_d"]), (name, arm)
    c = CASES["armsca/hinge_eq_both"]
    assert torch.tensor(c["min_d"], dtype=dtype) - 1.0 == 0 and torch.tensor(c["max_d"], dtype=dtype) - 2.0 == 0
    c = CASES["armsca/hinge_eq_cancel"]
    assert c["min_d"] == c["max_d"] == 2.0
    c = CASES["armsca/hinge_eq_max_quoted"]
    assert DC.armsca_winners(c, dtype)[(0, 0)][2] == c["max_d"] == 2.0


@pytest.mark.parametrize("dtype", [F64, F32])
def test_coincident_and_invalid_cases_are_what_they_say(dtype):
    for name in ("armsca/coincident_quoted", "armsca/coincident_active_arm"):
        c = CASES[name]
        w = DC.armsca_winners(c, dtype)
        for arm in c["zero_d"]:
            a, s, d, _ = w[(0, arm)]
            assert d == 0.0 and torch.equal(c["pos"][a], c["pos"][s]) and c["decomp"][s] == -1
    c = CASES["armsca/invalid_and_gap_b3"]
    dec = c["decomp"].view(3, 4)
    assert bool((dec[0] == -1).all()) and bool((dec[1] >= 0).all()) and sorted(set(dec[2].tolist())) == [-1, 0, 2]
    g = DC.armsca_grad(c, dtype)
    assert float(g[:8].abs().max()) == 0 and float(g[8:].abs().max()) > 0


# ------------------------------------------------------------------------------------------------- constructed: clash
def test_clash_constructed_sample_holds_every_edge():
    c = CASES["clash/constructed_nf63"]
    NL, NF = c["NL"], c["NF"]
    G64, S64 = DC.clash_G(c, F64)
    G32, S32 = DC.clash_G(c, F32)
    for G in (G64[:NL], G32[:NL]):
        assert bool((G < c["gamma"]).any()) and bool((G > c["gamma"]).any())       # both branches in the one sample
        assert float((c["gamma"] - G).abs().min()) >= DC.HINGE_MARGIN
    a, j = c["on_atom"]
    y32 = c["pos"][a] + c["offset"][0]                                              # fp32, as the kernel adds it
    assert torch.equal(y32, c["prot"][j]) and torch.equal(c["pos"][a].double() + c["offset"][0].double(), c["prot"][j].double())
    u = c["underflow"]
    yu = c["pos"][u] + c["offset"][0]
    assert float((c["prot"][:NF] - yu).norm(dim=1).min()) >= 60.0
    assert float(S32[u]) == 0.0 and S32.dtype == F32                                # the fp32 sum underflows to exactly 0
    assert float(G32[u]) == pytest.approx(-c["sigma"] * math.log(1e-3), rel=1e-6) and G32[u] > c["gamma"]
    g64, g32, _, _ = DC.reference("clash/constructed_nf63")
    assert float(g64[u].abs().max()) == 0 and float(g32[u].abs().max()) == 0
    assert float(g64[a].abs().max()) > 0                                            # the atom on a protein atom still feels the others
    # sample 1 has another protein and another offset
    assert not torch.equal(c["offset"][0], c["offset"][1]) and not torch.equal(c["prot"][:NF], c["prot"][NF:])


def test_clash_random_cases_use_two_proteins_and_a_far_offset():
    for n in RANDOM:
        c = CASES[n]
        if c["kind"] != "clash":
            continue
        assert c["B"] == 2 and c["prot"].shape == (2 * c["NF"], 3)
        assert float(c["offset"][1].norm()) > 100.0 and float(c["offset"][0].norm()) < 10.0
        assert not torch.equal(c["prot"][:c["NF"]], c["prot"][c["NF"]:])


# -------------------------------------------------------------------------------------------- constructed: arms_repul
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("mode", ["min", "all"])
def test_repul_constructed_case_holds_every_edge(mode, dtype):
    c = CASES[f"repul_{mode}/constructed"]
    NL = c["NL"]
    dec = c["decomp"].view(c["B"], NL)
    assert sorted(set(dec[0][dec[0] >= 0].tolist())) == [0, 2, 3]                   # gap at 1
    assert int((dec[0] == 2).sum()) == 1 and int((dec[0] == 3).sum()) == 1          # one-atom arms
    assert bool((dec[c["no_arm_sample"]] == -1).all())
    (p0, p1), (q0, q1) = c["coincident"]
    assert torch.equal(c["pos"][p0], c["pos"][p1]) and dec[0][p0] == dec[0][p1] >= 0
    assert torch.equal(c["pos"][q0], c["pos"][q1]) and dec[0][q0] != dec[0][q1] and min(dec[0][q0], dec[0][q1]) >= 0
    p, q = c["eq_pair"]
    pos = c["pos"].to(dtype)
    assert float(torch.norm(pos[p] - pos[q])) == c["max_d"] == 2.0 and dec[0][p] != dec[0][q]
    g = DC.repul_grad(c, dtype)
    assert bool(torch.isfinite(g).all())
    assert float(g[NL:2 * NL].abs().max()) == 0
    if mode == "min":                                                               # no exact cross-arm tie at a minimum (out of scope)
        _, mins = DC.repul_pairs(c, dtype)
        assert all(v[3] > v[2] for v in mins.values())
    else:
        # the pair at exactly max_d carries -+1 / (n1 n2 B) along x (inclusive hinge) and is atom q's only partner within max_d
        n1, n2 = int((dec[0] == dec[0][p]).sum()), int((dec[0] == dec[0][q]).sum())
        want = 1.0 / (n1 * n2 * c["B"])
        assert float(g[q][0]) == pytest.approx(-want, rel=1e-6) and float(g[q][1:].abs().max()) == 0


# ------------------------------------------------------------------------------------- the oracle's own conventions
def _armsca(x, decomp, min_d, max_d, dtype=F64):
    x = torch.tensor(x, dtype=dtype, requires_grad=True)
    dec = torch.tensor(decomp)
    e, n_valid = OD.armsca_prox_loss(x, torch.zeros(len(decomp), dtype=torch.long), dec, min_d, max_d)
    return torch.autograd.grad(e, x)[0], n_valid


@pytest.mark.parametrize("dtype", [F64, F32])
def test_oracle_armsca_has_a_zero_subgradient_on_coincident_atoms(dtype):
    g, n_valid = _armsca([[0, 0, 0], [0, 0, 0], [1, 0, 0]], [0, -1, -1], 1.2, 1.9, dtype)
    assert n_valid == 1 and torch.equal(g, torch.zeros(3, 3, dtype=dtype))


@pytest.mark.parametrize("dtype", [F64, F32])
def test_oracle_armsca_hinge_is_inclusive_at_equality(dtype):
    g, _ = _armsca([[0, 0, 0], [2, 0, 0]], [0, -1], 1.2, 2.0, dtype)
    assert torch.equal(g, torch.tensor([[-1, 0, 0], [1, 0, 0]], dtype=dtype))


@pytest.mark.parametrize("dtype", [F64, F32])
def test_oracle_armsca_skips_an_arm_id_without_atoms(dtype):
    """torch_scatter's scatter_min leaves 0 in an empty slot and passes no gradient; the mean still runs over max id + 1 arms."""
    g, _ = _armsca([[0, 0, 0], [3, 0, 0], [1, 0, 0], [5, 0, 0]], [0, 2, -1, -1], 1.2, 1.9, dtype)
    third = torch.tensor(1.0, dtype=dtype) / 3
    assert torch.equal(g[1], torch.stack([third, third * 0, third * 0])), g       # (2/3 with an empty slot that gathers the last row)
    assert torch.equal(g[0], torch.stack([third, third * 0, third * 0]))
    assert float(g.sum(0).abs().max()) < 1e-7


def test_oracle_scatter_min_empty_slots_hold_zero_and_pass_no_gradient():
    src = torch.tensor([[3.0, -1.0], [2.0, 5.0], [7.0, -4.0]], dtype=F64, requires_grad=True)
    index = torch.tensor([0, 3, 3])
    vals, arg = OO.scatter_min(src, index, dim=0)
    assert vals.shape == (4, 2) and arg.shape == (4, 2)
    assert torch.equal(vals.detach(), torch.tensor([[3.0, -1.0], [0.0, 0.0], [0.0, 0.0], [2.0, -4.0]], dtype=F64))
    assert torch.equal(arg, torch.tensor([[0, 0], [3, 3], [3, 3], [1, 2]]))        # empty: src.size(0)
    (vals * torch.tensor([[1.0, 2.0], [10.0, 20.0], [100.0, 200.0], [3.0, 4.0]], dtype=F64)).sum().backward()
    assert torch.equal(src.grad, torch.tensor([[1.0, 2.0], [3.0, 0.0], [0.0, 4.0]], dtype=F64))
    # no empty slot: the plain gather
    v2, a2 = OO.scatter_min(src.detach(), torch.tensor([1, 0, 1]), dim=0)
    assert torch.equal(v2, torch.tensor([[2.0, 5.0], [3.0, -4.0]], dtype=F64)) and torch.equal(a2, torch.tensor([[1, 1], [0, 2]]))


def test_sampler_batch_has_one_scaffold_atom_on_an_arm_atom_and_generic_margins_elsewhere():
    b = DC.sampler_batch()
    dec, pos = b["ligand_decomp_index"], b["init_ligand_pos"]
    assert pos.shape == (24, 3) and b["protein_pos"].shape == (80, 3)             # 40 + 12 atoms, B = 2
    assert int(dec[0]) == 0 and int(dec[8]) == -1 and torch.equal(pos[0], pos[8])
    h, w, cm, same, a = DC.sampler_margins(b)
    assert h >= DC.HINGE_MARGIN and w >= DC.WINNER_MARGIN and cm >= DC.HINGE_MARGIN and same
    for dtype in (F64, F32):                                                      # still coincident after centring, in both precisions
        win = DC.armsca_winners(a, dtype)
        assert win[(0, 0)][:3] == (0, 8, 0.0)
    d = torch.cdist(pos[:12].double(), pos[:12].double())
    d[0, 8] = d[8, 0] = 1.0
    assert float((d + torch.eye(12)).min()) > 0.1                                  # no other coincidence
