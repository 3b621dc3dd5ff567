"""The general distance restraints (typed atoms, ligand-ligand pairs, the harmonic form, per-step distances; dd_drift_restraint2 and the
new keys of the ``restraint`` entry of ``energy_drift_opt``) on the GPU.

1. The kernel through the C ABI at every case of tests/restraint2_cases.py against the gradient of the energy under float64 autograd
   (bounds from the float64 / fp32 oracle pair, never from the kernel), with dist / winner / winner2, accumulate = 0 onto NaN and = 1
   onto a known buffer.
2. Bit equality with the point kernel on old-form cases; reproducibility; the refusals.
3. A chain whose entry uses none of the new keys runs the point kernel and gives the bits of the same entry on the general kernel.
4. One reverse step on the device's own draws subtracts the oracle's gradient at (x_t, v_t), within the gradient's bound.
5. Compositions by ``torch.equal`` on chains of 6 steps at the small shapes of tests/test_gpu_restraint.py.
6. Trajectories against launches on the recorded states.
7. The harness: ``restraints_fn`` with the new keys gives the same sample under batch sizes 1 and 3."""
import ctypes
import math

import pytest
import torch

import restraint2_cases as C
import restraint_cases as RC
from decompdiff_amd import DecompScorePosNet3D, RESTRAINT_ANY, RESTRAINT_NONE, harness, hip_lib, synth
from test_gpu_fixed_atoms import philox_draws
from test_gpu_parity import _sample_hip, dev, maxabs, model
from test_gpu_restraint import STEPS, launch as launch_point, pair, run_rs, ulp
from test_gpu_sample_keys import KEYS, POCKETS, TRAJ, assert_same, single, split

pytestmark = pytest.mark.gpu
CASES = C.all_cases()
GENERAL = ("cls", "cls2", "pair", "atom2", "group2", "form")


def bits32(mask):
    """int64 class masks as the int32 tensor with the same low 32 bits."""
    return torch.where(mask >= 2 ** 31, mask - 2 ** 32, mask).to(torch.int32)


# ------------------------------------------------------------------------------------------------ 1: the kernel
def launch(case, out, accumulate, dist=None, winner=None, winner2=None, run_state=None, t_min=0, t_max=999, NL=None, decomp="case",
           v="case", R=None, drop=(), traj=None, traj_positions=0):
    """dd_drift_restraint2 on the case -> status (synchronised).  Every general array the case has is handed over (a case without class
    masks hands none); drop: names left NULL; run_state: (steps done, t_start) or None; traj: dict of device buffers or None."""
    lib, d = hip_lib.load(), dev()
    i32 = lambda t: t.to(device=d, dtype=torch.int32).contiguous()
    f32 = lambda t: t.to(device=d, dtype=torch.float32).contiguous()
    x = f32(case["pos"])
    dec = case["decomp"] if decomp == "case" else decomp
    dec = None if dec is None else i32(dec)
    lv = case.get("v") if v == "case" else v
    lv = None if lv is None else i32(lv)
    nlr = None if case["nl_real"] is None else i32(torch.tensor(case["nl_real"]))
    arrays = [i32(case["ptr"]), f32(case["point"]), f32(case["min_d"]), f32(case["max_d"]), f32(case["weight"]), i32(case["atom"]),
              i32(case["group"])]
    general = {}
    for k in GENERAL:
        t = case.get(k)
        if t is not None and k not in drop:
            general[k] = i32(bits32(t.long())) if k in ("cls", "cls2") else i32(t)
    general.update(traj or {})
    rs = hip_lib.restraints_struct(case["R"] if R is None else R, *arrays, False, t_min, t_max, traj_positions=traj_positions, **general)
    ctr = None if run_state is None else i32(torch.tensor([run_state[0], run_state[1], 0, 0]))
    rc = lib.dd_drift_restraint2(hip_lib.ptr(x), hip_lib.ptr(lv), hip_lib.ptr(dec), hip_lib.ptr(nlr), case["B"], case["NL"] if NL is None else NL,
                                 ctypes.byref(rs), hip_lib.ptr(ctr), hip_lib.ptr(out), accumulate, hip_lib.ptr(dist), hip_lib.ptr(winner),
                                 hip_lib.ptr(winner2), hip_lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def outputs(case, fill=float("nan")):
    n, R = case["B"] * case["NL"], case["R"]
    return (torch.full((n, 3), fill, device=dev()), torch.full((R,), float("nan"), device=dev()),
            torch.full((R,), -7, dtype=torch.int32, device=dev()), torch.full((R,), -7, dtype=torch.int32, device=dev()))


@pytest.mark.parametrize("name", C.NAMES)
def test_kernel_vs_float64_autograd(name):
    case, ref = CASES[name], C.reference(name)
    n, R, NL = case["B"] * case["NL"], case["R"], case["NL"]
    out, dist, win, win2 = outputs(case)                                 # accumulate = 0 must write every row
    hip_lib.check(launch(case, out, 0, dist, win, win2), name)
    buf = C.known_buffer(name, (n, 3))
    acc = buf.to(dev()).contiguous()                                     # accumulate = 1 adds onto what is there
    hip_lib.check(launch(case, acc, 1), name)
    out, acc, dist, win, win2 = out.cpu(), acc.cpu(), dist.cpu(), win.cpu().long(), win2.cpu().long()
    finite = bool(torch.isfinite(out).all()) and bool(torch.isfinite(acc).all())
    err = maxabs(out, ref["g64"]) if finite else float("nan")
    err_acc = maxabs(acc, buf.double() + ref["g64"]) if finite else float("nan")
    bnd = ref["bound"]
    bnd_acc = bnd + float(buf.abs().max()) * 2.0 ** -23                  # buffer + gradient is rounded once more, at the buffer's size
    fin = torch.isfinite(ref["dist"])
    err_d = maxabs(dist[fin], ref["dist"][fin]) if bool(fin.any()) else 0.0
    bnd_d = C.dist_bound(ref)
    C.report(name, err, ref["d32"], bnd, f" err_acc={err_acc:.3g} bound_acc={bnd_acc:.3g} err_dist={err_d:.3g} bound_dist={bnd_d:.3g} "
                                         f"|g|={float(ref['g64'].abs().max()):.3g} cmax={ref['cmax']:.3g} R={R}")
    assert finite, (name, out[~torch.isfinite(out).all(1)][:4])
    assert err < bnd, (name, err, bnd)
    assert err_acc < bnd_acc, (name, err_acc, bnd_acc)
    assert torch.equal(win, ref["winner"]), (name, win, ref["winner"])
    assert torch.equal(win2, ref["winner2"]), (name, win2, ref["winner2"])
    assert err_d <= bnd_d, (name, err_d, bnd_d)
    assert bool(torch.isinf(dist[~fin]).all()) and bool((dist[~fin] > 0).all())       # an empty set: +inf (and winners -1 above)
    if "empty_sample" in case:                                            # a sample without restraints: zeros over the NaN
        rows = slice(case["empty_sample"] * NL, (case["empty_sample"] + 1) * NL)
        assert torch.equal(out[rows], torch.zeros(NL, 3)) and torch.equal(acc[rows], buf[rows])
    if case["nl_real"] is not None:                                       # padding rows: zeros, never a gradient
        for b, nr in enumerate(case["nl_real"]):
            assert torch.equal(out[b * NL + nr:(b + 1) * NL], torch.zeros(NL - nr, 3)), (name, b)
    if "expect_rows" in case:
        want = torch.zeros(n, 3, dtype=torch.float64)
        for row, val in case["expect_rows"].items():
            want[row] = torch.tensor(val, dtype=torch.float64)
        assert maxabs(out, want) < bnd, (name, out)
    if "zero_d" in case:                                                  # d == 0: winners reported, nothing added
        assert all(float(dist[r]) == 0.0 and int(win[r]) >= 0 and int(win2[r]) >= 0 for r in case["zero_d"])
    # a pair's two ends carry exactly opposite rows when nothing else touches them
    if name == "pair_tie_in_wave_nl64":
        assert torch.equal(out[5], -out[9])


# ------------------------------------------------------------------------------------------------ 2: the two kernels, refusals
@pytest.mark.parametrize("NL", [2, 64, 65, 128])
def test_bit_equality_with_the_point_kernel(NL):
    """A point / linear / untyped case through dd_drift_restraint, and through dd_drift_restraint2 with an all-ones class mask (which
    sends the launch to the general kernel): the same bits in grad, dist and winner."""
    case = C.old_form_case(NL)
    n, R = case["B"] * case["NL"], case["R"]
    old, d_old, w_old, _ = outputs(case)
    hip_lib.check(launch_point(case, old, 0, d_old, w_old), "dd_drift_restraint")
    forced = dict(case, v=torch.arange(n) % 8, cls=torch.full((R,), C.ALL, dtype=torch.long))
    new, d_new, w_new, w2_new = outputs(case)
    hip_lib.check(launch(forced, new, 0, d_new, w_new, w2_new), "dd_drift_restraint2")
    assert float(old.abs().max()) > 0.1 and bool(torch.isfinite(old).all())
    assert torch.equal(new, old) and torch.equal(w_new, w_old) and bool((w2_new == -1).all())
    assert torch.equal(d_new.view(torch.int32), d_old.view(torch.int32))              # (bits: +inf of the empty groups included)
    # accumulate = 1 onto the same buffer, and inside / outside a time window
    a_old, a_new = (C.known_buffer("bits", (n, 3)).to(dev()) for _ in range(2))
    hip_lib.check(launch_point(case, a_old, 1, run_state=(3, 503), t_min=400, t_max=600), "dd_drift_restraint")
    hip_lib.check(launch(forced, a_new, 1, run_state=(3, 503), t_min=400, t_max=600), "dd_drift_restraint2")
    assert torch.equal(a_new, a_old) and not torch.equal(a_old.cpu(), C.known_buffer("bits", (n, 3)))
    # without any general array dd_drift_restraint2 IS the point kernel's launch; winner2 is all -1
    plain, d_p, w_p, w2_p = outputs(case)
    hip_lib.check(launch(case, plain, 0, d_p, w_p, w2_p), "dd_drift_restraint2, old form")
    assert torch.equal(plain, old) and torch.equal(w_p, w_old) and bool((w2_p == -1).all())


def test_runs_are_bitwise_reproducible():
    case = CASES["random_nl128_b3"]
    outs = []
    for _ in range(3):
        out, dist, win, win2 = outputs(case)
        hip_lib.check(launch(case, out, 0, dist, win, win2), "dd_drift_restraint2")
        outs.append((out.cpu(), dist.cpu(), win.cpu(), win2.cpu()))
    for k in range(4):
        assert torch.equal(outs[0][k].view(torch.int32), outs[1][k].view(torch.int32)) and torch.equal(outs[0][k].view(torch.int32), outs[2][k].view(torch.int32))


def test_bad_arguments_are_refused_and_nothing_is_written():
    case = CASES["sets_and_classes_b3"]
    n, R = case["B"] * case["NL"], case["R"]

    def refused(**kw):
        out = torch.full((n, 3), 7.0, device=dev())
        dist = torch.full((R,), 7.0, device=dev())
        rc = launch(kw.pop("case", case), out, 0, dist, **kw)
        return rc == -1 and bool((out == 7.0).all()) and bool((dist == 7.0).all())
    pairs = case["pair"]
    assert refused(drop=("atom2", "group2"))                              # pair set with neither atom2 nor group2
    assert refused(case=dict(case, atom2=torch.where(pairs, torch.full_like(case["atom2"], 6), case["atom2"])))      # atom2 == NL
    assert refused(case=dict(case, atom2=torch.full_like(case["atom2"], -2)))
    assert refused(case=dict(case, group2=torch.where(pairs & (case["atom2"] < 0), torch.full_like(case["group2"], -2), case["group2"])))
    assert refused(case=dict(case, group2=torch.where(pairs & (case["atom2"] < 0), torch.full_like(case["group2"], RESTRAINT_NONE), case["group2"])))
    assert refused(decomp=None)                                           # arm / scaffold groups (group2 too) without decomp_index
    only2 = dict(case, atom=torch.full_like(case["atom"], -1), group=torch.full_like(case["group"], RESTRAINT_ANY))
    assert refused(case=only2, decomp=None)                               # ... where only group2 needs it
    assert refused(case=dict(case, form=torch.full_like(case["form"], 2))) and refused(case=dict(case, form=torch.full_like(case["form"], -1)))
    assert refused(v=None)                                                # cls / cls2 given but lig_v NULL
    tr = dict(dist_traj=torch.full((4, R), 7.0, device=dev()))
    assert refused(traj=tr, traj_positions=0, run_state=(0, 999)) and bool((tr["dist_traj"] == 7.0).all())      # trajectory pointers without rows
    assert refused(R=R - 1) and refused(t_min=5, t_max=4)                 # (the existing list still holds)
    # the point entry refuses a struct that carries the general arrays
    out = torch.full((n, 3), 7.0, device=dev())
    lib, i32 = hip_lib.load(), lambda t: t.to(device=dev(), dtype=torch.int32).contiguous()
    f32 = lambda t: t.to(device=dev(), dtype=torch.float32).contiguous()
    arrays = [i32(case["ptr"]), f32(case["point"]), f32(case["min_d"]), f32(case["max_d"]), f32(case["weight"]), i32(case["atom"]), i32(case["group"])]
    form = i32(case["form"])
    rs = hip_lib.restraints_struct(R, *arrays, False, 0, 999, form=form)
    dec, x = i32(case["decomp"]), f32(case["pos"])
    assert lib.dd_drift_restraint(hip_lib.ptr(x), hip_lib.ptr(dec), None, case["B"], case["NL"], ctypes.byref(rs), None, hip_lib.ptr(out), 0, None,
                                  None, hip_lib.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    hip_lib.check(launch(case, out, 0), "the case itself")
    assert not bool((out == 7.0).any())


def test_trajectory_rows_follow_the_run_state():
    """Row `steps done` of the three buffers is written, window open or not; rows at or beyond traj_positions and launches without a
    run state write nothing."""
    name = "random_nl65_b3"
    case, ref = CASES[name], C.reference(name)
    n, R, P = case["B"] * case["NL"], case["R"], 4
    tr = dict(dist_traj=torch.full((P, R), 7.0, device=dev()), winner_traj=torch.full((P, R), -7, dtype=torch.int32, device=dev()),
              winner2_traj=torch.full((P, R), -7, dtype=torch.int32, device=dev()))
    out, dist, win, win2 = outputs(case)
    hip_lib.check(launch(case, out, 0, dist, win, win2, run_state=(2, 502), t_min=0, t_max=10, traj=tr, traj_positions=P), name)   # t = 500: closed
    assert torch.equal(out.cpu(), torch.zeros(n, 3))
    for p in range(P):
        if p == 2:
            assert torch.equal(tr["dist_traj"][p], dist) and torch.equal(tr["winner_traj"][p], win) and torch.equal(tr["winner2_traj"][p], win2)
        else:
            assert bool((tr["dist_traj"][p] == 7.0).all()) and bool((tr["winner_traj"][p] == -7).all()) and bool((tr["winner2_traj"][p] == -7).all())
    assert torch.equal(win.cpu().long(), ref["winner"]) and torch.equal(win2.cpu().long(), ref["winner2"])
    before = {k: t.clone() for k, t in tr.items()}
    hip_lib.check(launch(case, out, 0, run_state=(P, 900), traj=tr, traj_positions=P), name)                   # step == traj_positions
    hip_lib.check(launch(case, out, 0, traj=tr, traj_positions=P), name)                                       # no run state
    assert all(torch.equal(tr[k], before[k]) for k in tr) and float(out.abs().max()) > 0.1


# ------------------------------------------------------------------------------------------------ 3: old entries keep their kernel
def last_sig():
    return list(DecompScorePosNet3D._chain_cache.values())[-1]["restraint_sig"]


def test_an_entry_without_the_new_keys_runs_the_point_kernel_and_the_general_kernel_gives_its_bits():
    m, b = model(0), pair(41)
    e = RC.batch_entry(b, 41, weight=(0.1, 0.3), scale=True)
    want, rw = run_rs(m, b, e, seed=5)                                    # (recorded here: the point kernel's chain)
    assert last_sig()[4] == "point" and last_sig()[5] == 0
    assert "restraint_atom2" not in rw and "restraint_dist_traj" not in rw
    neutral, rn = run_rs(m, b, dict(e, classes=None, classes2=None, atom2=None, group2=None, form="linear", traj=False), seed=5)
    assert last_sig()[4] == "point"
    assert_same(neutral, want, "neutral spellings")
    # the same entry forced onto the general kernel (every class allowed): the same chain, bit for bit
    forced, rf = run_rs(m, b, dict(e, classes=[list(range(8))] * int(e["sample"].numel())), seed=5)
    assert last_sig()[4] == "general"
    assert_same(forced, want, "general kernel")
    for k in ("restraint_dist", "restraint_atom"):
        assert torch.equal(rf[k], rw[k]) and torch.equal(rn[k], rw[k]), k
    assert maxabs(want["pos"], run_rs(m, b, None, seed=5)[0]["pos"]) > 1e-3


# ------------------------------------------------------------------------------------------------ 4: one reverse step
def one_step(m, b, drift, t, **kw):
    """One reverse step at time t -> (result, the chain's CENTRED coordinates after it: the frame the step computes in)."""
    r = _sample_hip(m, b, 1, drift, kw.pop("noise", None), t, **kw)
    torch.cuda.synchronize()
    return r, m._last[1]["lig_pos"].detach().cpu().view(-1, 3).clone()


@pytest.mark.parametrize("variant", ["alone", "scaled"])
def test_one_reverse_step_subtracts_the_gradient(variant):
    """Positions after one step with a typed pair harmonic entry = the same step without it minus the float64 oracle's gradient at
    (x_t, v_t) (times pos_score_coef[t] with ``scale``), within the gradient's own bound (restraint2_cases: FLAT times the largest
    coefficient, or twice the fp32 oracle's distance) and nothing added to it.  Both calls draw on the device with the same seed -- the
    path production chains take; the draws of that position, read through dd_debug_philox and injected into a third call, give the
    seeded call's bits, so what cancels between the two calls is exactly that noise.  The comparison is made in the chain's centred
    frame, where the step computes: coordinates stay below 8 A there, so the three roundings that do not cancel (mean - g, and the sum
    with the noise in either call) are at most half an ulp of 8 each, 7.2e-7 in all, inside the bound of 1.05e-6; the caller's frame would add the
    rounding of `+ offset` at coordinates near 16."""
    scaled = variant == "scaled"
    b, entry, case = C.sampler_case(scale=scaled, weight=(0.05, 0.15))
    m, t, seed = model(0), 500, 77
    h, w = C.margins(case)
    assert h >= C.HINGE_MARGIN and w >= C.WINNER_MARGIN and C.same_branches(case)
    ref = C._reference(case)
    g64 = ref["g64"]
    assert float(g64.abs().max()) > 0.03
    plain, plain_c = one_step(m, b, None, t, seed=seed)
    got, got_c = one_step(m, b, [dict(entry, traj=True)], t, seed=seed)
    n, nb = b["init_ligand_pos"].size(0), b["init_ligand_fc_bond_type"].size(0)
    injected, injected_c = one_step(m, b, None, t, noise=philox_draws(seed, [t], n, nb))
    assert torch.equal(injected_c, plain_c) and torch.equal(injected["v"], plain["v"]) and torch.equal(injected["bond"], plain["bond"])
    coef = float(m.pos_score_coef[t]) if scaled else 1.0
    want = plain_c.double() - g64 * coef
    big = max(float(plain_c.abs().max()), float(got_c.abs().max()))
    err, tol = maxabs(got_c, want), ref["bound"]
    print(f"\nRESTRAINT2 step {variant}: err={err:.3g} bound={tol:.3g} (d32={ref['d32']:.3g}, largest centred coordinate {big:.3g}, "
          f"three half ulps {1.5 * ulp(big):.3g}) |g|={float(g64.abs().max()):.3g} coef={coef:.3g} moved={maxabs(got_c, plain_c):.3g}")
    assert big < 8.0 and err <= tol, (variant, err, tol, big)
    assert maxabs(got_c, plain_c) > 0.5 * float(g64.abs().max()) * coef                 # the term acted, at its size
    assert torch.equal(got["v"], plain["v"]) and torch.equal(got["bond"], plain["bond"])
    # the trajectory row of the one position: distances and winners at (x_t, v_t), in the CALLER's order
    order, NL = case["order"], case["NL"]
    flat = lambda w_: torch.where(w_ >= 0, w_ + case["sample"] * NL, w_)
    assert got["restraint_dist_traj"].shape == (1, case["R"])
    assert torch.equal(got["restraint_atom_traj"][0][order], flat(ref["winner"])) and torch.equal(got["restraint_atom2_traj"][0][order], flat(ref["winner2"]))
    fin = torch.isfinite(ref["dist"])
    assert maxabs(got["restraint_dist_traj"][0][order][fin], ref["dist"][fin]) <= C.dist_bound(ref)
    # dist / winners of the final state against the oracle on the state that came back
    final = C.centred_case(b, entry, pos=got["pos"].cpu(), v=got["v"].cpu())
    _, dist, win, win2, _ = C.grad(final, torch.float64)
    assert torch.equal(got["restraint_atom"][final["order"]], flat(torch.tensor(win))) and torch.equal(got["restraint_atom2"][final["order"]], flat(torch.tensor(win2)))
    dist = torch.tensor(dist)
    assert maxabs(got["restraint_dist"][final["order"]][torch.isfinite(dist)], dist[torch.isfinite(dist)]) < 1e-4   # (the returned positions carry the offset, re-subtracted here)


# ------------------------------------------------------------------------------------------------ 5: compositions
RS_KEYS = ("restraint_dist", "restraint_atom", "restraint_atom2", "restraint_dist_traj", "restraint_atom_traj", "restraint_atom2_traj")


def sub_entry(entry, k, n_l):
    """Sample k's share of a general entry over samples of n_l[b] atoms, as an entry for that sample alone."""
    keep = (entry["sample"] == k).nonzero()[:, 0]
    a0 = sum(n_l[:k])
    e = {key: (v[keep] if torch.is_tensor(v) else ([v[i] for i in keep.tolist()] if isinstance(v, list) else v)) for key, v in entry.items()}
    e["sample"] = torch.zeros_like(e["sample"])
    for key in ("atom", "atom2"):
        e[key] = torch.where(e[key] >= 0, e[key] - a0, e[key])
    return e


def same_reports(got, want, what, keys=RS_KEYS):
    for k in keys:
        assert (k in got) == (k in want), (what, k)
        if k in want:
            assert torch.equal(got[k], want[k]), (what, k)


def test_eager_captured_and_streamed_agree_and_the_term_acts(monkeypatch):
    m, b = model(0), pair(31)
    e = C.batch_entry(b, 31, weight=(0.1, 0.3), scale=True, traj=True)
    eager, re_ = run_rs(m, b, e, seed=5, use_graph=False)
    streamed, rs_ = run_rs(m, b, e, seed=5, use_graph=True)
    monkeypatch.setenv("DD_TRAJ_STREAMING", "0")
    captured, rc_ = run_rs(m, b, e, seed=5, use_graph=True)
    monkeypatch.delenv("DD_TRAJ_STREAMING")
    assert_same(captured, eager, "captured")
    assert_same(streamed, eager, "streamed")
    same_reports(rc_, re_, "captured")
    same_reports(rs_, re_, "streamed")
    assert last_sig()[4] == "general" and last_sig()[5] >= STEPS
    assert re_["restraint_dist_traj"].shape == (STEPS, int(e["sample"].numel())) and "restraint_atom2" in re_
    none, _ = run_rs(m, b, None, seed=5)
    assert maxabs(none["pos"], eager["pos"]) > 1e-3 and all(k in eager for k in TRAJ)
    # a harmonic entry is not the linear one
    lin, _ = run_rs(m, b, dict(e, form="linear"), seed=5)
    assert not torch.equal(lin["pos"], eager["pos"])


def test_padded_grouped_and_alone_agree(monkeypatch):
    """Ligands of 9, 8 and 6 atoms as one padded batch, as size groups, and each sample alone: the same chain per sample, the same
    restraint reports and trajectories."""
    m = model(0)
    n_l = [9, 8, 6]
    singles = [single(n, 300 + k) for k, n in enumerate(n_l)]
    batch = synth.concat_sampling_batches(singles)
    e = C.batch_entry(batch, 32, per_sample=(3, 4, 4), weight=(0.1, 0.3), traj=True)
    keys = KEYS[:3]
    alone = [run_rs(m, s, sub_entry(e, k, n_l), seed=keys[k]) for k, s in enumerate(singles)]
    padded, rp = run_rs(m, batch, e, sample_keys=keys)
    monkeypatch.setenv("DD_RAGGED_MODE", "groups")
    grouped, rg = run_rs(m, batch, e, sample_keys=keys)
    monkeypatch.delenv("DD_RAGGED_MODE")
    for what, got, r in (("padded", padded, rp), ("grouped", grouped, rg)):
        for k, part in enumerate(split(got, n_l)):
            assert_same(part, alone[k][0], f"{what}, sample {k}")
            mine = (e["sample"] == k).nonzero()[:, 0]
            a0 = sum(n_l[:k])
            for key in RS_KEYS:
                t = r[key][..., mine]
                if key != "restraint_dist" and key != "restraint_dist_traj":
                    t = torch.where(t >= 0, t - a0, t)
                assert torch.equal(t, alone[k][1][key]), (what, k, key)
    assert bool((rp["restraint_atom2"] >= 0).any()) and bool(torch.isfinite(rp["restraint_dist"]).any())
    assert maxabs(padded["pos"], run_rs(m, batch, None, sample_keys=keys)[0]["pos"]) > 1e-2


def test_a_keyed_sample_with_its_restraints_in_a_batch_of_three_is_that_sample_alone():
    m = model(0)
    singles = [single(8, 310 + k) for k in range(3)]
    batch = synth.concat_sampling_batches(singles)
    e = C.batch_entry(batch, 33, per_sample=(0, 4, 3), weight=(0.1, 0.3), t_min=996)        # sample 0 has none
    got, r = run_rs(m, batch, e, sample_keys=KEYS[:3])
    for k, part in enumerate(split(got, [8] * 3)):
        alone, ra = run_rs(m, singles[k], sub_entry(e, k, [8] * 3), seed=KEYS[k])
        assert_same(part, alone, f"sample {k}")
        mine = (e["sample"] == k).nonzero()[:, 0]
        assert torch.equal(r["restraint_dist"][mine], ra["restraint_dist"]), k
    plain0, _ = run_rs(m, singles[0], None, seed=KEYS[0])
    assert_same(split(got, [8] * 3)[0], plain0, "the sample without restraints")


@pytest.mark.parametrize("resample", [None, dict(jump_length=2, n_resample=2)], ids=["plain", "resampled"])
@pytest.mark.parametrize("mode", ["hold", "replace"])
def test_with_fixed_atoms_held_rows_keep_their_bits_and_the_free_end_moves(mode, resample):
    m, b = model(0), pair(35)
    mask = b["ligand_decomp_index"] == -1
    g = torch.Generator().manual_seed(35)
    n, nb = b["init_ligand_pos"].shape[0], b["init_ligand_fc_bond_type"].numel()
    fx = dict(mask=mask, pos=b["prior_centers"][b["ligand_decomp_batch"]] + 0.8 * torch.randn(n, 3, generator=g),
              v=torch.randint(0, 8, (n,), generator=g), bond=torch.randint(0, 5, (nb,), generator=g), mode=mode)
    # every restraint a harmonic pair arm x scaffold: the scaffold end is held, the arm end is free
    R = 4
    e = dict(type="restraint", sample=torch.tensor([0, 1, 0, 1]), point=None, min_d=0.5, max_d=1.0, weight=0.2,
             group=torch.tensor([0, 0, 1, 1]), group2=torch.full((R,), -1), classes2=[None, list(range(8)), None, [0, 1, 2, 3]],
             form="harmonic", traj=True)
    kw = dict(seed=3, fixed=fx) if resample is None else dict(seed=3, fixed=fx, resample=resample)
    with_rs, r = run_rs(m, b, e, **kw)
    without, _ = run_rs(m, b, None, **kw)
    eager, re_ = run_rs(m, b, e, use_graph=False, **kw)
    assert_same(with_rs, eager, "captured = eager")
    same_reports(r, re_, "captured = eager")
    for k in ("pos", "v", "pos_traj", "v_traj"):
        sel = (lambda t: t[:, mask]) if k.endswith("traj") else (lambda t: t[mask])
        assert torch.equal(sel(with_rs[k]), sel(without[k])), k
    assert maxabs(with_rs["pos"][~mask], without["pos"][~mask]) > 1e-3
    n_pos = STEPS if resample is None else STEPS + 2 * (STEPS // 2)
    assert with_rs["pos_traj"].shape[0] == n_pos and r["restraint_dist_traj"].shape == (n_pos, R)
    if resample is not None:
        assert r["t_traj"].shape[0] == n_pos                             # the rows are those of t_traj
    won = r["restraint_atom_traj"] >= 0
    assert bool(won.any()) and bool(mask[r["restraint_atom2_traj"][won]].all()) and not bool(mask[r["restraint_atom_traj"][won]].any())


def test_other_restraint_values_replay_the_cached_graph():
    m, b = model(0), pair(36)
    e1 = C.batch_entry(b, 36, weight=(0.1, 0.3))
    e2 = C.batch_entry(b, 37, per_sample=(2, 5), weight=(0.2, 0.4))       # other classes, pairs and forms, another split, same capacity
    e2["form"] = e2["form"][::-1]
    run_rs(m, b, e1, seed=1)
    n_entries, n_graphs = len(DecompScorePosNet3D._chain_cache), DecompScorePosNet3D._graph_counter
    got, r = run_rs(m, b, e2, seed=2)
    assert len(DecompScorePosNet3D._chain_cache) == n_entries and DecompScorePosNet3D._graph_counter == n_graphs
    eager, re_ = run_rs(m, b, e2, seed=2, use_graph=False)
    assert_same(got, eager, "replayed graph")
    same_reports(r, re_, "replayed graph")
    assert not torch.equal(got["pos"], run_rs(m, b, e1, seed=2)[0]["pos"])


# ------------------------------------------------------------------------------------------------ 6: trajectories
def relaunch(b, e, pos, v):
    """dd_drift_restraint2 on a recorded state (center_pos_mode="none": the caller's frame is the kernel's) -> (dist, flat winner, flat
    winner2) in the caller's restraint order."""
    case = C.centred_case(b, e, pos=pos, v=v, centre=False)
    out, dist, win, win2 = outputs(case)
    hip_lib.check(launch(case, out, 0, dist, win, win2), "dd_drift_restraint2")
    R, NL = case["R"], case["NL"]
    flat = lambda w_: torch.where(w_ >= 0, w_ + case["sample"] * NL, w_)
    back = lambda t: torch.empty_like(t).index_copy_(0, case["order"], t)
    return back(dist.cpu()), back(flat(win.cpu().long())), back(flat(win2.cpu().long()))


def check_traj(b, e, r, out):
    for p in range(out["pos_traj"].shape[0]):
        pos, v = (b["init_ligand_pos"], b["init_ligand_v"]) if p == 0 else (out["pos_traj"][p - 1], out["v_traj"][p - 1])
        dist, win, win2 = relaunch(b, e, pos, v)
        assert torch.equal(r["restraint_dist_traj"][p], dist), p
        assert torch.equal(r["restraint_atom_traj"][p], win) and torch.equal(r["restraint_atom2_traj"][p], win2), p
    dist, win, win2 = relaunch(b, e, out["pos"], out["v"])                  # the final report is that of the final state
    assert torch.equal(r["restraint_dist"], dist) and torch.equal(r["restraint_atom"], win) and torch.equal(r["restraint_atom2"], win2)


def test_trajectories_are_the_launches_on_the_recorded_states():
    m, b = model(0), pair(38)
    e = C.batch_entry(b, 38, weight=(0.1, 0.3), traj=True)
    kw = dict(seed=9, center_pos_mode="none")
    out, r = run_rs(m, b, e, **kw)
    assert r["restraint_dist_traj"].dtype == torch.float32 and r["restraint_atom_traj"].dtype == torch.int64 and r["restraint_atom2_traj"].dtype == torch.int64
    assert r["restraint_dist_traj"].shape == r["restraint_atom_traj"].shape == r["restraint_atom2_traj"].shape == (STEPS, int(e["sample"].numel()))
    check_traj(b, e, r, out)
    assert not torch.equal(r["restraint_dist_traj"][0], r["restraint_dist_traj"][STEPS - 1])
    # traj does not depend on keep_traj
    lean, rl = run_rs(m, b, e, keep_traj=False, **kw)
    assert torch.equal(lean["pos"], out["pos"]) and "pos_traj" not in lean
    same_reports(rl, r, "keep_traj=False")
    # outside the window: the chain without the term, the rows still written
    closed = dict(e, t_min=0, t_max=0)
    off, ro = run_rs(m, b, closed, **kw)
    plain, _ = run_rs(m, b, None, **kw)
    assert_same(off, plain, "window closed")
    check_traj(b, closed, ro, off)
    assert bool(torch.isfinite(ro["restraint_dist_traj"]).any())
    # without pairs there is no second-atom trajectory
    e1 = RC.batch_entry(b, 38, weight=(0.1, 0.3), traj=True)
    _, r1 = run_rs(m, b, e1, **kw)
    assert "restraint_dist_traj" in r1 and "restraint_atom2_traj" not in r1 and "restraint_atom2" not in r1


# ------------------------------------------------------------------------------------------------ 7: the harness
def test_harness_restraints_fn_with_the_new_keys_gives_the_same_sample_under_any_batch_size():
    m, pocket = model(0), POCKETS[8]
    centre = torch.from_numpy(pocket.prior_centers).float().mean(0)

    def fn(g, dec):
        gen = torch.Generator().manual_seed(1000 + g)
        if g == 1:
            return None
        n = int(dec.numel())
        if g == 2:                                                        # pairs only: no point
            return dict(min_d=0.5, max_d=1.0, weight=0.2, atom=torch.tensor([0, -1]), atom2=torch.tensor([n - 1, -1]),
                        group=torch.tensor([RESTRAINT_ANY, 0]), group2=[None, -1], classes2=[None, [0, 1, 2, 3]], form="harmonic")
        return dict(point=centre + torch.randn(3, 3, generator=gen), min_d=0.5, max_d=torch.tensor([1.0, 1.5, math.inf]), weight=0.2,
                    atom=torch.tensor([n - 1, -1, -1]), group=torch.tensor([RESTRAINT_ANY, -1, 0]), group2=[None, None, 1],
                    classes=[None, [1, 2, 3, 4], None], form=["linear", "harmonic", "harmonic"])
    job = lambda bs: harness.sample_diffusion_ligand_decomp(m, pocket, num_samples=3, batch_size=bs, device="cuda:0", num_steps=3,
                                                            init="device", sample_key_seed=7, restraints_fn=fn,
                                                            restraint_opts=dict(scale=True, traj=True))
    one, three = job(1), job(3)
    for k in one:
        if k == "time_list":
            continue
        assert len(one[k]) == len(three[k]) == 3, k
        for g in range(3):
            assert (one[k][g] == three[k][g]).all() and one[k][g].shape == three[k][g].shape, (k, g)
    assert one["restraint_dist"][1].shape == (0,) and one["restraint_atom2"][0].shape == (3,) and one["restraint_dist_traj"][2].shape == (3, 2)
    assert int(one["restraint_atom"][2][0]) == 0 and int(one["restraint_atom2"][2][0]) == 7 and int(one["restraint_atom2"][0][0]) == -1
    plain = harness.sample_diffusion_ligand_decomp(m, pocket, num_samples=3, batch_size=3, device="cuda:0", num_steps=3, init="device",
                                                   sample_key_seed=7)
    assert (plain["pred_pos"][1] == one["pred_pos"][1]).all() and not (plain["pred_pos"][2] == one["pred_pos"][2]).all()
