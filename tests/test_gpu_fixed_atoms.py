"""Fixed atoms (``sample_diffusion(fixed=...)``, dd_sample_steps_fixed / dd_graph_create_fixed / dd_fixed_init) on the GPU.

References.  Free rows: the oracle (``oracle.diffusion.sample_diffusion``) driven one step at a time with that step's draws, the held
rows overwritten in between by this file's float64 restatement of the header's formulas (`forward_level`).  Held rows: that
restatement itself -- they depend on the known values and the row's draws only.  Compositions (eager / captured / padded / grouped /
split / alone) are ``torch.equal``.

Shapes: pockets of 40-48 atoms, ligands of 6-9 atoms (knn 32: every sample has knn + 1 atoms, so ragged batches take the padded
route), B <= 3, chains of at most 6 steps.  The atom and bond rows of a batch fill more than one block of the step launch, 6 / 8 atoms
inside a padded width of 9 move the bond rows, and 13 atom classes run the second instantiation of the atom template."""
import functools
import math

import pytest
import torch

import golden_utils as GU
from decompdiff_amd import batch_layout as BL
from decompdiff_amd import harness, hip_lib, pocket_data, synth
from oracle import diffusion as OD
from oracle import ops as OO
from test_gpu_parity import POS_TOL, dev, maxabs, model
from test_gpu_sample_keys import KEYS, POCKETS, TRAJ, assert_same, model_nc, run, single, split

pytestmark = pytest.mark.gpu
DRIFT = [dict(type="armsca_prox", min_d=1.2, max_d=1.9), dict(type="clash", sigma=2.0, gamma=4.0)]
LOG_ZERO = math.log(1e-30)                                 # log(clamp(onehot, 1e-30)) off the class


# ------------------------------------------------------------------------------------------------ inputs
def pair(seed, nl=8, nc=8):
    """A dense batch of two samples of the pocket with `nl` ligand atoms."""
    torch.manual_seed(seed)
    return synth.build_sampling_batch(POCKETS[nl], 2, num_classes=nc)


def known(b, mask, seed, mode, nc=8, **kw):
    """A `fixed` dict: known coordinates around the atoms' prior centres, random known classes on EVERY row (free rows: never read)."""
    g = torch.Generator().manual_seed(seed)
    n, nb = b["init_ligand_pos"].shape[0], b["init_ligand_fc_bond_type"].numel()
    pos = b["prior_centers"][b["ligand_decomp_batch"]] + 0.8 * torch.randn(n, 3, generator=g)
    return dict(mask=mask.clone(), pos=pos, v=torch.randint(0, nc, (n,), generator=g), bond=torch.randint(0, 5, (nb,), generator=g),
                mode=mode, **kw)


def scaffold(b):
    return b["ligand_decomp_index"] == -1


def held_bonds(b, mask):
    fc = b["ligand_fc_bond_index"]
    return mask[fc[0]] & mask[fc[1]]


def fixed_rows(fx, n_l, k):
    """Sample k's share of a flat `fixed` whose samples have n_l[b] ligand atoms."""
    a0, b0 = sum(n_l[:k]), sum(n * (n - 1) for n in n_l[:k])
    n = n_l[k]
    out = {key: fx[key][a0:a0 + n] for key in ("mask", "pos", "v")}
    out["bond"] = fx["bond"][b0:b0 + n * (n - 1)]
    out.update({key: fx[key] for key in ("mode", "init") if key in fx})
    return out


def offsets(b):
    return OO.scatter_mean(b["protein_pos"], b["batch_protein"], dim=0)       # decompdiff.py:20-32, as the oracle takes it


def ulp(x):
    return 2.0 ** (math.floor(math.log2(x)) - 23)


# ------------------------------------------------------------------------------------------------ float64 restatement
def forward_level(m, b, fx, level, u_v, u_b, eps, off):
    """Level `level` of the forward process (decompdiff.py:436-455, transitions.py:146-150) for EVERY row from the clean values of
    `fx` and one step's draws, float64: centred coordinates xc [n,3], classes v [n] / bond [n_bond], the smallest gap between the two
    best Gumbel scores of a row (atoms, bonds), and the largest magnitude that enters the coordinate formula.  `off` [B,3]: the
    centring offset; x0c and cc are the fp32 differences the library forms."""
    ac = m.alphas_cumprod.detach().double().cpu()
    A, S = ac[level].sqrt(), (1.0 - ac[level]).sqrt()
    off_l = off[b["batch_ligand"]]
    x0c = (fx["pos"].float() - off_l).double()
    cc = (b["prior_centers"].float()[b["ligand_decomp_batch"]] - off_l).double()
    std = b["prior_stds"].double()[b["ligand_decomp_batch"]]
    noise = S * eps.double() * std
    xc = A * (x0c - cc) + noise + cc
    big = max(float(t.abs().max()) for t in (x0c, cc, x0c - cc, noise, xc))

    def classes(tr, v0, u):
        K = u.shape[-1]
        log_v0 = torch.full((v0.numel(), K), LOG_ZERO, dtype=torch.float64)
        log_v0[torch.arange(v0.numel()), v0] = 0.0
        a, c = log_v0 + tr.log_alphas_cumprod_v.detach().double().cpu()[level], \
            tr.log_one_minus_alphas_cumprod_v.detach().double().cpu()[level] + tr.prior_probs.detach().double().cpu().reshape(-1)
        mx = torch.max(a, c)
        score = -torch.log(-torch.log(u.double() + 1e-30) + 1e-30) + mx + torch.log(torch.exp(a - mx) + torch.exp(c - mx))
        top = score.topk(2, dim=-1).values
        return score.argmax(-1), top[:, 0] - top[:, 1]
    v, gap_v = classes(m.atom_type_trans, fx["v"], u_v)
    bond, gap_b = classes(m.bond_type_trans, fx["bond"], u_b)
    return dict(xc=xc, v=v, bond=bond, gap_v=gap_v, gap_b=gap_b, big=big)


def oracle_loop(m, b, fx, steps, draws, t0, drift=None, start=None):
    """The chain of `steps` steps from time t0: every step is the oracle's (one step, that step's draws), then the held rows are
    overwritten -- hold: the known values; replace: `forward_level` at t - 1 with the same draws (t = 0: the clean values).
    `start`: the state in front of the first step (default: the batch's, with the held rows as the mode prepares them)."""
    cfg, sd = GU.weights(0)
    mask, hb = fx["mask"], held_bonds(b, fx["mask"])
    off = offsets(b)
    off_l = off[b["batch_ligand"]].double()
    pos, v, bond = (start or {}).get("pos", b["init_ligand_pos"]).clone(), (start or {}).get("v", b["init_ligand_v"]).clone(), \
        (start or {}).get("bond", b["init_ligand_fc_bond_type"]).clone()
    if fx["mode"] == "hold":
        pos[mask], v[mask], bond[hb] = fx["pos"][mask], fx["v"][mask], fx["bond"][hb]
    out = {k: [] for k in ("pos", "v", "bond", "gap")}
    for i in range(steps):
        t = t0 - i
        noise = {k: draws[k][i:i + 1] for k in ("u_v", "u_b", "eps")}
        state = dict(b, init_ligand_pos=pos, init_ligand_v=v, init_ligand_fc_bond_type=bond)
        r = OD.sample_diffusion(sd, cfg, num_steps=1, t_start=t, noise=noise, energy_drift_opt=drift, keep_traj=False, **state)
        pos, v, bond = r["pos"].clone(), r["v"].clone(), r["bond"].clone()
        if fx["mode"] == "hold" or t == 0:
            pos[mask], v[mask], bond[hb] = fx["pos"][mask], fx["v"][mask], fx["bond"][hb]
        else:
            lv = forward_level(m, b, fx, t - 1, noise["u_v"][0], noise["u_b"][0], noise["eps"][0], off)
            pos[mask], v[mask], bond[hb] = (lv["xc"] + off_l)[mask].float(), lv["v"][mask], lv["bond"][hb]
            out["gap"].append(min(float(lv["gap_v"][mask].min()), float(lv["gap_b"][hb].min()) if bool(hb.any()) else 9.0))
        for k, t_ in (("pos", pos), ("v", v), ("bond", bond)):
            out[k].append(t_.clone())
    return {k: (torch.stack(val) if k != "gap" else val) for k, val in out.items()}


# ------------------------------------------------------------------------------------------------ 1: nothing held
@pytest.mark.parametrize("layout", ["dense", "padded"])
@pytest.mark.parametrize("mode", ["hold", "replace"])
def test_all_false_mask_is_the_unfixed_chain(mode, layout):
    m = model(0)
    if layout == "dense":
        b = pair(1)
    else:
        b = synth.concat_sampling_batches([single(8, 10), single(6, 11), single(9, 12)])
        assert BL.fits_padded(BL.BatchLayout([48, 40, 44], [8, 6, 9]), m.config.knn)
    n = b["init_ligand_pos"].shape[0]
    fx = known(b, torch.zeros(n, dtype=torch.bool), 3, mode)
    for kw in (dict(), dict(use_graph=False), dict(keep_traj=False)):       # captured + streamed, eager, captured
        want = run(m, b, 3, seed=77, **kw)
        assert_same(run(m, b, 3, seed=77, fixed=fx, **kw), want, f"{mode} {layout} {kw}")


def test_all_false_mask_thirteen_classes_and_a_held_third():
    """The 13-class instantiation of the atom template: nothing held is the unfixed chain; the scaffold held keeps its classes."""
    m, b = model_nc(13), pair(2, nc=13)
    fx = known(b, torch.zeros(16, dtype=torch.bool), 4, "hold", nc=13)
    assert_same(run(m, b, 3, seed=5, fixed=fx), run(m, b, 3, seed=5), "nothing held")
    fx = known(b, scaffold(b), 4, "hold", nc=13)
    fx["v"][fx["mask"]] = torch.tensor([12, 9, 0, 11, 12, 8])                  # the upper classes too
    r, free = run(m, b, 3, seed=5, fixed=fx), run(m, b, 3, seed=5)
    mask = fx["mask"]
    assert bool((r["v_traj"][:, mask] == fx["v"][mask]).all()) and torch.equal(r["v"][mask], fx["v"][mask])
    assert not torch.equal(r["v0_traj"], free["v0_traj"])                       # the network sees the held atoms


# ------------------------------------------------------------------------------------------------ 2, 3, 9: hold against the oracle loop
@functools.lru_cache(maxsize=None)
def hold_chain(with_drift):
    m, b = model(0), pair(21)
    steps, t0 = 6, m.num_timesteps - 1
    fx = known(b, scaffold(b), 22, "hold")                                      # 3 of 8 atoms per sample
    torch.manual_seed(23)
    draws = synth.draw_step_noise(steps, 16, 2 * 56)
    drift = DRIFT if with_drift else None
    got = run(m, b, steps, noise=draws, fixed=fx, energy_drift_opt=drift)
    want = oracle_loop(m, b, fx, steps, draws, t0, drift)
    return m, b, fx, got, want


@pytest.mark.parametrize("with_drift", [False, True], ids=["plain", "drift"])
def test_hold_held_rows_stay_and_free_rows_follow_the_oracle(with_drift):
    m, b, fx, got, want = hold_chain(with_drift)
    mask, hb = fx["mask"], held_bonds(b, fx["mask"])
    assert int(mask.sum()) == 6 and int(hb.sum()) == 12
    # held rows: the known classes at every step, coordinates bit-constant and within one ulp of the known ones
    assert bool((got["v_traj"][:, mask] == fx["v"][mask]).all()) and bool((got["bond_traj"][:, hb] == fx["bond"][hb]).all())
    for i in range(1, got["pos_traj"].shape[0]):
        assert torch.equal(got["pos_traj"][i][mask], got["pos_traj"][0][mask]), i
    off_l = offsets(b)[b["batch_ligand"]]
    assert torch.equal(got["pos"][mask], ((fx["pos"] - off_l) + off_l)[mask])
    # (two roundings, the centring and the re-adding, each at most half an ulp of the larger of |known| and |known - offset|)
    assert float((got["pos"][mask] - fx["pos"][mask]).abs().max()) <= ulp(max(float(fx["pos"][mask].abs().max()),
                                                                              float((fx["pos"] - off_l)[mask].abs().max())))
    # free rows against the oracle loop: types exact at every step, coordinates within the project's tolerance
    assert torch.equal(got["v_traj"], want["v"]) and torch.equal(got["bond_traj"], want["bond"])
    err = maxabs(got["pos_traj"][:, ~mask], want["pos"][:, ~mask])
    print(f"\nFIXED hold ({'drift' if with_drift else 'plain'}): free rows vs oracle loop over 6 steps, max |dpos| {err:.3g} (tol {POS_TOL:g})")
    assert err < POS_TOL
    # the posterior trajectories stay the network's for held rows too: log-probabilities of a distribution
    assert float((got["vt_traj"][:, mask].exp().sum(-1) - 1).abs().max()) < 1e-4


def test_hold_bonds_with_one_held_endpoint_are_sampled():
    m, b, fx, got, want = hold_chain(False)
    mask, fc = fx["mask"], b["ligand_fc_bond_index"]
    one = mask[fc[0]] ^ mask[fc[1]]
    both = mask[fc[0]] & mask[fc[1]]
    assert int(one.sum()) == 2 * 2 * 3 * 5
    assert torch.equal(got["bond_traj"][:, one], want["bond"][:, one])
    assert bool((got["bond_traj"][:, one] != fx["bond"][one]).any())            # sampled, not held
    assert bool((got["bond_traj"][:, both] == fx["bond"][both]).all())


def test_hold_drift_moves_free_arm_atoms_because_of_held_scaffold_atoms():
    m, b, fx, got, want = hold_chain(True)
    _, _, _, _, plain = hold_chain(False)
    mask = fx["mask"]
    # the armsca energy pairs every arm with its nearest SCAFFOLD atom -- the held ones: its gradient at the prepared state
    x = b["init_ligand_pos"].clone()
    x[mask] = fx["pos"][mask]
    x = (x - offsets(b)[b["batch_ligand"]]).requires_grad_(True)
    e, n_valid = OD.armsca_prox_loss(x, b["batch_ligand"], b["ligand_decomp_index"], DRIFT[0]["min_d"], DRIFT[0]["max_d"])
    g = torch.autograd.grad(e, x)[0]
    arm = b["ligand_decomp_index"] >= 0
    assert n_valid == 2 and float(g[arm & ~mask].abs().max()) > 0 and float(g[mask].abs().max()) > 0
    # ... the free rows feel it (first step already), the held rows do not move although their own gradient is not zero
    assert maxabs(want["pos"][0][~mask], plain["pos"][0][~mask]) > 1e-4
    assert torch.equal(got["pos_traj"][-1][mask], got["pos_traj"][0][mask])


# ------------------------------------------------------------------------------------------------ 4: replace, injected noise
@pytest.mark.parametrize("nc", [8, 13])
@pytest.mark.parametrize("where", ["last", "first"])
def test_replace_with_injected_noise_is_the_forward_process_of_the_clean_values(where, nc):
    """Held rows against the float64 restatement, model frame (center_pos_mode 'none': the trajectory IS the centred state), over
    the LAST six steps (t = 5 .. 0: the clean class nearly always survives, the step at t = 0 restores the clean values) and the
    FIRST six (t = T - 1 ..: the classes are nearly uniform, most rows leave theirs).
    Coordinates: the library forms x from fp32 tables with six fp32 operations (sub, three mul, two add) -- eight roundings of at
    most half an ulp of the largest magnitude `big` that enters: 4 ulp(big).  Types: exact, the restatement's two best Gumbel
    scores are more than 1e-3 apart in every held row at every step (asserted; fp32 scores carry ~1e-5)."""
    m, b = model_nc(nc), pair(31, nc=nc)
    steps, T = 6, m.num_timesteps
    mask = scaffold(b)
    mask[0] = True                                                              # and one arm atom: another centre
    hb = held_bonds(b, mask)
    fx = known(b, mask, 32, "replace", nc=nc, init="given")
    torch.manual_seed(33 if where == "last" else 34)
    draws = synth.draw_step_noise(steps, 16, 2 * 56, num_classes=nc)
    t0 = steps - 1 if where == "last" else T - 1
    r = run(m, b, steps, center_pos_mode="none", noise=draws, fixed=fx, start_step=T - 1 - t0)
    off = torch.zeros(2, 3)
    worst, gap, left = 0.0, 9.0, 0
    for i in range(steps):
        t = t0 - i
        if t == 0:
            break
        lv = forward_level(m, b, fx, t - 1, draws["u_v"][i], draws["u_b"][i], draws["eps"][i], off)
        gap = min(gap, float(lv["gap_v"][mask].min()), float(lv["gap_b"][hb].min()))
        left += int((lv["v"][mask] != fx["v"][mask]).sum()) + int((lv["bond"][hb] != fx["bond"][hb]).sum())
        assert torch.equal(r["v_traj"][i][mask], lv["v"][mask]) and torch.equal(r["bond_traj"][i][hb], lv["bond"][hb]), i
        err, bound = float((r["pos_traj"][i].double() - lv["xc"])[mask].abs().max()), 4 * ulp(lv["big"])
        worst = max(worst, err / bound)
        assert err <= bound, (i, err, bound)
    print(f"\nFIXED replace nc={nc} {where} steps: held coordinates vs float64, worst error / bound {worst:.3f}; smallest score gap "
          f"{gap:.3g}; {left} held rows off their clean class")
    assert gap > 1e-3
    if where == "first":
        assert left > 50                                                        # the draws decide, not the clean class
    else:
        # the step at t = 0 leaves the clean values: types exact, centred coordinates bit-equal to x0c
        assert torch.equal(r["v"][mask], fx["v"][mask]) and torch.equal(r["bond"][hb], fx["bond"][hb])
        assert torch.equal(r["pos"][mask], fx["pos"][mask]) and torch.equal(r["pos_traj"][-1][mask], fx["pos"][mask])
    # free rows were sampled, and v0_traj stays the network's reconstruction for held rows (a log-softmax)
    assert not torch.equal(r["pos"][~mask], b["init_ligand_pos"][~mask])
    assert float((r["v0_traj"][:, mask].exp().sum(-1) - 1).abs().max()) < 1e-4


# ------------------------------------------------------------------------------------------------ 5: replace, Philox, init draw
def philox(seed, t, rows, kind):
    lib = hip_lib.load()
    out = torch.empty(rows * {1: 8, 2: 5, 7: 1}[kind], device=dev())
    hip_lib.check(lib.dd_debug_philox(seed, t, rows, kind, hip_lib.ptr(out), hip_lib.stream_ptr()), "dd_debug_philox")
    torch.cuda.synchronize()
    return out.cpu()


def philox_draws(seed, times, n, nb):
    return {"u_v": torch.stack([philox(seed, t, n, 1).view(n, 8) for t in times]),
            "u_b": torch.stack([philox(seed, t, nb, 2).view(nb, 5) for t in times]),
            "eps": torch.stack([philox(seed, t, 3 * n, 7).view(n, 3) for t in times])}


def test_replace_with_device_noise_draws_level_l_at_time_l_plus_one():
    m, b = model(0), pair(41)
    seed, steps, T = 4242, 4, m.num_timesteps
    mask = scaffold(b)
    hb = held_bonds(b, mask)
    fx = known(b, mask, 42, "replace")
    off = offsets(b)
    off_l = off[b["batch_ligand"]].double()
    # the initial level T - 1, drawn at time T: a chain of no steps returns the prepared state
    d0 = philox_draws(seed, [T], 16, 112)
    lv = forward_level(m, b, fx, T - 1, d0["u_v"][0], d0["u_b"][0], d0["eps"][0], off)
    assert min(float(lv["gap_v"][mask].min()), float(lv["gap_b"][hb].min())) > 1e-3
    r0 = run(m, b, 0, seed=seed, fixed=fx)
    xc0 = m._last[1]["lig_pos"].cpu().view(16, 3)
    assert torch.equal(r0["v"][mask], lv["v"][mask]) and torch.equal(r0["bond"][hb], lv["bond"][hb])
    assert float((xc0.double() - lv["xc"])[mask].abs().max()) <= 4 * ulp(lv["big"])
    assert torch.equal(r0["v"][~mask], b["init_ligand_v"][~mask]) and torch.equal(r0["bond"][~hb], b["init_ligand_fc_bond_type"][~hb])
    assert torch.equal(xc0[~mask], (b["init_ligand_pos"] - off[b["batch_ligand"]])[~mask])
    # all steps: the oracle loop fed with the device's draws of times T - 1 .. T - steps, started from that level
    draws = philox_draws(seed, [T - 1 - i for i in range(steps)], 16, 112)
    start = dict(pos=b["init_ligand_pos"].clone(), v=b["init_ligand_v"].clone(), bond=b["init_ligand_fc_bond_type"].clone())
    start["pos"][mask], start["v"][mask], start["bond"][hb] = (lv["xc"] + off_l)[mask].float(), lv["v"][mask], lv["bond"][hb]
    want = oracle_loop(m, b, fx, steps, draws, T - 1, start=start)
    assert min(want["gap"]) > 1e-3, want["gap"]
    got = run(m, b, steps, seed=seed, fixed=fx)
    assert torch.equal(got["v_traj"], want["v"]) and torch.equal(got["bond_traj"], want["bond"])
    err = maxabs(got["pos_traj"], want["pos"])
    print(f"\nFIXED replace, device noise: all rows vs oracle loop over {steps} steps, max |dpos| {err:.3g} (tol {POS_TOL:g})")
    assert err < POS_TOL


# ------------------------------------------------------------------------------------------------ 6: split chains
@pytest.mark.parametrize("mode", ["hold", "replace"])
def test_split_chain_continues_the_unsplit_one(mode):
    m, b = model(0), pair(51)
    fx = known(b, scaffold(b), 52, mode)
    full = run(m, b, 6, center_pos_mode="none", seed=9, fixed=fx)
    first = run(m, b, 2, center_pos_mode="none", seed=9, fixed=fx)
    b2 = dict(b)
    b2["init_ligand_pos"], b2["init_ligand_v"], b2["init_ligand_fc_bond_type"] = first["pos"], first["v"], first["bond"]
    rest = run(m, b2, 4, center_pos_mode="none", seed=9, fixed=dict(fx, init="given"), start_step=2)
    joined = {k: rest[k] for k in ("pos", "v", "bond")}
    joined.update({k: torch.cat([first[k], rest[k]]) for k in TRAJ})
    assert_same(joined, full, f"{mode}: 2 + 4 steps")
    if mode == "replace":                                                       # the held rows do move in this mode
        assert not torch.equal(full["pos_traj"][0][fx["mask"]], full["pos_traj"][1][fx["mask"]])


# ------------------------------------------------------------------------------------------------ 7, 8: ragged batches
def ragged_case(mode):
    n_l = [8, 6, 9]
    singles = [single(n, 60 + k) for k, n in enumerate(n_l)]
    b = synth.concat_sampling_batches(singles)
    mask = torch.cat([scaffold(singles[0]), torch.zeros(6, dtype=torch.bool), torch.ones(9, dtype=torch.bool)])
    return n_l, singles, b, known(b, mask, 61, mode)


@pytest.mark.parametrize("mode", ["hold", "replace"])
def test_padded_batch_with_different_masks_equals_each_sample_alone(mode, monkeypatch):
    monkeypatch.setenv("DD_RAGGED_MODE", "padded")
    m = model(0)
    n_l, singles, b, fx = ragged_case(mode)
    assert BL.fits_padded(BL.BatchLayout([48, 40, 44], n_l), m.config.knn)
    keys = KEYS[:3]
    alone = [run(m, s, 4, seed=k, fixed=fixed_rows(fx, n_l, i)) for i, (s, k) in enumerate(zip(singles, keys))]
    assert_same(alone[1], run(m, singles[1], 4, seed=keys[1]), "nothing held: the unfixed chain")
    parts = split(run(m, b, 4, sample_keys=keys, fixed=fx), n_l)
    for i in range(3):
        assert_same(parts[i], alone[i], f"{mode}, sample {i}")
    if mode == "hold":                                                          # everything held: the known values come back
        f2 = fixed_rows(fx, n_l, 2)
        off_l = offsets(singles[2])[singles[2]["batch_ligand"]]
        assert torch.equal(parts[2]["v"], f2["v"]) and torch.equal(parts[2]["bond"], f2["bond"])
        assert torch.equal(parts[2]["pos"], (f2["pos"] - off_l) + off_l)
        assert bool((parts[2]["v_traj"] == f2["v"]).all()) and bool((parts[2]["bond_traj"] == f2["bond"]).all())
    # the same samples in another order
    order = [2, 0, 1]
    b2 = synth.concat_sampling_batches([singles[i] for i in order])
    fx2 = {k: torch.cat([fixed_rows(fx, n_l, i)[k] for i in order]) for k in ("mask", "pos", "v", "bond")}
    fx2["mode"] = mode
    parts = split(run(m, b2, 4, sample_keys=[keys[i] for i in order], fixed=fx2), [n_l[i] for i in order])
    for p, i in enumerate(order):
        assert_same(parts[p], alone[i], f"{mode}, sample {i} at position {p}")


@pytest.mark.parametrize("mode", ["hold", "replace"])
def test_grouped_route_equals_the_padded_route(mode, monkeypatch):
    m = model(0)
    n_l, singles, b, fx = ragged_case(mode)
    b = synth.concat_sampling_batches(singles + [single(6, 70)])               # two samples share a size group
    n = b["init_ligand_pos"].shape[0]
    fx = known(b, torch.cat([fx["mask"], torch.tensor([True, False, True, False, False, True])]), 62, mode)
    keys = KEYS[:4]
    monkeypatch.setenv("DD_RAGGED_MODE", "padded")
    want = run(m, b, 3, sample_keys=keys, fixed=fx)
    assert want["pos"].shape[0] == n
    for concurrent in ("0", "1"):
        monkeypatch.setenv("DD_RAGGED_MODE", "groups")
        monkeypatch.setenv("DD_RAGGED_CONCURRENT", concurrent)
        assert_same(run(m, b, 3, sample_keys=keys, fixed=fx), want, f"{mode}, groups (concurrent {concurrent})")


# ------------------------------------------------------------------------------------------------ 10: one graph per shape and mode
def test_cached_graph_serves_other_masks_and_known_values_but_not_the_other_mode(monkeypatch):
    m, b = model(0), pair(81)
    fa = known(b, scaffold(b), 82, "replace")
    fb = known(b, ~scaffold(b), 83, "replace")
    monkeypatch.setenv("DD_CHAIN_CACHE", "1")
    m._evict_chain_cache(0)
    ra = run(m, b, 3, seed=1, fixed=fa)
    assert len(m._chain_cache) == 1
    ent = next(iter(m._chain_cache.values()))
    graph, graph_id = ent["graph"].value, ent["graph_id"]
    assert graph and ent["fixed"] == "replace"
    rb = run(m, b, 3, seed=1, fixed=fb)
    assert len(m._chain_cache) == 1 and next(iter(m._chain_cache.values())) is ent
    assert ent["graph"].value == graph and ent["graph_id"] == graph_id          # the very graph, replayed
    assert_same(rb, run(m, b, 3, seed=1, fixed=fb, use_graph=False), "second mask, eager")
    assert_same(ra, run(m, b, 3, seed=1, fixed=fa, use_graph=False), "first mask, eager")
    assert not torch.equal(ra["pos"], rb["pos"])
    for other in (dict(fixed=dict(fa, mode="hold")), dict()):                   # the other mode, and no fixed atoms: captured again
        ro = run(m, b, 3, seed=1, **other)
        ent = next(iter(m._chain_cache.values()))
        assert len(m._chain_cache) == 1 and ent["graph_id"] != graph_id, other
        graph_id = ent["graph_id"]
        assert_same(ro, run(m, b, 3, seed=1, use_graph=False, **other), f"{list(other)} eager")
    m._evict_chain_cache(0)


def test_separate_step_launches_are_bit_identical_to_the_fused_one(debug_options):
    """k_step_rows / k_step_pos as launches of their own (dd_debug_set_option(7, 0), measurement build) against k_step_all: the
    same row and coordinate bodies under the other grid pick the same classes and write the same bits -- without fixed atoms and
    in both of their modes, dense and padded."""
    if not debug_options:
        return
    lib = hip_lib.load()
    m, b = model(0), pair(85)
    n_l, singles, hb, _ = ragged_case("hold")
    for mode in (None, "hold", "replace"):
        kw, kwh = {}, {}
        if mode is not None:
            kw = dict(fixed=known(b, scaffold(b), 86, mode))
            kwh = dict(fixed=known(hb, torch.cat([scaffold(singles[0]), torch.zeros(6, dtype=torch.bool), torch.ones(9, dtype=torch.bool)]), 87, mode))
        try:
            fused, fused_h = run(m, b, 3, seed=3, **kw), run(m, hb, 3, sample_keys=KEYS[:3], **kwh)
            assert lib.dd_debug_set_option(7, 0) == 0
            apart, apart_h = run(m, b, 3, seed=3, **kw), run(m, hb, 3, sample_keys=KEYS[:3], **kwh)
        finally:
            assert lib.dd_debug_set_option(7, 1) == 0
        assert_same(apart, fused, f"{mode} dense")
        assert_same(apart_h, fused_h, f"{mode} padded")


# ------------------------------------------------------------------------------------------------ 11: the harness
def test_harness_holds_the_scaffold_of_the_reference_ligand():
    """`fixed_fn` end to end: every sample of a 'ref'-sized job keeps the scaffold of the pocket's reference ligand (arm id -1;
    build_batch puts the scaffold rows last) -- its types exactly, its coordinates within the two roundings of centring."""
    m = model(0)
    f = GU.make_pocket_fields(5)
    data = pocket_data.PocketData(**{k: f[k] for k in ("protein_pos", "protein_element", "protein_is_backbone", "protein_atom_to_aa_type",
                                                       "pocket_atom_masks", "num_arms", "num_scaffold", "arms_prior", "scaffold_prior",
                                                       "ligand_atom_mask", "ligand_pos", "full_protein_pos")})
    decomp, ref_pos = data.ligand_atom_mask, data.ligand_pos
    n = decomp.numel()
    sca = decomp == -1
    assert bool(sca[-5:].all()) and int(sca.sum()) == 5 and n == 9
    g = torch.Generator().manual_seed(91)
    ref_v, ref_b = torch.randint(0, 8, (n,), generator=g), torch.randint(0, 5, (n * (n - 1),), generator=g)
    seen = []

    def fixed_fn(index, decomp_of_sample):
        seen.append(index)
        assert torch.equal(decomp_of_sample, decomp)
        return dict(mask=decomp_of_sample == -1, pos=ref_pos, v=ref_v, bond=ref_b)
    torch.manual_seed(92)
    out = harness.sample_diffusion_ligand_decomp(m, data, num_samples=3, batch_size=2, device=dev(), num_steps=3, prior_mode="subpocket",
                                                 num_atoms_mode="ref", sample_key_seed=5, fixed_fn=fixed_fn, fixed_mode="hold")
    assert len(out["pred_pos"]) == 3 and seen == [0, 1, 2]
    off = data.protein_pos.mean(0)
    bound = ulp(max(float(ref_pos[sca].abs().max()), float((ref_pos - off)[sca].abs().max())))
    fc = out["pred_bond_index"][0]
    hb = sca[torch.from_numpy(fc[0])] & sca[torch.from_numpy(fc[1])]
    for k in range(3):
        assert torch.equal(torch.from_numpy(out["pred_v"][k])[sca], ref_v[sca])
        assert torch.equal(torch.from_numpy(out["pred_bond_type"][k])[hb], ref_b[hb])
        diff = float((torch.from_numpy(out["pred_pos"][k]).float() - ref_pos)[sca].abs().max())
        assert diff <= bound, (k, diff, bound)
        assert bool((torch.from_numpy(out["pred_v_traj"][k])[:, sca] == ref_v[sca]).all())
    assert not torch.equal(torch.from_numpy(out["pred_pos"][0])[~sca], torch.from_numpy(out["pred_pos"][1])[~sca])
