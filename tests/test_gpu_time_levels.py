"""Strided sampling (``sample_diffusion(time_levels=...)``) on the GPU: the unchanged kernels held to the respaced tables at every
place a table is read.

References.  (1) The plain chain: a list that is a run of consecutive levels reads the native tables' own entries at the same Philox
words, so the strided call is ``torch.equal`` to the plain one -- alone and under every composition that reads another table (the
fixed table, the jump table, tab_score, the restraint window).  (2) The oracle loop (``oracle.diffusion.sample_diffusion``) run on
respaced tables that THIS file builds in float64 from the oracle's own schedule functions, for a list with gaps.  (3) The float64
restatement of the forward process of tests/test_gpu_fixed_atoms.py (`forward_level`) at the REAL level of the next position.
Compositions (split / alone / padded / grouped / batch size) are ``torch.equal``.

Shapes as in tests/test_gpu_fixed_atoms.py: `pair` (two samples, 48 + 8 atoms), `ragged_case` (8 / 6 / 9 ligand atoms); chains of
at most 12 positions."""
import numpy as np
import pytest
import torch

import golden_utils as GU
from decompdiff_amd import DecompScorePosNet3D, harness, shipped_config, synth
from oracle import diffusion as OD
from test_gpu_fixed_atoms import forward_level, held_bonds, known, pair, philox_draws, ragged_case, scaffold, ulp
from test_gpu_parity import POS_TOL, dev, maxabs, model, to_dev
from test_gpu_resample import times
from test_gpu_sample_keys import KEYS, POCKETS, TRAJ, assert_same, split

pytestmark = pytest.mark.gpu
LEVELS = [999, 600, 250, 40, 3, 0]                         # a list with gaps, S = 6
LAST10 = list(range(9, -1, -1))                            # the last ten levels: S = 10, virtual level = real level
_NOISE_MODEL = []


def mean_model(mean):
    """The shared C0 model, or one synthetic-weight model with model_mean_type = 'noise' (built once)."""
    if mean == "C0":
        return model(0)
    if not _NOISE_MODEL:
        cfg = shipped_config(model_mean_type="noise")
        m = DecompScorePosNet3D(cfg, 29, 10, 8)
        sd = m.state_dict()
        sd.update(synth.synthetic_state_dict(cfg, 0))
        m.load_state_dict(sd, strict=True)
        _NOISE_MODEL.append(m.to(dev()))
    return _NOISE_MODEL[0]


def trun(m, b, steps=None, center_pos_mode="protein", **kw):
    """One call: results, stacked trajectories, ``t_traj`` and the restraint results, on the host."""
    r = m.sample_diffusion(num_steps=steps, center_pos_mode=center_pos_mode, **to_dev(b), **kw)
    out = {k: r[k].cpu() for k in ("pos", "v", "bond")}
    out.update({k: torch.stack(r[k]) for k in TRAJ if len(r[k])})
    out.update({k: r[k].cpu() for k in r if k == "t_traj" or k.startswith("restraint_")})
    return out


def without_t(r):
    return {k: v for k, v in r.items() if k != "t_traj"}


def restraint(b, **kw):
    """One restraint per sample of a `pair`: the nearest atom of the sample within 0.5 A of a point 1 A off its first arm centre."""
    pts = b["prior_centers"][b["ligand_decomp_batch"]][[0, 8]] + torch.tensor([1.0, 0.0, 0.0])
    return dict(type="restraint", sample=torch.tensor([0, 1]), point=pts.float(), min_d=0.0, max_d=0.5, weight=0.5, **kw)


# ------------------------------------------------------------------------------------------------ 1: identities with the plain chain
@pytest.mark.parametrize("mean", ["C0", "noise"])
def test_full_list_and_last_ten_levels_are_the_plain_chain(mean):
    m, b = mean_model(mean), pair(501)
    T = m.num_timesteps
    for kw in (dict(), dict(use_graph=False), dict(keep_traj=False)):           # captured + streamed, eager, captured
        want = trun(m, b, 4, seed=31, **kw)
        got = trun(m, b, 4, seed=31, time_levels=range(T - 1, -1, -1), **kw)
        assert got["t_traj"].tolist() == [T - 1, T - 2, T - 3, T - 4] and got["t_traj"].dtype == torch.int64 and "t_traj" not in want
        assert_same(without_t(got), want, f"{mean} full list {kw}")
        # S = 10: dd_sampler.T = 10, the tables are the native tables' first ten entries, the Philox words coincide
        want = trun(m, b, 10, seed=32, start_step=T - 10, **kw)
        got = trun(m, b, None, seed=32, time_levels=LAST10, **kw)               # (num_steps defaults to S)
        assert got["t_traj"].tolist() == LAST10
        assert_same(without_t(got), want, f"{mean} last ten levels {kw}")
    assert not torch.equal(trun(m, b, 4, seed=31, time_levels=LEVELS)["pos"], trun(m, b, 4, seed=31)["pos"])


def _compositions():
    b = pair(511)
    n, nb = 16, 112
    g = torch.Generator().manual_seed(512)
    known_lig = dict(pos=b["prior_centers"][b["ligand_decomp_batch"]] + 0.5 * torch.randn(n, 3, generator=g),
                     v=torch.randint(0, 8, (n,), generator=g), bond=torch.randint(0, 5, (nb,), generator=g))
    drawn = dict(b, init_ligand_pos=None, init_ligand_v=None, init_ligand_fc_bond_type=None)
    return {
        "hold": (b, dict(seed=41, fixed=known(b, scaffold(b), 513, "hold", init="given"))),
        "replace": (b, dict(seed=42, fixed=known(b, scaffold(b), 514, "replace", init="given"))),
        "replace+resample": (b, dict(seed=43, fixed=known(b, scaffold(b), 515, "replace", init="given"),
                                     resample=dict(jump_length=2, n_resample=2))),
        "hold+resample": (b, dict(seed=44, fixed=known(b, scaffold(b), 516, "hold"), resample=dict(jump_length=2, n_resample=2))),
        "noised init": (drawn, dict(seed=45, init=dict(mode="noised", **known_lig))),
        "scaled drift": (b, dict(seed=46, energy_drift_opt=[dict(type="armsca_prox", min_d=1.2, max_d=1.9, scale=True),
                                                            dict(type="clash", sigma=2.0, gamma=4.0, scale=True)])),
        "restraint window": (b, dict(seed=47, energy_drift_opt=[restraint(b, t_min=3, t_max=6, scale=True, traj=True)])),
    }


@pytest.mark.parametrize("name", ["hold", "replace", "replace+resample", "hold+resample", "noised init", "scaled drift", "restraint window"])
def test_last_ten_levels_equal_the_plain_chain_under_every_composition(name):
    """Every table is respaced consistently: dd_fixed.tab (replace, noised init), the jump table, tab_score (scale=True) and the
    restraint window's host map, each against the plain chain over the same ten levels."""
    m = model(0)
    b, kw = _compositions()[name]
    T = m.num_timesteps
    want = trun(m, b, 10, start_step=T - 10, **kw)
    got = trun(m, b, 10, time_levels=LAST10, **kw)
    if "resample" in kw:                                    # virtual level = real level: the very times of the plain schedule
        assert got["t_traj"].tolist() == times(9, 10) and len(times(9, 10)) == 20
        assert_same(got, want, name)
    else:
        assert_same(without_t(got), want, name)
    if name == "restraint window":
        free = trun(m, b, 10, start_step=T - 10, seed=kw["seed"])
        assert got["restraint_dist_traj"].shape == (10, 2) and not torch.equal(got["pos"], free["pos"])     # the window did open
        assert torch.equal(got["pos_traj"][:3], free["pos_traj"][:3])                                       # ... at t = 6, not before


def test_last_ten_levels_padded_ragged_batch_with_sample_keys(monkeypatch):
    monkeypatch.setenv("DD_RAGGED_MODE", "padded")
    m = model(0)
    n_l, singles, b, fx = ragged_case("replace")
    fx = dict(fx, init="given")
    T = m.num_timesteps
    want = trun(m, b, 10, start_step=T - 10, sample_keys=KEYS[:3], fixed=fx)
    assert_same(without_t(trun(m, b, 10, time_levels=LAST10, sample_keys=KEYS[:3], fixed=fx)), want, "padded, keyed, replace")


# ------------------------------------------------------------------------------------------------ 2: a list with gaps, the oracle
def oracle_tables(cfg, asc):
    """The respaced tables in the oracle's layout, float64 from the oracle's own schedule functions (decompdiff.py:95-131 and
    transitions.py:98-120 applied to alphas_cumprod' = alphas_cumprod[asc], log_cumprod' = log_cumprod[asc])."""
    betas = OD.sigmoid_betas(cfg.beta_start, cfg.beta_end, cfg.num_diffusion_timesteps)
    ac = np.cumprod(1.0 - betas)[asc]
    prev = np.append(1.0, ac[:-1])
    alphas = ac / prev
    betas = 1.0 - alphas
    f = OD.f32
    pt = dict(betas=f(betas), alphas_cumprod=f(ac), alphas_cumprod_prev=f(prev),
              posterior_mean_c0_coef=f(betas * np.sqrt(prev) / (1.0 - ac)),
              posterior_mean_ct_coef=f((1.0 - prev) * np.sqrt(alphas) / (1.0 - ac)),
              posterior_var=f(betas * (1.0 - prev) / (1.0 - ac)), pos_score_coef=f(betas / np.sqrt(alphas)))
    pv = pt["posterior_var"].numpy()
    pt["posterior_logvar"] = f(np.log(np.append(pv[1], pv[1:])))
    lca = np.cumsum(np.log(OD.cosine_alphas(cfg.num_diffusion_timesteps, cfg.v_beta_s)))[asc]
    la = np.append(lca[0], lca[1:] - lca[:-1])
    l1m = lambda a: np.log(1 - np.exp(a) + 1e-40)

    def cat(cfg_, num_classes, prior_probs=None):
        assert prior_probs is None
        return dict(log_alphas_v=f(la), log_one_minus_alphas_v=f(l1m(la)), log_alphas_cumprod_v=f(lca),
                    log_one_minus_alphas_cumprod_v=f(l1m(lca)), prior_probs=f(-np.log(num_classes).repeat(num_classes)[None, :]))
    return pt, cat


def score_gap(log_prob, u):
    """The smallest gap between the two best Gumbel scores of a row (float64), over every position."""
    score = -torch.log(-torch.log(u.double() + 1e-30) + 1e-30) + log_prob.double()
    top = score.topk(2, dim=-1).values
    return float((top[..., 0] - top[..., 1]).min())


@pytest.mark.parametrize("drift", [None, [dict(type="armsca_prox", min_d=1.2, max_d=1.9, scale=True)]], ids=["plain", "scaled armsca"])
def test_strided_chain_follows_the_oracle_on_respaced_tables(drift, monkeypatch):
    """Six positions at levels 999, 600, 250, 40, 3, 0 with injected noise, free-running: the oracle's loop is the reference's
    loop of a model with six timesteps whose tables are the respaced ones.  Types exact at every position, coordinates within the
    project's tolerance; the oracle's two best Gumbel scores are more than 1e-4 apart in every row at every position (asserted)."""
    m, b = model(0), pair(521)
    cfg, sd = GU.weights(0)
    torch.manual_seed(522)
    noise = synth.draw_step_noise(6, 16, 112)
    pt, cat = oracle_tables(cfg, LEVELS[::-1])
    monkeypatch.setattr(OD, "position_tables", lambda cfg_: pt)
    monkeypatch.setattr(OD, "categorical_tables", cat)
    want = OD.sample_diffusion(sd, cfg, num_steps=6, t_start=5, noise=noise, energy_drift_opt=drift, **b)
    monkeypatch.undo()
    gap = min(score_gap(torch.stack(want["vt_traj"]), noise["u_v"]), score_gap(torch.stack(want["bt_traj"]), noise["u_b"]))
    got = trun(m, b, 6, noise=noise, time_levels=LEVELS, energy_drift_opt=drift)
    err = maxabs(got["pos_traj"], torch.stack(want["pos_traj"]))
    moved = maxabs(want["pos_traj"][0], want["pos_traj"][-1])
    print(f"\nSTRIDED {'drift' if drift else 'plain'}: 6 positions vs the oracle on respaced tables, max |dpos| {err:.3g} (tol {POS_TOL:g}), "
          f"smallest score gap {gap:.3g}, the chain moved {moved:.3g}")
    assert gap > 1e-4
    assert got["t_traj"].tolist() == LEVELS
    assert torch.equal(got["v_traj"], torch.stack(want["v_traj"])) and torch.equal(got["bond_traj"], torch.stack(want["bond_traj"]))
    assert torch.equal(got["v"], want["v"]) and torch.equal(got["bond"], want["bond"])
    assert err < POS_TOL and maxabs(got["pos"], want["pos"]) < POS_TOL


# ------------------------------------------------------------------------------------------------ 3: replace mode across gaps
def test_replace_mode_noises_held_rows_to_the_real_level_of_the_next_position():
    """After the position at level L[p] the held rows are a forward-process sample at the REAL level L[p + 1], drawn with that
    position's device draws at Philox word tau = S - 1 - p; after the last position they are the clean values.  Bounds: those of
    test_replace_with_injected_noise_is_the_forward_process_of_the_clean_values (4 ulp(big); classes exact, gaps > 1e-3)."""
    m, b = model(0), pair(531)
    seed, S = 5353, len(LEVELS)
    mask = scaffold(b)
    mask[0] = True
    hb = held_bonds(b, mask)
    fx = known(b, mask, 532, "replace")
    r = trun(m, b, S, center_pos_mode="none", seed=seed, fixed=fx, time_levels=LEVELS)
    off = torch.zeros(2, 3)
    worst, gap = 0.0, 9.0
    for p in range(S - 1):
        d = philox_draws(seed, [S - 1 - p], 16, 112)
        lv = forward_level(m, b, fx, LEVELS[p + 1], d["u_v"][0], d["u_b"][0], d["eps"][0], off)
        gap = min(gap, float(lv["gap_v"][mask].min()), float(lv["gap_b"][hb].min()))
        assert torch.equal(r["v_traj"][p][mask], lv["v"][mask]) and torch.equal(r["bond_traj"][p][hb], lv["bond"][hb]), p
        err, bound = float((r["pos_traj"][p].double() - lv["xc"])[mask].abs().max()), 4 * ulp(lv["big"])
        worst = max(worst, err / bound)
        assert err <= bound, (p, err, bound)
    print(f"\nSTRIDED replace: held coordinates vs float64 at the real levels, worst error / bound {worst:.3f}; smallest score gap {gap:.3g}")
    assert gap > 1e-3
    assert torch.equal(r["v"][mask], fx["v"][mask]) and torch.equal(r["bond"][hb], fx["bond"][hb])
    assert torch.equal(r["pos"][mask], fx["pos"][mask]) and torch.equal(r["pos_traj"][-1][mask], fx["pos"][mask])


# ------------------------------------------------------------------------------------------------ 4: split and re-batched chains
def test_split_strided_chain_is_the_unsplit_one():
    m, b = model(0), pair(541)
    full = trun(m, b, None, center_pos_mode="none", seed=9, time_levels=LEVELS)
    first = trun(m, b, 3, center_pos_mode="none", seed=9, time_levels=LEVELS)
    b2 = dict(b, init_ligand_pos=first["pos"], init_ligand_v=first["v"], init_ligand_fc_bond_type=first["bond"])
    rest = trun(m, b2, 3, center_pos_mode="none", seed=9, time_levels=LEVELS, start_step=3)
    assert first["t_traj"].tolist() == LEVELS[:3] and rest["t_traj"].tolist() == LEVELS[3:]
    joined = {k: rest[k] for k in ("pos", "v", "bond")}
    joined.update({k: torch.cat([first[k], rest[k]]) for k in TRAJ + ("t_traj",)})
    assert_same(joined, full, "3 + 3 positions")


def test_strided_keyed_sample_alone_padded_and_grouped(monkeypatch):
    m = model(0)
    n_l, singles, b, _ = ragged_case("hold")
    keys = KEYS[:3]
    alone = [without_t(trun(m, s, None, seed=k, time_levels=LEVELS)) for s, k in zip(singles, keys)]
    for mode in ("padded", "groups"):
        monkeypatch.setenv("DD_RAGGED_MODE", mode)
        r = trun(m, b, None, sample_keys=keys, time_levels=LEVELS)
        assert r["t_traj"].tolist() == LEVELS
        for i, part in enumerate(split(without_t(r), n_l)):
            assert_same(part, alone[i], f"{mode}, sample {i}")


def test_harness_device_init_with_time_levels_does_not_depend_on_the_batch_size():
    m = model(0)
    runs = [harness.sample_diffusion_ligand_decomp(m, POCKETS[8], num_samples=2, batch_size=bs, device=dev(), init="device",
                                                   sample_key_seed=77, time_levels=LEVELS) for bs in (1, 2)]
    for key in ("pred_pos", "pred_v", "pred_bond_type", "pred_pos_traj", "pred_v_traj", "pred_b_traj", "pred_vt_traj"):
        for g in range(2):
            assert np.array_equal(np.asarray(runs[0][key][g]), np.asarray(runs[1][key][g])), (key, g)
    assert len(runs[0]["pred_pos_traj"][0]) == len(LEVELS)                      # num_steps=None: the whole list
    plain = harness.sample_diffusion_ligand_decomp(m, POCKETS[8], num_samples=2, batch_size=2, device=dev(), init="device",
                                                   sample_key_seed=77, num_steps=6)
    assert not np.array_equal(plain["pred_pos"][0], runs[0]["pred_pos"][0])


# ------------------------------------------------------------------------------------------------ 5: windows and t_traj
def test_restraint_windows_are_real_levels():
    """Positions 1 .. 5 of the list (levels 600 .. 0): the window [30, 700] holds the levels 600, 250, 40 -- as [40, 600] does --,
    [4, 39] holds none, and [999, 999] holds only a level the chain never visits: it never opens."""
    m, b = model(0), pair(551)
    call = lambda **win: trun(m, b, 5, seed=61, time_levels=LEVELS, start_step=1, energy_drift_opt=[restraint(b, traj=True, **win)])
    wide, tight, empty, never = call(t_min=30, t_max=700), call(t_min=40, t_max=600), call(t_min=4, t_max=39), call(t_min=999, t_max=999)
    assert wide["t_traj"].tolist() == LEVELS[1:]
    assert_same(wide, tight, "[30, 700] against [40, 600]")
    assert_same(empty, never, "[4, 39] against a window that never opens")
    assert not torch.equal(wide["pos"], never["pos"])
    assert empty["restraint_dist"].shape == (2,) and bool(torch.isfinite(empty["restraint_dist"]).all()) and bool((empty["restraint_atom"] >= 0).all())
    assert bool(torch.isfinite(empty["restraint_dist_traj"]).all())
    # a window that never opens adds exact zeros: the chain without the term; the open one parts from it while the window is open
    free = trun(m, b, 5, seed=61, time_levels=LEVELS, start_step=1)
    assert_same({k: never[k] for k in free}, free, "never open against no restraint")
    assert not torch.equal(wide["pos_traj"][:3], free["pos_traj"][:3])


def test_t_traj_with_resample_holds_the_real_levels_of_the_schedule():
    m, b = model(0), pair(561)
    fx = known(b, scaffold(b), 562, "hold")
    r = trun(m, b, None, seed=71, time_levels=LEVELS, fixed=fx, resample=dict(jump_length=2, n_resample=2))
    virtual = times(5, 6)
    assert len(virtual) == 12 and r["t_traj"].tolist() == [LEVELS[5 - t] for t in virtual] and r["pos_traj"].shape[0] == 12
    assert r["t_traj"].tolist()[:4] == [999, 600, 999, 600]


# ------------------------------------------------------------------------------------------------ 6: cache hygiene
def test_one_graph_per_schedule_and_no_stale_tables(monkeypatch):
    monkeypatch.setenv("DD_CHAIN_CACHE", "1")
    m, b = model(0), pair(571)
    m._evict_chain_cache(0)
    n0 = DecompScorePosNet3D._graph_counter
    calls = [dict(), dict(time_levels=LEVELS), dict(time_levels=LAST10), dict(), dict(time_levels=LEVELS)]
    runs = [without_t(trun(m, b, 4, seed=81, **kw)) for kw in calls]
    assert DecompScorePosNet3D._graph_counter == n0 + 3                         # one capture per schedule
    assert len(m._chain_cache) == 3
    assert_same(runs[3], runs[0], "plain again")
    assert_same(runs[4], runs[1], "levels A again")
    assert not torch.equal(runs[0]["pos"], runs[1]["pos"]) and not torch.equal(runs[1]["pos"], runs[2]["pos"])
    assert_same(runs[1], without_t(trun(m, b, 4, seed=81, time_levels=LEVELS, use_graph=False)), "levels A, eager")
    m._evict_chain_cache(0)
