"""Host side of strided sampling (``sample_diffusion(time_levels=...)``): the respaced schedule tables
(`schedules.position_tables` / `categorical_tables` with ``levels=``), the validation of the list, the two host mappings of real
time (restraint windows, ``t_traj``) and `stride_levels`.  No GPU.

The subset's reference is a float64 restatement written here from `get_beta_schedule` / `cosine_beta_schedule`; the identities
are those of a Gaussian / categorical chain whose marginals at the kept levels are the full chain's (s < t two neighbours of the
list): c0' + ct' sqrt(acp_t / acp_s) sqrt(acp_s) = sqrt(acp_s) etc., exact in real arithmetic, 1e-12 in float64."""
import numpy as np
import pytest
import torch

from decompdiff_amd import DecompScorePosNet3D, schedules, shipped_config, stride_levels
from decompdiff_amd.model import _Call, _as_time_levels, _virtual_window

CFG = shipped_config()
T = CFG.num_diffusion_timesteps
SUBSET = [0, 3, 40, 250, 600, 999]
PRIORS = {8: [0.3, 0.2, 0.1, 0.1, 0.1, 0.1, 0.05, 0.05], 5: [0.6, 0.2, 0.1, 0.05, 0.05]}


def cat_tables(nc, prior, levels=None):
    return schedules.categorical_tables(CFG.v_beta_schedule, T, CFG.v_beta_s, nc, PRIORS[nc] if prior else None, levels=levels)


# ------------------------------------------------------------------------------------------------ the full list
def test_full_list_reproduces_the_native_position_tables():
    native = schedules.position_tables(CFG)
    for levels in (list(range(T)), np.arange(T), torch.arange(T).numpy()):
        full = schedules.position_tables(CFG, levels)
        assert set(full) == set(native)
        for k in native:
            assert torch.equal(full[k], native[k]), k


@pytest.mark.parametrize("prior", [False, True], ids=["uniform", "prior_probs"])
@pytest.mark.parametrize("nc", [8, 5])
def test_full_list_reproduces_the_native_categorical_tables(nc, prior):
    native, full = cat_tables(nc, prior), cat_tables(nc, prior, list(range(T)))
    assert set(full) == set(native)
    for k in native:
        assert torch.equal(full[k], native[k]), k


def test_levels_none_is_todays_call():
    a, b = schedules.position_tables(CFG), schedules.position_tables(CFG, levels=None)
    assert all(torch.equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------------ a subset, against float64
def acp64():
    betas = schedules.get_beta_schedule(beta_schedule=CFG.beta_schedule, beta_start=CFG.beta_start, beta_end=CFG.beta_end,
                                        num_diffusion_timesteps=T)
    return np.cumprod(1.0 - betas)


def test_subset_position_tables_against_a_float64_restatement():
    assert CFG.beta_schedule != "cosine"
    a = acp64()[SUBSET]                                   # acp' of virtual level tau
    prev = np.append(1.0, a[:-1])
    alpha = a / prev
    beta = 1.0 - alpha
    c0, ct, var = beta * np.sqrt(prev) / (1.0 - a), (1.0 - prev) * np.sqrt(alpha) / (1.0 - a), beta * (1.0 - prev) / (1.0 - a)
    # marginal consistency, float64: x_s = c0 x_0 + ct x_t + sqrt(var) e reproduces q(x_s | x_0) when x_t ~ q(x_t | x_0)
    assert np.abs(c0 + ct * np.sqrt(a) - np.sqrt(prev)).max() < 1e-12
    assert np.abs(ct ** 2 * (1.0 - a) + var - (1.0 - prev)).max() < 1e-12
    got = schedules.position_tables(CFG, SUBSET)
    f32 = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float64)).float()
    want = {"betas": beta, "alphas_cumprod": a, "alphas_cumprod_prev": prev, "sqrt_alphas_cumprod": np.sqrt(a),
            "sqrt_one_minus_alphas_cumprod": np.sqrt(1.0 - a), "sqrt_recip_alphas_cumprod": np.sqrt(1.0 / a),
            "sqrt_recipm1_alphas_cumprod": np.sqrt(1.0 / a - 1.0), "posterior_mean_c0_coef": c0, "posterior_mean_ct_coef": ct,
            "posterior_var": var, "pos_score_coef": beta / np.sqrt(alpha)}
    assert set(got) == set(want) | {"posterior_logvar"}
    for k, w in want.items():
        assert got[k].shape == (len(SUBSET),) and torch.equal(got[k], f32(w)), k
    # the quirk of the full schedule: the log of the fp32 variance, entry 0 := entry 1
    pv = f32(var).numpy()
    assert torch.equal(got["posterior_logvar"], f32(np.log(np.append(pv[1], pv[1:]))))
    # the kept entries of the cumulative tables are the full schedule's own
    native = schedules.position_tables(CFG)
    for k in ("alphas_cumprod", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod",
              "sqrt_recipm1_alphas_cumprod"):
        assert torch.equal(got[k], native[k][SUBSET]), k
    # ... the one-step tables are NOT (a stride's beta is larger than the level's own)
    assert float(got["betas"][3]) > 10 * float(native["betas"][250])


@pytest.mark.parametrize("nc", [8, 5])
def test_subset_categorical_tables_against_a_float64_restatement(nc):
    log_cum = np.cumsum(np.log(schedules.cosine_beta_schedule(T, CFG.v_beta_s)))[SUBSET]
    log_alpha = np.append(log_cum[0], np.diff(log_cum))
    assert np.abs(log_alpha[1:] + log_cum[:-1] - log_cum[1:]).max() < 1e-12 and log_alpha[0] == log_cum[0]
    l1m = lambda x: np.log(1 - np.exp(x) + 1e-40)
    f32 = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float64)).float()
    got, native = cat_tables(nc, True, SUBSET), cat_tables(nc, True)
    for k, w in (("log_alphas_v", log_alpha), ("log_one_minus_alphas_v", l1m(log_alpha)), ("log_alphas_cumprod_v", log_cum),
                 ("log_one_minus_alphas_cumprod_v", l1m(log_cum))):
        assert torch.equal(got[k], f32(w)), k
    assert torch.equal(got["prior_probs"], native["prior_probs"])
    assert torch.equal(got["log_alphas_cumprod_v"], native["log_alphas_cumprod_v"][SUBSET])


@pytest.mark.parametrize("bad", [[3], [], [3, 3], [5, 3], [-1, 3], [3, T], [0.0, 3.0], [[0, 3]]])
def test_schedule_builders_refuse_bad_levels(bad):
    with pytest.raises(ValueError):
        schedules.position_tables(CFG, bad)
    with pytest.raises(ValueError):
        cat_tables(8, False, bad)


# ------------------------------------------------------------------------------------------------ the model's table builders
def test_model_builders_compose_from_the_table_dict():
    m = DecompScorePosNet3D(CFG, 29, 10, 8, prior_atom_types=PRIORS[8], prior_bond_types=PRIORS[5])
    # default, the module's own dict and the full list: the same bits
    full = m.schedule_tables(list(range(T)))
    for tables in (m.schedule_tables(), full):
        for mode in ("C0", "noise"):
            assert torch.equal(m.position_step_table(mode, tables), m.position_step_table(mode))
        assert torch.equal(m.fixed_step_table(tables), m.fixed_step_table())
        assert torch.equal(m.resample_jump_table(3, tables), m.resample_jump_table(3))
    assert torch.equal(full["atom_type_trans"]["prior_probs"], m.atom_type_trans.prior_probs.detach())
    # the last ten levels' tables ARE the native tables' first ten entries
    ten = m.schedule_tables(list(range(10)))
    for mode in ("C0", "noise"):
        assert torch.equal(m.position_step_table(mode, ten), m.position_step_table(mode)[:, :10])
    assert torch.equal(m.fixed_step_table(ten), m.fixed_step_table()[:, :10])
    assert torch.equal(m.resample_jump_table(2, ten), m.resample_jump_table(2)[:, :10])
    # a subset: [.][S] tables; the fixed table's entries are the kept levels', the jump over one position spans the real gap
    sub = m.schedule_tables(SUBSET)
    assert m.position_step_table("C0", sub).shape == (3, 6) and m.resample_jump_table(1, sub).shape == (6, 6)
    assert torch.equal(m.fixed_step_table(sub), m.fixed_step_table()[:, SUBSET])
    a = acp64()
    assert abs(float(m.resample_jump_table(1, sub)[0, 4]) - np.sqrt(a[600] / a[250])) < 1e-6


# ------------------------------------------------------------------------------------------------ validation of time_levels
@pytest.mark.parametrize("bad", [
    [True, False], [999.0, 0.0], [5, 5, 0], [0, 5], [9, 5, 7], [T, 5], [5, -1], [5], [], 7, "90", [[5, 0]],
    np.array([5.0, 0.0]), np.array([[5, 0]]), torch.tensor([5.0, 0.0]), torch.tensor([True, False]), torch.tensor([[5, 0]]),
    torch.tensor([0, 5]), np.array([5, 5])])
def test_time_levels_validation_errors(bad):
    with pytest.raises(ValueError):
        _as_time_levels(bad, T)


@pytest.mark.parametrize("form", [list, tuple, np.array, torch.tensor, lambda v: np.array(v, dtype=np.int32), lambda v: range(9, -1, -1)])
def test_time_levels_forms(form):
    lv = _as_time_levels(form(list(range(9, -1, -1))), T)
    assert lv.dtype == torch.int64 and lv.tolist() == list(range(10))      # the real level of every virtual level


def test_positions_beyond_the_list_raise():
    for steps, start in ((7, 0), (6, 1), (1, 6), (1, -1)):
        with pytest.raises(ValueError):
            _Call(6, steps, start)
    m = DecompScorePosNet3D(CFG, 29, 10, 8)
    z = torch.zeros(0)
    with pytest.raises(ValueError):                        # (before any tensor is looked at)
        m.sample_diffusion(z, z, z, None, z, z, z, z, None, None, z, None, None, None, z, z, num_steps=4, start_step=3,
                           time_levels=SUBSET[::-1])
    with pytest.raises(ValueError):
        m.sample_diffusion(z, z, z, None, z, z, z, z, None, None, z, None, None, None, z, z, time_levels=SUBSET)


# ------------------------------------------------------------------------------------------------ host mappings
def test_restraint_window_mapping():
    lv = torch.tensor(SUBSET)
    assert _virtual_window(lv, 0, T - 1) == (0, 5)
    assert _virtual_window(lv, 30, 700) == (2, 4) == _virtual_window(lv, 40, 600)
    assert _virtual_window(lv, 4, 39) is None and _virtual_window(lv, 601, 998) is None and _virtual_window(lv, 1, 2) is None
    assert _virtual_window(lv, 0, 0) == (0, 0) and _virtual_window(lv, 0, 2) == (0, 0)          # the low end
    assert _virtual_window(lv, 999, 999) == (5, 5) and _virtual_window(lv, 601, 999) == (5, 5)  # the high end
    assert _virtual_window(lv, 3, 3) == (1, 1) and _virtual_window(lv, 3, 40) == (1, 2)
    assert _virtual_window(torch.tensor([2, 5]), 0, 1) is None and _virtual_window(torch.tensor([2, 5]), 6, 9) is None
    full = torch.arange(T)
    assert _virtual_window(full, 17, 230) == (17, 230)


def test_t_traj_mapping():
    lv = torch.tensor(SUBSET)
    exec_order = SUBSET[::-1]
    assert _Call(6, 6, levels=lv).t_traj.tolist() == exec_order
    assert _Call(6, 3, start_step=2, levels=lv).t_traj.tolist() == exec_order[2:5]
    t = _Call(6, 2, start_step=4, levels=lv).t_traj
    assert t.tolist() == [3, 0] and t.dtype == torch.int64
    # resampled: the virtual times of the schedule's positions, mapped
    rs = dict(t_traj=torch.tensor([4, 3, 4, 3, 2]), n_total=5)
    assert _Call(6, 3, start_step=1, resample=rs, levels=lv).t_traj.tolist() == [600, 250, 600, 250, 40]
    # unstrided: as before -- nothing without resample, the schedule's own times with it
    assert _Call(1000, 4).t_traj is None
    assert _Call(1000, 3, resample=rs).t_traj.tolist() == [4, 3, 4, 3, 2]


# ------------------------------------------------------------------------------------------------ stride_levels
def test_stride_levels():
    assert stride_levels(T, T) == list(range(T - 1, -1, -1))
    for n in (2, 10, 100):
        lv = stride_levels(T, n)
        assert len(lv) == n and lv[0] == T - 1 and lv[-1] == 0 and all(isinstance(v, int) for v in lv)
        assert all(a > b for a, b in zip(lv, lv[1:])) and len(set(lv)) == n
        gaps = {a - b for a, b in zip(lv, lv[1:])}
        assert max(gaps) - min(gaps) <= 1                  # evenly spaced
        _as_time_levels(lv, T)
    assert stride_levels(T, 2) == [T - 1, 0] and stride_levels(7, 4) == [6, 4, 2, 0]
    for bad in (1, 0, T + 1):
        with pytest.raises(ValueError):
            stride_levels(T, bad)
