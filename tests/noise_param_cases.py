"""GPU cases of model_mean_type = 'noise' end to end: sampling (dense, padded ragged, graph replay, start_step resumption, drift
with and without `scale`) and the training objective (eager, torch.no_grad validation, GraphedTrainStep) against fixtures from the
reference itself (tools/make_noise_golden.py).  Run by tests/test_gpu_noise_param.py in a process of their own (see there);
`pytest -m gpu tests/noise_param_cases.py` runs them directly."""
import json

import numpy as np
import pytest
import torch

import golden_utils as GU
from decompdiff_amd import DecompScorePosNet3D, shipped_config, synth, training
from test_gpu_configs import _check_chain, _fixture_chain, _hetero_batch
from test_gpu_parity import LOGIT_TOL, POS_TOL, _sample_hip, dev, maxabs
from test_gpu_parity import model as c0_model
from test_gpu_training import _grads_agree, _loss_kwargs

pytestmark = pytest.mark.gpu

_MODELS = {}
B8_STD = [1.0, 0.9, 0.8, 1.1, 1.0, 0.95, 1.05, 0.85]


def _new_model(mode):
    cfg = shipped_config(model_mean_type=mode)
    m = DecompScorePosNet3D(cfg, 29, 10, 8)
    sd = m.state_dict()
    sd.update(synth.synthetic_state_dict(cfg, 0))
    m.load_state_dict(sd, strict=True)
    return m.to(dev())


def noise_model():
    if "noise" not in _MODELS:
        _MODELS["noise"] = _new_model("noise")
    return _MODELS["noise"]


def _step_case(g, t_start, tag):
    """(batch, drift, noise) of one case of steps_noise.npz, re-drawn as the generator drew it."""
    p = f"t{t_start}_{tag}_"
    drift = GU.DRIFT if tag == "drift" else None
    b = GU.batch_from_npz(g)
    for k in ("init_ligand_pos", "init_ligand_v", "init_ligand_fc_bond_type", "prior_stds"):
        b[k] = torch.from_numpy(g[p + "in_" + k])
    torch.manual_seed(int(g[p + "seed"]))
    synth.build_sampling_batch(synth.make_pocket_small(1), 2, per_sample_std_scale=[1.0, 0.8] if drift else None)
    noise = synth.draw_step_noise(1, b["init_ligand_pos"].size(0), b["init_ligand_fc_bond_type"].size(0))
    assert GU.same_checksum(GU.checksum(noise), g[p + "noise_checksum"])
    return b, drift, noise


def _check_step(m, g, t_start, tag, label="noise"):
    p = f"t{t_start}_{tag}_"
    b, drift, noise = _step_case(g, t_start, tag)
    r = _sample_hip(m, b, 1, drift, noise, t_start)
    e_pos = maxabs(r["pos"], g[p + "pos"])
    e_lp = max(maxabs(r["vt_traj"][0], g[p + "log_v_prob"]), maxabs(r["bt_traj"][0], g[p + "log_b_prob"]),
               maxabs(r["v0_traj"][0], g[p + "log_v_recon"]))
    nv = int((r["v"].cpu() != torch.from_numpy(g[p + "v"])).sum())
    nb = int((r["bond"].cpu() != torch.from_numpy(g[p + "bond"])).sum())
    print(f"{label} step t={t_start} {tag}: pos {e_pos:.3g} log-probs {e_lp:.3g} v-mismatch {nv} bond-mismatch {nb}")
    assert e_pos < POS_TOL and e_lp < LOGIT_TOL
    assert nv == 0 and nb == 0
    return r


# ------------------------------------------------------------------------------------ sampling
@pytest.mark.parametrize("t_start", [999, 500, 1, 0])
@pytest.mark.parametrize("tag", ["plain", "drift"])
def test_single_steps_noise_reference_golden(t_start, tag):
    _check_step(noise_model(), GU.load("steps_noise"), t_start, tag)


@pytest.mark.parametrize("name,std_scale", [("traj3_noise_b8_plain", None), ("traj3_noise_b8_drift", B8_STD)])
def test_sampling_b8_noise_reference_golden(name, std_scale):
    g, b, noise = _fixture_chain(name, synth.make_pocket_small(8), 8, std_scale)
    assert b["init_ligand_pos"].shape[0] == 8 * 30 and b["protein_pos"].shape[0] == 8 * 300
    r = _sample_hip(noise_model(), b, 3, json.loads(str(g["drift"])), noise)
    _check_chain(f"noise ({name}: NP=300, NL=30, B=8)", r, g, 3)


def test_sampling_20_steps_noise_reference_golden():
    g, b, noise = _fixture_chain("traj20_noise", synth.make_pocket_small(2), 2, [1.0, 0.85])
    r = _sample_hip(noise_model(), b, 20, json.loads(str(g["drift"])), noise)
    _check_chain("noise (traj20_noise: 20 steps, B=2, drift)", r, g, 20)


def test_resume_from_the_reference_checkpoint_with_start_step():
    """The last 12 steps of traj20_noise restarted with start_step = 8 from the reference's own state after 8 steps."""
    g, b, noise = _fixture_chain("traj20_noise", synth.make_pocket_small(2), 2, [1.0, 0.85])
    bb = dict(b)
    bb["init_ligand_pos"] = torch.from_numpy(g["traj_pos"][7].astype(np.float32))
    bb["init_ligand_v"] = torch.from_numpy(g["traj_v"][7].astype(np.int64))
    bb["init_ligand_fc_bond_type"] = torch.from_numpy(g["traj_bond"][7].astype(np.int64))
    r = _sample_hip(noise_model(), bb, 12, json.loads(str(g["drift"])), {k: v[8:] for k, v in noise.items()}, start_step=8)
    err = maxabs(r["pos"], g["out_pos"])
    print(f"noise: steps 8..19 resumed from the reference's step-8 state: final pos err {err:.3g}")
    assert err < POS_TOL
    assert np.array_equal(r["v"].cpu().numpy(), g["out_v"]) and np.array_equal(r["bond"].cpu().numpy(), g["out_bond"])


@pytest.mark.parametrize("drift", [False, True])
def test_resumed_noise_chain_is_the_unsplit_chain(drift):
    """Philox noise, frame fixed (center_pos_mode='none'): 16 steps in one call == 6 steps, then 10 with start_step = 6, bit for bit."""
    torch.manual_seed(5)
    b = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in synth.build_sampling_batch(synth.make_pocket_small(3), 4).items()}
    m = noise_model()
    kw = dict(center_pos_mode="none", energy_drift_opt=GU.DRIFT if drift else None, seed=77)
    full = m.sample_diffusion(num_steps=16, **b, **kw)
    first = m.sample_diffusion(num_steps=6, **b, **kw)
    b2 = dict(b)
    b2["init_ligand_pos"], b2["init_ligand_v"], b2["init_ligand_fc_bond_type"] = first["pos"], first["v"], first["bond"]
    rest = m.sample_diffusion(num_steps=10, start_step=6, **b2, **kw)
    for k in ("pos", "v", "bond"):
        assert torch.equal(rest[k], full[k]), k
    assert all(torch.equal(x, y) for x, y in zip(list(first["pos_traj"]) + list(rest["pos_traj"]), full["pos_traj"]))
    assert bool(torch.isfinite(full["pos"]).all())


def test_noise_graph_replay_equals_eager_launches():
    g, b, noise = _fixture_chain("traj20_noise", synth.make_pocket_small(2), 2, [1.0, 0.85])
    n5 = {k: v[:5] for k, v in noise.items()}
    drift = json.loads(str(g["drift"]))
    r1 = _sample_hip(noise_model(), b, 5, drift, n5, use_graph=True)
    r2 = _sample_hip(noise_model(), b, 5, drift, n5, use_graph=False)
    for k in ("pos", "v", "bond"):
        assert torch.equal(r1[k], r2[k]), k
    assert torch.equal(torch.stack(r1["pos_traj"]), torch.stack(r2["pos_traj"]))
    assert torch.equal(torch.stack(r1["bt_traj"]), torch.stack(r2["bt_traj"]))
    assert maxabs(torch.stack(r1["pos_traj"]), g["traj_pos"][:5]) < POS_TOL


def test_noise_padded_heterogeneous_batch_equals_size_groups(monkeypatch):
    """One padded launch sequence (the default) against one dense group per size (DD_RAGGED_MODE=groups, several chains replayed
    together) in noise mode, armsca + clash drift, injected noise."""
    sizes, n_prot = [9, 37, 20, 33, 17, 25], [150, 260, 120, 200, 180, 131]
    b = _hetero_batch(sizes, n_prot, seed=4)
    steps = 4
    noise = synth.draw_step_noise(steps, b["init_ligand_pos"].size(0), b["init_ligand_fc_bond_type"].size(0))
    outs = {}
    for mode in ("padded", "groups"):
        monkeypatch.setenv("DD_RAGGED_MODE", mode)
        outs[mode] = _sample_hip(noise_model(), b, steps, GU.DRIFT, noise)
    p, q = outs["padded"], outs["groups"]
    err = maxabs(p["pos"], q["pos"])
    e_bt = maxabs(torch.stack(p["bt_traj"]), torch.stack(q["bt_traj"]))
    print(f"noise padded vs groups: pos diff {err:.3g}, bond log-prob diff {e_bt:.3g}")
    assert p["pos"].shape == (sum(sizes), 3)
    assert err < 5e-6 and e_bt < 5e-5
    # (the mode reaches the ragged path: the C0 model moves the same batch elsewhere)
    c0 = _sample_hip(c0_model(0), b, steps, GU.DRIFT, noise)
    assert maxabs(c0["pos"], p["pos"]) > 10 * POS_TOL
    assert torch.equal(p["v"], q["v"]) and torch.equal(p["bond"], q["bond"])


def test_scale_drift_in_noise_mode():
    """`scale: True` multiplies the drift gradient by pos_score_coef[t] after the folded mean (decompdiff.py:656-668): one step at
    t = 500 on the same injected noise with drift off / on / scaled -- (scaled - off) == coef * (on - off)."""
    g = GU.load("steps_noise")
    b, drift, noise = _step_case(g, 500, "drift")
    m = noise_model()
    scaled = [dict(d, scale=True) for d in drift]
    off, on, sc = (_sample_hip(m, b, 1, d, noise, 500)["pos"].double() for d in (None, drift, scaled))
    coef = float(m.pos_score_coef[500])
    assert float((on - off).abs().max()) > 1e-4                   # the drift acts
    err = float(((sc - off) - coef * (on - off)).abs().max())
    print(f"noise scale drift at t=500: coef {coef:.3g}, |scaled - coef * unscaled| {err:.3g}")
    assert err < 1e-5


def test_changing_the_mode_repacks_the_tables():
    """A C0 model switched to 'noise' after construction samples the noise fixture (the packed tables follow the mode), and
    switched back reproduces its C0 step bit for bit."""
    m = _new_model("C0")
    g = GU.load("steps_noise")
    b, drift, noise = _step_case(g, 999, "plain")
    c0 = _sample_hip(m, b, 1, drift, noise, 999)
    assert maxabs(c0["pos"], g["t999_plain_pos"]) > 10 * POS_TOL        # C0 is not the noise fixture
    m.model_mean_type = "noise"
    _check_step(m, g, 999, "plain", label="C0 model switched to noise")
    m.model_mean_type = "C0"
    again = _sample_hip(m, b, 1, drift, noise, 999)
    assert torch.equal(again["pos"], c0["pos"])


# ------------------------------------------------------------------------------------ training
def _check_losses(label, losses, g, rel=None):
    """The bounds of tests/test_gpu_training.py: 1e-4 (absolute below 1, relative above) and, for the eager route, 2e-3 relative."""
    for k in ("pos", "v", "bond"):
        got, want = float(losses[k]), float(g["loss_" + k])
        print(f"{label} loss {k}: {got:.7g} (reference {want:.7g})")
        assert abs(got - want) <= 1e-4 * max(1.0, abs(want)), k
        assert rel is None or abs(got - want) <= rel * abs(want) + 1e-7, k


@pytest.mark.parametrize("fixture", ["loss_grad_noise", "loss_grad_noise_ragged"])
def test_noise_loss_and_gradients_match_reference(fixture):
    g = GU.load(fixture)
    m = _new_model("noise").train()
    kw = _loss_kwargs(g)
    torch.manual_seed(int(g["noise_seed"]))
    res = m.get_diffusion_loss(**kw)
    _check_losses(f"eager {fixture}", res["losses"], g, rel=2e-3)
    assert maxabs(res["pred_ligand_pos"], g["out_pred_ligand_pos"]) < 1e-4
    assert maxabs(res["pred_ligand_v"], g["out_pred_ligand_v"]) < 1e-4
    assert maxabs(res["x0"], g["out_x0"]) < 1e-5
    loss = res["losses"]["pos"] + 100.0 * res["losses"]["v"] + 100.0 * res["losses"]["bond"]
    loss.backward()
    params = dict(m.named_parameters())
    worst = 0.0
    for key in [k for k in g.files if k.startswith("grad__")]:
        name = key[len("grad__"):].replace("__", ".")
        want = torch.from_numpy(g[key])
        rel = float((params[name].grad.cpu() - want).abs().max() / want.abs().max().clamp(min=1e-12))
        worst = max(worst, rel)
        assert rel < 2e-3, (name, rel)
    names = [str(n) for n in g["grad_norm_names"]]
    got_norms = np.array([float(params[n].grad.double().norm()) if params[n].grad is not None else 0.0 for n in names])
    rel_n = np.abs(got_norms - g["grad_norms"]) / np.maximum(g["grad_norms"], 1e-6 * g["grad_norms"].max())
    print(f"noise {fixture}: {len(names)} parameter gradients, worst relative tensor error {worst:.2g}, norm error {rel_n.max():.2g}")
    assert rel_n.max() < 2e-3
    assert all(params[n].grad is not None for n in names)


@pytest.mark.parametrize("fixture", ["loss_grad_noise", "loss_grad_noise_ragged"])
def test_noise_validation_loss_uses_the_fused_forward_and_agrees(fixture):
    g = GU.load(fixture)
    m = _new_model("noise")
    kw = _loss_kwargs(g)
    with torch.no_grad():
        torch.manual_seed(int(g["noise_seed"]))
        v = m.get_diffusion_loss(**kw)
    assert not v["losses"]["pos"].requires_grad
    _check_losses(f"no_grad {fixture}", v["losses"], g)
    assert maxabs(v["pred_ligand_pos"], g["out_pred_ligand_pos"]) < 1e-4


@pytest.mark.parametrize("fixture", ["loss_grad_noise", "loss_grad_noise_ragged"])
def test_noise_graphed_train_step_matches_reference(fixture):
    """GraphedTrainStep (dense: `objective`; mixed sizes: the padded layout, `objective_padded`) with lr = 0, so every iteration sees
    the fixture's weights: two eager iterations, then the captured one -- losses and gradients of the replay against the reference."""
    g = GU.load(fixture)
    m = _new_model("noise").train()
    opt = torch.optim.Adam(m.parameters(), lr=0.0, capturable=True)
    gs = training.GraphedTrainStep(m, opt, loss_weights=(1.0, 100.0, 100.0), warmup=2)
    kw = _loss_kwargs(g)
    for _ in range(3):
        torch.manual_seed(int(g["noise_seed"]))
        out = gs.step(**kw)
        _check_losses(f"graphed {fixture}", out["losses"], g)
    assert gs.replays == 1 and gs.eager_steps == 2
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    _grads_agree(grads, grads, g)
