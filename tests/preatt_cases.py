"""GPU cases of the distance-aware bond head (bond_net_type = 'pre_att') end to end: forward, sampling (dense, padded ragged and
grouped ragged, graph replay, start_step resumption, drift) and the training objective (eager, torch.no_grad validation,
GraphedTrainStep) against fixtures from the reference itself (tools/make_preatt_golden.py).  Run by tests/test_gpu_bond_head.py in
a process of their own (see there); `pytest -m gpu tests/preatt_cases.py` runs them directly."""
import json

import numpy as np
import pytest
import torch

import golden_utils as GU
from decompdiff_amd import DecompScorePosNet3D, harness, shipped_config, synth, training
from noise_param_cases import _check_losses, _step_case
from test_gpu_configs import _check_chain, _fixture_chain, _hetero_batch
from test_gpu_parity import LOGIT_TOL, POS_TOL, _forward_hip, _sample_hip, dev, maxabs
from test_gpu_parity import model as lin_model
from test_gpu_training import _grads_agree, _loss_kwargs

pytestmark = pytest.mark.gpu

_MODELS = {}
B8_STD = [1.0, 0.9, 0.8, 1.1, 1.0, 0.95, 1.05, 0.85]


def _new_model():
    cfg = shipped_config(bond_net_type="pre_att")
    m = DecompScorePosNet3D(cfg, 29, 10, 8)
    sd = m.state_dict()
    sd.update(synth.synthetic_state_dict(cfg, 0))
    m.load_state_dict(sd, strict=True)
    return m.to(dev())


def preatt_model():
    if "pre_att" not in _MODELS:
        _MODELS["pre_att"] = _new_model()
    return _MODELS["pre_att"]


# ------------------------------------------------------------------------------------ forward
def test_forward_preatt_reference_golden():
    g = GU.load("forward_preatt")
    out = _forward_hip(preatt_model(), GU.batch_from_npz(g))
    torch.cuda.synchronize()
    errs = {k: maxabs(out[k], g["out_" + k]) for k in ("pred_ligand_pos", "pred_ligand_v", "pred_bond")}
    print("pre_att forward (NP=300, NL=30, B=2): " + ", ".join(f"{k} {v:.3g}" for k, v in errs.items()))
    assert errs["pred_ligand_pos"] < 2e-5 and errs["pred_ligand_v"] < 2e-4 and errs["pred_bond"] < 2e-4
    # the lin model reads other weights: the pre_att head really is what produced pred_bond
    lin = _forward_hip(lin_model(0), GU.batch_from_npz(g))
    assert maxabs(lin["pred_bond"], g["out_pred_bond"]) > 1e-2


# ------------------------------------------------------------------------------------ sampling
@pytest.mark.parametrize("t_start", [999, 500, 1, 0])
@pytest.mark.parametrize("tag", ["plain", "drift"])
def test_single_steps_preatt_reference_golden(t_start, tag):
    g = GU.load("steps_preatt")
    p = f"t{t_start}_{tag}_"
    b, drift, noise = _step_case(g, t_start, tag)
    r = _sample_hip(preatt_model(), b, 1, drift, noise, t_start)
    e_pos = maxabs(r["pos"], g[p + "pos"])
    e_lp = max(maxabs(r["vt_traj"][0], g[p + "log_v_prob"]), maxabs(r["bt_traj"][0], g[p + "log_b_prob"]),
               maxabs(r["v0_traj"][0], g[p + "log_v_recon"]))
    nv = int((r["v"].cpu() != torch.from_numpy(g[p + "v"])).sum())
    nb = int((r["bond"].cpu() != torch.from_numpy(g[p + "bond"])).sum())
    print(f"pre_att step t={t_start} {tag}: pos {e_pos:.3g} log-probs {e_lp:.3g} v-mismatch {nv} bond-mismatch {nb}")
    assert e_pos < POS_TOL and e_lp < LOGIT_TOL
    assert nv == 0 and nb == 0


@pytest.mark.parametrize("name,std_scale", [("traj3_preatt_b8_plain", None), ("traj3_preatt_b8_drift", B8_STD)])
def test_sampling_b8_preatt_reference_golden(name, std_scale):
    g, b, noise = _fixture_chain(name, synth.make_pocket_small(8), 8, std_scale)
    assert b["init_ligand_pos"].shape[0] == 8 * 30 and b["protein_pos"].shape[0] == 8 * 300
    r = _sample_hip(preatt_model(), b, 3, json.loads(str(g["drift"])), noise)
    _check_chain(f"pre_att ({name}: NP=300, NL=30, B=8)", r, g, 3)


def test_sampling_20_steps_preatt_reference_golden():
    g, b, noise = _fixture_chain("traj20_preatt", synth.make_pocket_small(2), 2, [1.0, 0.85])
    r = _sample_hip(preatt_model(), b, 20, json.loads(str(g["drift"])), noise)
    _check_chain("pre_att (traj20_preatt: 20 steps, B=2, drift)", r, g, 20)


def test_preatt_resume_from_the_reference_state_with_start_step():
    """The last 12 steps of traj20_preatt restarted with start_step = 8 from the reference's own state after 8 steps."""
    g, b, noise = _fixture_chain("traj20_preatt", synth.make_pocket_small(2), 2, [1.0, 0.85])
    bb = dict(b)
    bb["init_ligand_pos"] = torch.from_numpy(g["traj_pos"][7].astype(np.float32))
    bb["init_ligand_v"] = torch.from_numpy(g["traj_v"][7].astype(np.int64))
    bb["init_ligand_fc_bond_type"] = torch.from_numpy(g["traj_bond"][7].astype(np.int64))
    r = _sample_hip(preatt_model(), bb, 12, json.loads(str(g["drift"])), {k: v[8:] for k, v in noise.items()}, start_step=8)
    err = maxabs(r["pos"], g["out_pos"])
    print(f"pre_att: steps 8..19 resumed from the reference's step-8 state: final pos err {err:.3g}")
    assert err < POS_TOL
    assert np.array_equal(r["v"].cpu().numpy(), g["out_v"]) and np.array_equal(r["bond"].cpu().numpy(), g["out_bond"])


@pytest.mark.parametrize("drift", [False, True])
def test_resumed_preatt_chain_is_the_unsplit_chain(drift):
    """Philox noise, frame fixed (center_pos_mode='none'): 16 steps in one call == 6 steps, then 10 with start_step = 6, bit for bit."""
    torch.manual_seed(5)
    b = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in synth.build_sampling_batch(synth.make_pocket_small(3), 4).items()}
    m = preatt_model()
    kw = dict(center_pos_mode="none", energy_drift_opt=GU.DRIFT if drift else None, seed=77)
    full = m.sample_diffusion(num_steps=16, **b, **kw)
    first = m.sample_diffusion(num_steps=6, **b, **kw)
    b2 = dict(b)
    b2["init_ligand_pos"], b2["init_ligand_v"], b2["init_ligand_fc_bond_type"] = first["pos"], first["v"], first["bond"]
    rest = m.sample_diffusion(num_steps=10, start_step=6, **b2, **kw)
    for k in ("pos", "v", "bond"):
        assert torch.equal(rest[k], full[k]), k
    assert bool(torch.isfinite(full["pos"]).all())


def test_preatt_graph_replay_equals_eager_launches():
    g, b, noise = _fixture_chain("traj20_preatt", synth.make_pocket_small(2), 2, [1.0, 0.85])
    n5 = {k: v[:5] for k, v in noise.items()}
    drift = json.loads(str(g["drift"]))
    r1 = _sample_hip(preatt_model(), b, 5, drift, n5, use_graph=True)
    r2 = _sample_hip(preatt_model(), b, 5, drift, n5, use_graph=False)
    for k in ("pos", "v", "bond"):
        assert torch.equal(r1[k], r2[k]), k
    assert torch.equal(torch.stack(r1["pos_traj"]), torch.stack(r2["pos_traj"]))
    assert torch.equal(torch.stack(r1["bt_traj"]), torch.stack(r2["bt_traj"]))
    assert maxabs(torch.stack(r1["pos_traj"]), g["traj_pos"][:5]) < POS_TOL


def test_preatt_padded_heterogeneous_batch_equals_size_groups(monkeypatch):
    """One padded launch sequence (the default) against one dense group per size (DD_RAGGED_MODE=groups: several chains replayed
    together through dd_sample_steps_graph_multi_ex), armsca + clash drift, injected noise."""
    sizes, n_prot = [9, 37, 20, 33, 17, 25], [150, 260, 120, 200, 180, 131]
    b = _hetero_batch(sizes, n_prot, seed=4)
    steps = 4
    noise = synth.draw_step_noise(steps, b["init_ligand_pos"].size(0), b["init_ligand_fc_bond_type"].size(0))
    outs = {}
    for mode in ("padded", "groups"):
        monkeypatch.setenv("DD_RAGGED_MODE", mode)
        outs[mode] = _sample_hip(preatt_model(), b, steps, GU.DRIFT, noise)
    p, q = outs["padded"], outs["groups"]
    err = maxabs(p["pos"], q["pos"])
    e_bt = maxabs(torch.stack(p["bt_traj"]), torch.stack(q["bt_traj"]))
    print(f"pre_att padded vs groups: pos diff {err:.3g}, bond log-prob diff {e_bt:.3g}")
    assert p["pos"].shape == (sum(sizes), 3)
    assert err < 5e-6 and e_bt < 5e-5
    assert torch.equal(p["v"], q["v"]) and torch.equal(p["bond"], q["bond"])
    assert bool(torch.isfinite(torch.stack(p["bt_traj"])).all())


def test_preatt_harness_runs_and_matches_the_model():
    """harness.sample_diffusion_ligand_decomp with a pre_att model: one batch of 2 equals model.sample_diffusion on that batch."""
    pocket = synth.make_pocket_small(5)
    out = harness.sample_diffusion_ligand_decomp(preatt_model(), pocket, num_samples=2, batch_size=2, device="cuda:0", num_steps=3,
                                                 seed=11)
    assert len(out["pred_pos"]) == 2 and all(np.isfinite(p).all() for p in out["pred_pos"])
    assert all(t.shape[0] == 3 for t in out["pred_b_traj"])


# ------------------------------------------------------------------------------------ training
def _loss_model():
    return _new_model().train()


@pytest.mark.parametrize("fixture", ["loss_grad_preatt", "loss_grad_preatt_ragged"])
def test_preatt_loss_and_gradients_match_reference(fixture):
    g = GU.load(fixture)
    m = _loss_model()
    kw = _loss_kwargs(g)
    torch.manual_seed(int(g["noise_seed"]))
    res = m.get_diffusion_loss(**kw)
    _check_losses(f"eager {fixture}", res["losses"], g, rel=2e-3)
    assert maxabs(res["pred_ligand_pos"], g["out_pred_ligand_pos"]) < 1e-4
    assert maxabs(res["pred_ligand_v"], g["out_pred_ligand_v"]) < 1e-4
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
    print(f"pre_att {fixture}: {len(names)} parameter gradients, worst relative tensor error {worst:.2g}, norm error {rel_n.max():.2g}")
    assert rel_n.max() < 2e-3
    assert all(params[n].grad is not None for n in names)
    assert tuple(params["bond_inference.0.weight"].grad.shape) == (128, 148)


@pytest.mark.parametrize("fixture", ["loss_grad_preatt", "loss_grad_preatt_ragged"])
def test_preatt_validation_loss_uses_the_fused_forward_and_agrees(fixture):
    g = GU.load(fixture)
    m = _new_model()
    kw = _loss_kwargs(g)
    with torch.no_grad():
        torch.manual_seed(int(g["noise_seed"]))
        v = m.get_diffusion_loss(**kw)
    assert not v["losses"]["pos"].requires_grad
    _check_losses(f"no_grad {fixture}", v["losses"], g)
    assert maxabs(v["pred_ligand_pos"], g["out_pred_ligand_pos"]) < 1e-4


@pytest.mark.parametrize("fixture", ["loss_grad_preatt", "loss_grad_preatt_ragged"])
def test_preatt_graphed_train_step_matches_reference(fixture):
    """GraphedTrainStep with lr = 0: two eager iterations, then the captured one -- losses and gradients against the reference."""
    g = GU.load(fixture)
    m = _loss_model()
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


# ------------------------------------------------------------------------------------ the lin model beside it
def test_lin_model_unchanged_after_preatt_ran():
    """In the same process, after every pre_att case: the lin model still reproduces its shipped fixtures."""
    preatt_model()
    m = lin_model(0)
    g = GU.load("forward_small")
    out = _forward_hip(m, GU.batch_from_npz(g))
    e = max(maxabs(out[k], g["out_" + k]) for k in ("pred_ligand_pos", "pred_ligand_v", "pred_bond"))
    gs = GU.load("steps")
    b, drift, noise = _step_case(gs, 500, "drift")
    r = _sample_hip(m, b, 1, drift, noise, 500)
    e_pos = maxabs(r["pos"], gs["t500_drift_pos"])
    print(f"lin model after pre_att: forward {e:.3g}, step t=500 drift pos {e_pos:.3g}")
    assert e < 2e-4 and e_pos < POS_TOL
    assert torch.equal(r["bond"].cpu(), torch.from_numpy(gs["t500_drift_bond"]))
