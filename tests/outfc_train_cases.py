"""GPU cases of the training objective with the node output MLPs (x2h_out_fc = True): loss and all 644 parameter gradients through
network (dense fixture), network_padded and network_grouped (ragged fixture), the torch.no_grad validation path and one
GraphedTrainStep iteration, against fixtures from the reference itself (tools/make_outfc_golden.py) at the bounds of the existing
training tests.  Run by tests/test_gpu_out_fc_training.py in a process of their own."""
import numpy as np
import pytest
import torch

import golden_utils as GU
from decompdiff_amd import training
from noise_param_cases import _check_losses
from outfc_cases import _new_model
from test_gpu_parity import maxabs
from test_gpu_training import _grads_agree, _loss_kwargs

pytestmark = pytest.mark.gpu


def _loss_model():
    return _new_model().train()


@pytest.mark.parametrize("fixture,mode", [("loss_grad_outfc", None), ("loss_grad_outfc_ragged", "padded"),
                                          ("loss_grad_outfc_ragged", "groups")])
def test_outfc_loss_and_gradients_match_reference(fixture, mode, monkeypatch):
    if mode is not None:
        monkeypatch.setenv("DD_TRAIN_PAD", "1" if mode == "padded" else "0")
    g = GU.load(fixture)
    m = _loss_model()
    kw = _loss_kwargs(g)
    torch.manual_seed(int(g["noise_seed"]))
    res = m.get_diffusion_loss(**kw)
    _check_losses(f"eager {fixture} {mode}", res["losses"], g, rel=2e-3)
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
    assert len(names) == 644 and sum(".node_output." in n for n in names) == 72
    got_norms = np.array([float(params[n].grad.double().norm()) if params[n].grad is not None else 0.0 for n in names])
    rel_n = np.abs(got_norms - g["grad_norms"]) / np.maximum(g["grad_norms"], 1e-6 * g["grad_norms"].max())
    print(f"out_fc {fixture} {mode}: {len(names)} parameter gradients, worst relative tensor error {worst:.2g}, norm error {rel_n.max():.2g}")
    assert rel_n.max() < 2e-3
    assert all(params[n].grad is not None for n in names)


@pytest.mark.parametrize("fixture", ["loss_grad_outfc", "loss_grad_outfc_ragged"])
def test_outfc_validation_loss_uses_the_fused_forward_and_agrees(fixture):
    g = GU.load(fixture)
    m = _new_model()
    kw = _loss_kwargs(g)
    with torch.no_grad():
        torch.manual_seed(int(g["noise_seed"]))
        v = m.get_diffusion_loss(**kw)
    assert not v["losses"]["pos"].requires_grad
    _check_losses(f"no_grad {fixture}", v["losses"], g)
    assert maxabs(v["pred_ligand_pos"], g["out_pred_ligand_pos"]) < 1e-4


def test_outfc_graphed_train_step_equals_the_eager_one():
    """GraphedTrainStep with lr = 0: two eager iterations, then the captured one -- the same losses and gradients."""
    g = GU.load("loss_grad_outfc")
    m = _loss_model()
    opt = torch.optim.Adam(m.parameters(), lr=0.0, capturable=True)
    gs = training.GraphedTrainStep(m, opt, loss_weights=(1.0, 100.0, 100.0), warmup=2)
    kw = _loss_kwargs(g)
    grads = []
    for _ in range(3):
        torch.manual_seed(int(g["noise_seed"]))
        out = gs.step(**kw)
        _check_losses("graphed loss_grad_outfc", out["losses"], g)
        grads.append({n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None})
    assert gs.replays == 1 and gs.eager_steps == 2
    assert len(grads[2]) == 644
    _grads_agree(grads[2], grads[1], g)
