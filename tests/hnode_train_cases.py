"""GPU cases of the training objective with the narrow bond layer (h_node_in_bond_net = False): loss and all 572 parameter
gradients through network (dense fixture), network_padded and network_grouped (ragged fixture) with DD_TRAIN_FUSED_ATTN 0 and 1,
against fixtures from the reference itself (tools/make_hnode_golden.py) at the bounds of tests/outfc_train_cases.py; the narrow
model against its zero-extended wide twin (tests/test_hnode_host.py zero_extend); the torch.no_grad validation path and one
GraphedTrainStep capture and replay.  Run by tests/test_gpu_hnode_training.py in a process of their own."""
import re

import numpy as np
import pytest
import torch

import blocks_fixtures as BF
import golden_utils as GU
from decompdiff_amd import shipped_config, synth, training
from hnode_cases import _batch, _load
from noise_param_cases import _check_losses
from test_gpu_parity import dev, maxabs
from test_gpu_training import _grads_agree, _loss_kwargs
from test_hnode_host import narrow_config, zero_extend

pytestmark = pytest.mark.gpu


def _narrow():
    cfg = narrow_config()
    return _load(cfg, synth.synthetic_state_dict(cfg, 0)).train()


def _total(res):
    return res["losses"]["pos"] + 100.0 * res["losses"]["v"] + 100.0 * res["losses"]["bond"]


@pytest.mark.parametrize("fused", ["0", "1"], ids=["aten-attn", "fused-attn"])
@pytest.mark.parametrize("fixture,mode", [("loss_grad_hnode", None), ("loss_grad_hnode_ragged", "padded"),
                                          ("loss_grad_hnode_ragged", "groups")])
def test_hnode_loss_and_gradients_match_reference(fixture, mode, fused, monkeypatch):
    monkeypatch.setenv("DD_TRAIN_FUSED_ATTN", fused)
    if mode is not None:
        monkeypatch.setenv("DD_TRAIN_PAD", "1" if mode == "padded" else "0")
    g = GU.load(fixture)
    m = _narrow()
    kw = _loss_kwargs(g)
    torch.manual_seed(int(g["noise_seed"]))
    res = m.get_diffusion_loss(**kw)
    tag = f"hnode {fixture} {mode or 'dense'} fused_attn={fused}"
    _check_losses(f"eager {tag}", res["losses"], g, rel=2e-3)
    assert maxabs(res["pred_ligand_pos"], g["out_pred_ligand_pos"]) < 1e-4
    assert maxabs(res["pred_ligand_v"], g["out_pred_ligand_v"]) < 1e-4
    _total(res).backward()
    params = dict(m.named_parameters())
    worst = 0.0
    for key in [k for k in g.files if k.startswith("grad__")]:
        name = key[len("grad__"):].replace("__", ".")
        want = torch.from_numpy(g[key])
        rel = float((params[name].grad.cpu() - want).abs().max() / want.abs().max().clamp(min=1e-12))
        worst = max(worst, rel)
        assert rel < 2e-3, (name, rel)
    names = [str(n) for n in g["grad_norm_names"]]
    assert len(names) == 572
    assert tuple(params["refine_net.base_block.0.bond_layer.hk_func.net.0.weight"].grad.shape) == (128, 181)
    got_norms = np.array([float(params[n].grad.double().norm()) if params[n].grad is not None else 0.0 for n in names])
    rel_n = np.abs(got_norms - g["grad_norms"]) / np.maximum(g["grad_norms"], 1e-6 * g["grad_norms"].max())
    print(f"{tag}: {len(names)} parameter gradients, worst relative tensor error {worst:.2g}, norm error {rel_n.max():.2g}")
    assert rel_n.max() < 2e-3
    assert all(params[n].grad is not None for n in names)


@pytest.mark.parametrize("fixture", ["loss_grad_hnode", "loss_grad_hnode_ragged"])
def test_hnode_validation_loss_uses_the_fused_forward_and_agrees(fixture):
    g = GU.load(fixture)
    m = _narrow().eval()
    kw = _loss_kwargs(g)
    with torch.no_grad():
        torch.manual_seed(int(g["noise_seed"]))
        v = m.get_diffusion_loss(**kw)
    assert not v["losses"]["pos"].requires_grad
    _check_losses(f"no_grad hnode {fixture}", v["losses"], g)
    assert maxabs(v["pred_ligand_pos"], g["out_pred_ligand_pos"]) < 1e-4


@pytest.mark.parametrize("fused", ["0", "1"], ids=["aten-attn", "fused-attn"])
@pytest.mark.parametrize("fixture", ["loss_grad_hnode", "loss_grad_hnode_ragged"])
def test_hnode_loss_equals_the_zero_extended_wide_model(fixture, fused, monkeypatch):
    """Losses bit for bit; gradients on the shared slices within the bound two backward passes of one model are held to
    (tests/test_gpu_training.py _grads_agree); the wide model's gradient on its zero columns is not constrained.

    What makes the losses equal: the key / value first Linears are split by columns over the library's GEMMs (the wide model adds
    gathered zero projections), the narrow query Linear is the wide network's 256-column product with a zero atom half, and the
    centring offset of a ragged batch is a fixed-order sum."""
    monkeypatch.setenv("DD_TRAIN_FUSED_ATTN", fused)
    g = GU.load(fixture)
    kw = _loss_kwargs(g)
    cfg = narrow_config()
    sd = synth.synthetic_state_dict(cfg, 0)
    out = []
    for m in (_load(cfg, sd).train(), _load(shipped_config(), zero_extend(sd)).train()):
        torch.manual_seed(int(g["noise_seed"]))
        res = m.get_diffusion_loss(**kw)
        _total(res).backward()
        out.append(({k: res["losses"][k].detach().clone() for k in ("pos", "v", "bond")},
                    {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}))
    (ln, gn), (lw, gw) = out
    for k in ("pos", "v", "bond"):
        print(f"hnode zero extension, training {fixture} fused_attn={fused} loss {k}: narrow {float(ln[k]):.9g} wide {float(lw[k]):.9g} "
              f"diff {abs(float(ln[k]) - float(lw[k])):.3g}")
    shared = {}
    for n, t in gw.items():
        m_ = re.search(r"\.bond_layer\.(hk|hv|hq)_func\.net\.0\.weight$", n)
        shared[n] = t[:, :(128 if m_.group(1) == "hq" else 181)] if m_ else t
    _grads_agree(gn, shared)
    for k in ("pos", "v", "bond"):
        assert torch.equal(ln[k], lw[k]), (k, float(ln[k]), float(lw[k]))


def test_hnode_graphed_train_step_capture_and_replay():
    """GraphedTrainStep at 2 x (44 + 12) atoms with lr = 0: two eager iterations, then the captured one -- the same losses and
    gradients."""
    b = _batch(44, (3, 3), 6, 2, seed=2023)
    kw = BF.loss_kwargs(b, [500, 20], dev())
    m = _narrow()
    opt = torch.optim.Adam(m.parameters(), lr=0.0, capturable=True)
    gs = training.GraphedTrainStep(m, opt, loss_weights=(1.0, 100.0, 100.0), warmup=2)
    losses, grads = [], []
    for _ in range(3):
        torch.manual_seed(7)
        out = gs.step(**kw)
        losses.append({k: float(out["losses"][k]) for k in ("pos", "v", "bond")})
        grads.append({n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None})
    assert gs.replays == 1 and gs.eager_steps == 2
    assert len(grads[2]) == 572
    print("graphed hnode train step: eager " + str(losses[1]) + " captured " + str(losses[2]))
    for k in ("pos", "v", "bond"):
        assert abs(losses[2][k] - losses[1][k]) <= 1e-4 * max(1.0, abs(losses[1][k])), k
    _grads_agree(grads[2], grads[1])
