"""GPU (-m gpu): the gradients of the training network off the synthetic weights, against torch autograd through the oracle in
float64 -- the cases, the scalar, the per-tensor metric and the bound of tests/train_grad_cases.py.  training.network on the dense
shapes, training.network_padded and training.network_grouped (the size-group route, DD_TRAIN_PAD=0) on the ragged pair; both
ragged routes are held to the same float64 gradient, not to each other.  Per case: the three outputs within
stress_weights.bound(d32) of the float64 outputs, every parameter with a finite gradient, and rel_t <= bound(d32_t) for every
learnable tensor.  The bound comes from the two oracle runs alone.

Exemptions.  A case may exempt at most train_grad_cases.MAX_EXEMPT tensors, each named in EXEMPT with its demonstrated cause;
only ATen's atomic index_add_ in the remaining index_select backwards and a ReLU pre-activation within fp32 rounding of 0 that
takes the other side are causes -- a kernel is not.  The fp32 oracle needs none (tests/test_train_grad_host.py)."""
import pytest
import torch

import golden_utils as GU
import stress_weights as SW
import train_grad_cases as TG
from decompdiff_amd import DecompScorePosNet3D, shipped_config, training
from test_gpu_parity import dev, maxabs, to_dev

pytestmark = pytest.mark.gpu

# (regime, shape, route) -> {tensor name: cause}
EXEMPT = {}

_MODEL = {}
_WORST = {}


def model_for(regime):
    """One regime's model at a time (the cases are ordered by regime), in train() mode."""
    if regime not in _MODEL:
        _MODEL.clear()
        cfg = shipped_config()
        m = DecompScorePosNet3D(cfg, 29, 10, 8)
        sd = m.state_dict()
        sd.update(SW.regime_state_dict(regime, cfg))
        m.load_state_dict(sd, strict=True)
        _MODEL[regime] = m.to(dev()).train()
    return _MODEL[regime]


@pytest.fixture(scope="module", autouse=True)
def parity_lines():
    yield
    for regime, rec in sorted(_WORST.items()):
        GU.note_parity(f"training gradients vs fp64 autograd, weights '{regime}' ({rec['n']} cases): closest to its bound {rec['text']}")


def _judge(regime, shape, route, m, out, ref):
    """The assertions of one case on the outputs `out` of a network call on model m (its .grad fields are filled here)."""
    TG.scalar(out, ref["cot"]).backward()
    torch.cuda.synchronize()
    params = {n: p for n, p in m.named_parameters() if p.requires_grad}       # (the schedule tables are frozen parameters)
    assert set(params) == set(ref["grad64"]) and len(params) == TG.N_LEARNABLE
    missing = sorted(n for n, p in params.items() if p.grad is None)
    grads = {n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in params.items()}
    out_bound, bnd = TG.bounds(ref)
    errs = {k: maxabs(out[k].detach(), ref["out64"][k]) for k in SW.OUTPUTS}
    rel = TG.rel_errors(grads, ref["grad64"])
    exempt = EXEMPT.get((regime, shape, route), {})
    print(f"\nTRAINOUT {regime} {shape} {route} " + " ".join(f"{k}:{errs[k]:.2g}/{out_bound[k]:.2g}(d32 {ref['d32_out'][k]:.2g})" for k in errs))
    worst, over = TG.report(f"TRAINGRAD[{route}]", regime, shape, rel, bnd, ref["d32"], exempt)
    rec = _WORST.setdefault(regime, dict(n=0, ratio=-1.0))
    rec["n"] += 1
    if rel[worst] / bnd[worst] > rec["ratio"]:
        rec.update(ratio=rel[worst] / bnd[worst], text=f"{worst} at {shape} ({route}): rel {rel[worst]:.2g} (bound {bnd[worst]:.2g}, "
                                                          f"fp32 oracle vs fp64 {ref['d32'][worst]:.2g})")
    assert not missing, missing
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    for k in SW.OUTPUTS:
        assert out[k].shape == ref["out64"][k].shape and bool(torch.isfinite(out[k]).all()), k
        assert errs[k] < out_bound[k], (k, errs[k], out_bound[k])
    assert len(exempt) <= TG.MAX_EXEMPT and set(exempt) <= set(rel)
    assert not over, [(n, rel[n], bnd[n]) for n in over]


@pytest.mark.parametrize("regime,shape", sorted(TG.cases(TG.DENSE)))
def test_network_gradients_vs_fp64_autograd(regime, shape):
    ref = TG.reference(regime, shape)
    m = model_for(regime)
    m.zero_grad(set_to_none=True)
    b = to_dev(ref["batch"])
    out = training.network(m, b["protein_pos"], b["protein_v"], b["batch_protein"], b["init_ligand_pos"], b["init_ligand_v"],
                           b["ligand_v_aux"], b["batch_ligand"], b["ligand_fc_bond_index"], b["init_ligand_fc_bond_type"])
    _judge(regime, shape, "dense", m, out, ref)


@pytest.mark.parametrize("route", ["padded", "grouped"])
@pytest.mark.parametrize("regime", TG.SHAPES[TG.RAGGED][1])
def test_ragged_network_gradients_vs_fp64_autograd(regime, route, monkeypatch):
    """Two complexes of different size: as one padded dense pass (network_padded), and as one dense pass per size through the
    routing switch of get_diffusion_loss (network_grouped with DD_TRAIN_PAD=0)."""
    ref = TG.reference(regime, TG.RAGGED)
    m = model_for(regime)
    m.zero_grad(set_to_none=True)
    b = to_dev(ref["batch"])
    n_p, n_l = [s[0] for s in TG.RAGGED_SIZES], [s[1] for s in TG.RAGGED_SIZES]
    assert torch.bincount(ref["batch"]["batch_protein"]).tolist() == n_p and torch.bincount(ref["batch"]["batch_ligand"]).tolist() == n_l
    if route == "padded":
        out = training.network_padded(m, b["protein_pos"], b["protein_v"], b["init_ligand_pos"], b["init_ligand_v"], b["ligand_v_aux"],
                                      b["init_ligand_fc_bond_type"], n_p, n_l)
        assert out is not None, "every sample has K + 1 real atoms: the padded route must take the batch"
    else:
        monkeypatch.setenv("DD_TRAIN_PAD", "0")
        calls = []
        monkeypatch.setattr(training, "network_padded", lambda *a, **k: calls.append(1))
        out = training.network_grouped(training.network, m, b["protein_pos"], b["protein_v"], b["batch_protein"], b["init_ligand_pos"],
                                       b["init_ligand_v"], b["ligand_v_aux"], b["batch_ligand"], b["ligand_fc_bond_index"],
                                       b["init_ligand_fc_bond_type"])
        assert not calls, "DD_TRAIN_PAD=0 must route the batch through the size groups"
    _judge(regime, TG.RAGGED, route, m, out, ref)
