"""GPU (-m gpu): training.network with DD_TRAIN_FUSED_ATTN=1 -- every attention site of a layer as one differentiable op call
(functional.scatter_attention / scatter_attention_pos on the layer's SegmentPlan: dd_attn_aggregate_* forward,
dd_attn_aggregate_*_bwd backward).  Judged exactly as the composed path is: the cases, the scalar, the metric and the bound of
tests/train_grad_cases.py through test_gpu_train_grad._judge, with an EMPTY exemption table -- the fused sites have no atomic
index_add_, so a tensor over its bound here is a finding about the kernels.  A spy counts the op calls; one GraphedTrainStep
run shows that the fused step captures (no device -> host round trip) and that its replays follow the eager fused steps."""
import pytest
import torch

import test_gpu_train_grad as TGG
import train_grad_cases as TG
from decompdiff_amd import DecompScorePosNet3D, shipped_config, synth, training
from decompdiff_amd import functional as FN
from test_gpu_parity import dev, to_dev

pytestmark = pytest.mark.gpu


def _spy(monkeypatch):
    calls = dict(node=0, pos=0)
    node, pos = FN.scatter_attention, FN.scatter_attention_pos

    def spy_node(*a, **k):
        calls["node"] += 1
        return node(*a, **k)

    def spy_pos(*a, **k):
        calls["pos"] += 1
        return pos(*a, **k)
    monkeypatch.setattr(FN, "scatter_attention", spy_node)
    monkeypatch.setattr(FN, "scatter_attention_pos", spy_pos)
    return calls


def _network(m, b):
    return training.network(m, b["protein_pos"], b["protein_v"], b["batch_protein"], b["init_ligand_pos"], b["init_ligand_v"],
                            b["ligand_v_aux"], b["batch_ligand"], b["ligand_fc_bond_index"], b["init_ligand_fc_bond_type"])


@pytest.mark.parametrize("regime,shape", sorted(TG.cases(TG.DENSE)))
def test_fused_network_gradients_vs_fp64_autograd(regime, shape, monkeypatch):
    monkeypatch.setenv("DD_TRAIN_FUSED_ATTN", "1")
    monkeypatch.setattr(TGG, "EXEMPT", {})                 # no exemptions for the fused route
    monkeypatch.setattr(TGG, "_WORST", {})                 # (the composed path's parity summary stays its own)
    calls = _spy(monkeypatch)
    ref = TG.reference(regime, shape)
    m = TGG.model_for(regime)
    m.zero_grad(set_to_none=True)
    out = _network(m, to_dev(ref["batch"]))
    L = int(ref["cfg"].num_layers)
    assert calls == dict(node=3 * L, pos=2 * L), calls     # (NL = 3 still has triplets: one member per bond)
    TGG._judge(regime, shape, "fused", m, out, ref)


def test_switch_off_makes_no_fused_call(monkeypatch):
    monkeypatch.delenv("DD_TRAIN_FUSED_ATTN", raising=False)
    calls = _spy(monkeypatch)
    ref = TG.reference("synthetic", "tiny_20+3_B2")
    m = TGG.model_for("synthetic")
    with torch.no_grad():
        _network(m, to_dev(ref["batch"]))
    monkeypatch.setenv("DD_TRAIN_FUSED_ATTN", "0")
    with torch.no_grad():
        _network(m, to_dev(ref["batch"]))
    assert calls == dict(node=0, pos=0), calls


def test_graphed_fused_train_step_follows_the_eager_fused_steps(monkeypatch):
    """The form of test_gpu_training.test_graphed_train_step_follows_the_eager_steps, one shape, eight steps, both runs fused."""
    monkeypatch.setenv("DD_TRAIN_FUSED_ATTN", "1")
    calls = _spy(monkeypatch)
    torch.manual_seed(3)
    b = synth.build_sampling_batch(synth.make_pocket(31, 80, (4, 4), 6, num_full_protein=0), 3)
    d = lambda t: t.to(dev()) if torch.is_tensor(t) else t
    kw = dict(
        protein_pos=d(b["protein_pos"]), protein_v=d(b["protein_v"]), batch_protein=d(b["batch_protein"]),
        protein_group_idx=d(b["protein_group_idx"]), ligand_pos=d(b["init_ligand_pos"]), ligand_v=d(b["init_ligand_v"]),
        ligand_v_aux=d(b["ligand_v_aux"]), batch_ligand=d(b["batch_ligand"]), ligand_group_idx=d(b["ligand_group_idx"]),
        prior_centers=d(b["prior_centers"]), prior_stds=d(b["prior_stds"]), prior_num_atoms=d(b["prior_num_atoms"]),
        batch_prior=d(b["batch_prior"]), prior_group_idx=d(b["prior_group_idx"]), ligand_decomp_batch=d(b["ligand_decomp_batch"]),
        ligand_decomp_index=d(b["ligand_decomp_index"]), ligand_fc_bond_index=d(b["ligand_fc_bond_index"]),
        ligand_fc_bond_type=d(b["init_ligand_fc_bond_type"]), batch_ligand_bond=d(b["batch_ligand_bond"]))

    def fresh(capturable):
        m = DecompScorePosNet3D(shipped_config(), 29, 10, 8)
        sd = m.state_dict(); sd.update(synth.synthetic_state_dict(shipped_config(), 1)); m.load_state_dict(sd)
        m = m.to(dev()).train()
        return m, torch.optim.Adam(m.parameters(), lr=1e-4, capturable=capturable)

    steps, L = 8, int(shipped_config().num_layers)
    m_e, opt_e = fresh(False)
    torch.manual_seed(11)
    eager = []
    for _ in range(steps):
        opt_e.zero_grad(set_to_none=True)
        r = m_e.get_diffusion_loss(**kw)
        loss = r["losses"]["pos"] + 100.0 * r["losses"]["v"] + 100.0 * r["losses"]["bond"]
        loss.backward(); opt_e.step()
        eager.append(float(loss))
    assert calls == dict(node=3 * L * steps, pos=2 * L * steps), calls
    m_g, opt_g = fresh(True)
    gs = training.GraphedTrainStep(m_g, opt_g, loss_weights=(1.0, 100.0, 100.0), warmup=2)
    torch.manual_seed(11)
    graphed = [float(gs.step(**kw)["loss"]) for _ in range(steps)]
    print(f"\nFUSEDGRAPH eager {eager}\nFUSEDGRAPH graphed {graphed}")
    assert gs.replays == steps - 2 and gs.eager_steps == 2 and len(gs._graphs) == 1
    # two warm-up steps and one capture ran the network's Python: the replays did not
    assert calls == dict(node=3 * L * (steps + 3), pos=2 * L * (steps + 3)), calls
    for a, c in zip(eager, graphed):
        assert abs(a - c) <= 2e-4 * max(1.0, abs(a)), (eager, graphed)
