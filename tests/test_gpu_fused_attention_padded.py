"""GPU (-m gpu): DD_TRAIN_FUSED_ATTN=1 in a PADDED pass (training.network_padded / objective_padded: a batch of different
complexes as one dense pass) -- the bond-graph and triplet attention sites as one masked op call each
(functional.scatter_attention / scatter_attention_pos with member_mask: dd_attn_aggregate_*_masked and their backward), the kNN
sites unmasked (dd_knn_masked keeps padding atoms out of the graph).  The batch is the ragged pair of tests/train_grad_cases.py
(30 + 9 and 44 + 14 atoms, signed_sharp): padding members exist at both masked sites.  Judged exactly as the composed padded
route is -- test_gpu_train_grad._judge against the float64 oracle, the bounds of train_grad_cases.bounds unchanged, with an EMPTY
exemption table.  A spy counts the op calls and the masks they carry; one GraphedTrainStep run shows that the padded fused step
captures, that its replays follow the eager fused steps, and that a graph belongs to the setting it was captured under."""
import pytest
import torch

import test_gpu_train_grad as TGG
import train_grad_cases as TG
from decompdiff_amd import DecompScorePosNet3D, shipped_config, synth, training
from decompdiff_amd import functional as FN
from test_gpu_parity import dev, to_dev

pytestmark = pytest.mark.gpu

REGIME = "signed_sharp"
N_P, N_L = [s[0] for s in TG.RAGGED_SIZES], [s[1] for s in TG.RAGGED_SIZES]


def _spy(monkeypatch, masks=None):
    """Counts the op calls and those that carry a member_mask; the masks themselves are appended to `masks`."""
    calls = dict(node=0, pos=0, node_masked=0, pos_masked=0)
    masks = [] if masks is None else masks
    node, pos = FN.scatter_attention, FN.scatter_attention_pos

    def spy_node(*a, **k):
        calls["node"] += 1
        m = k.get("member_mask")
        if m is not None:                                  # (no device -> host round trip in here: the spy runs inside a capture too)
            assert m.dtype == torch.bool and m.numel() == a[1].size(0)
            calls["node_masked"] += 1
            masks.append(m)
        return node(*a, **k)

    def spy_pos(*a, **k):
        calls["pos"] += 1
        m = k.get("member_mask")
        if m is not None:
            assert m.dtype == torch.bool and m.numel() == a[1].size(0)
            calls["pos_masked"] += 1
            masks.append(m)
        return pos(*a, **k)
    monkeypatch.setattr(FN, "scatter_attention", spy_node)
    monkeypatch.setattr(FN, "scatter_attention_pos", spy_pos)
    return calls


def _padded(m, b):
    out = training.network_padded(m, b["protein_pos"], b["protein_v"], b["init_ligand_pos"], b["init_ligand_v"], b["ligand_v_aux"],
                                  b["init_ligand_fc_bond_type"], N_P, N_L)
    assert out is not None, "every sample has K + 1 real atoms: the padded route must take the batch"
    return out


def test_padded_fused_network_gradients_vs_fp64_autograd(monkeypatch):
    monkeypatch.setenv("DD_TRAIN_FUSED_ATTN", "1")
    monkeypatch.setattr(TGG, "EXEMPT", {})                 # no exemptions for the fused route
    monkeypatch.setattr(TGG, "_WORST", {})                 # (the composed path's parity summary stays its own)
    masks = []
    calls = _spy(monkeypatch, masks)
    ref = TG.reference(REGIME, TG.RAGGED)
    m = TGG.model_for(REGIME)
    m.zero_grad(set_to_none=True)
    out = _padded(m, to_dev(ref["batch"]))
    L = int(ref["cfg"].num_layers)
    assert len(masks) == 3 * L and all(bool(x.any()) and not bool(x.all()) for x in masks), "padding members at every masked site"
    # per layer: kNN node, bond-graph node (masked), triplet (masked); kNN coordinate, bond-graph coordinate (masked)
    assert calls == dict(node=3 * L, pos=2 * L, node_masked=2 * L, pos_masked=L), calls
    TGG._judge(REGIME, TG.RAGGED, "padded_fused", m, out, ref)


def test_switch_off_makes_no_fused_call_in_a_padded_pass(monkeypatch):
    calls = _spy(monkeypatch)
    ref = TG.reference(REGIME, TG.RAGGED)
    m = TGG.model_for(REGIME)
    b = to_dev(ref["batch"])
    monkeypatch.delenv("DD_TRAIN_FUSED_ATTN", raising=False)
    with torch.no_grad():
        _padded(m, b)
    monkeypatch.setenv("DD_TRAIN_FUSED_ATTN", "0")
    with torch.no_grad():
        _padded(m, b)
    assert calls == dict(node=0, pos=0, node_masked=0, pos_masked=0), calls


def test_graphed_padded_fused_train_step_follows_the_eager_fused_steps(monkeypatch):
    """The form of test_gpu_fused_attention_training's captured step on the ragged pair: six steps, both runs fused."""
    monkeypatch.setenv("DD_TRAIN_FUSED_ATTN", "1")
    calls = _spy(monkeypatch)
    b = TG.ragged_batch()
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

    steps, L = 6, int(shipped_config().num_layers)
    per_step = dict(node=3 * L, pos=2 * L, node_masked=2 * L, pos_masked=L)
    m_e, opt_e = fresh(False)
    torch.manual_seed(11)
    eager = []
    for _ in range(steps):
        opt_e.zero_grad(set_to_none=True)
        r = m_e.get_diffusion_loss(**kw)
        loss = r["losses"]["pos"] + 100.0 * r["losses"]["v"] + 100.0 * r["losses"]["bond"]
        loss.backward(); opt_e.step()
        eager.append(float(loss))
    assert calls == {k: v * steps for k, v in per_step.items()}, calls
    m_g, opt_g = fresh(True)
    gs = training.GraphedTrainStep(m_g, opt_g, loss_weights=(1.0, 100.0, 100.0), warmup=2)
    torch.manual_seed(11)
    graphed = [float(gs.step(**kw)["loss"]) for _ in range(steps)]
    print(f"\nFUSEDPADGRAPH eager {eager}\nFUSEDPADGRAPH graphed {graphed}")
    assert gs.replays == 4 and gs.eager_steps == 2 and len(gs._graphs) == 1
    assert next(iter(gs._graphs))[0] == "padded"
    # two warm-up steps and one capture ran the network's Python: the replays did not
    assert calls == {k: v * (steps + 3) for k, v in per_step.items()}, calls
    for a, c in zip(eager, graphed):
        assert abs(a - c) <= 2e-4 * max(1.0, abs(a)), (eager, graphed)
    # a graph belongs to the setting it was captured under: with the switch unset the next step of the same shape does not replay
    # the fused graph (it is a warm-up step of a new entry) ...
    monkeypatch.delenv("DD_TRAIN_FUSED_ATTN", raising=False)
    before = dict(calls)
    assert bool(torch.isfinite(gs.step(**kw)["loss"]))
    assert gs.replays == 4 and gs.eager_steps == 3 and len(gs._graphs) == 1
    # ... and after its warm-up that entry is captured beside the first, on the composed path
    for _ in range(2):
        assert bool(torch.isfinite(gs.step(**kw)["loss"]))
    assert len(gs._graphs) == 2 and gs.replays == 5 and gs.eager_steps == 4
    assert sorted(k[-1] for k in gs._graphs) == [False, True]
    assert calls == before, "the composed padded step makes no fused call"
