"""GPU (-m gpu): ``DecompScorePosNet3D.forward()`` on a PyG-style batch of DIFFERENT complexes (protein and ligand counts all
different, one ligand beyond 64 atoms) against per-sample ``forward()`` calls and against the oracle.

Criteria, none of them new:
  * collated vs per-sample forward: the bounds of the existing comparison of one padded launch sequence with the per-size dense
    groups (tests/test_gpu_configs.py::test_padded_heterogeneous_batch_equals_size_groups: coordinates 5e-6, log-probabilities
    5e-5) -- the padded launch runs the masked kernels without the layer-0 tables, the per-sample calls the dense ones with them,
    so the sums associate differently; a batch that takes the size-group fallback runs the very same dense call per sample and
    must be bit-identical;
  * vs the oracle per sample: the tolerances of the single-forward parity test (tests/test_gpu_parity.py: POS_TOL / LOGIT_TOL)."""
import pytest
import torch

import golden_utils as GU
from decompdiff_amd import DecompScorePosNet3D, shipped_config, synth, training
from oracle import model as OM

pytestmark = pytest.mark.gpu
POS_TOL = 1e-4          # tests/test_gpu_parity.py
LOGIT_TOL = 1e-4
PAD_POS_TOL = 5e-6      # tests/test_gpu_configs.py: padded launch vs size groups
PAD_LOGIT_TOL = 5e-5
KEYS = ("pred_ligand_pos", "pred_ligand_v", "pred_bond")


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def maxabs(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


_MODELS = {}


def model(kind="lin"):
    if kind not in _MODELS:
        nc = 13 if kind == "nc13" else 8
        cfg = shipped_config(bond_net_type="pre_att") if kind == "pre_att" else shipped_config()
        m = DecompScorePosNet3D(cfg, 29, nc + 2, nc)
        sd = m.state_dict()
        sd.update(synth.synthetic_state_dict(cfg, 0, ligand_atom_feature_dim=nc + 2, num_classes=nc))
        m.load_state_dict(sd, strict=True)
        _MODELS[kind] = m.to(dev())
    return _MODELS[kind]


# (protein atoms, arm atoms, scaffold atoms): ligands of 66, 9 and 20 atoms in pockets of 44, 61 and 50 -- all counts different,
# one ligand in the 8-tile kernels (beyond 64 atoms), every sample with more than knn + 1 = 33 atoms
SHAPES = [(44, (22, 22), 22), (61, (3, 3), 3), (50, (6, 6), 8)]
TINY = [(44, (22, 22), 22), (20, (2, 2), 2), (50, (6, 6), 8)]      # second sample: 20 + 6 = 26 atoms < knn + 1 -> size groups
_BATCHES = {}


def samples(shapes_key="SHAPES", nc=8):
    """The per-sample batches (CPU) of a set of shapes, drawn once."""
    key = (shapes_key, nc)
    if key not in _BATCHES:
        torch.manual_seed(17)
        shapes = SHAPES if shapes_key == "SHAPES" else TINY
        _BATCHES[key] = [synth.build_sampling_batch(synth.make_pocket(60 + i, np_, arms, sca, num_full_protein=np_ + 20), 1, num_classes=nc)
                         for i, (np_, arms, sca) in enumerate(shapes)]
    return _BATCHES[key]


def fwd(m, b, **extra):
    bd = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in b.items()}
    out = m(protein_pos=bd["protein_pos"], protein_v=bd["protein_v"], batch_protein=bd["batch_protein"],
            protein_group_idx=bd["protein_group_idx"], init_ligand_pos=bd["init_ligand_pos"], init_ligand_v=bd["init_ligand_v"],
            init_ligand_v_aux=bd["ligand_v_aux"], batch_ligand=bd["batch_ligand"], ligand_group_idx=bd["ligand_group_idx"],
            prior_centers=bd["prior_centers"], prior_stds=bd["prior_stds"], batch_prior=bd["batch_prior"],
            prior_group_idx=bd["prior_group_idx"], ligand_fc_bond_index=bd["ligand_fc_bond_index"],
            init_ligand_fc_bond_type=bd["init_ligand_fc_bond_type"], **extra)
    return {k: v.clone() for k, v in out.items()}


def per_sample(m, parts):
    outs = [fwd(m, p) for p in parts]
    return {k: torch.cat([o[k] for o in outs], 0) for k in KEYS}


def check_collated(kind, parts, tag, **extra):
    m = model(kind)
    whole = fwd(m, synth.concat_sampling_batches(parts), **extra)
    each = per_sample(m, parts)
    torch.cuda.synchronize()
    errs = {k: maxabs(whole[k], each[k]) for k in KEYS}
    print(f"ragged forward ({tag}): collated vs per-sample " + ", ".join(f"{k} {v:.3g}" for k, v in errs.items()))
    n_l = [int(p["batch_ligand"].numel()) for p in parts]
    assert whole["pred_ligand_pos"].shape == (sum(n_l), 3) and whole["pred_ligand_v"].shape == (sum(n_l), m.num_classes)
    assert whole["pred_bond"].shape == (sum(n * (n - 1) for n in n_l), 5)
    assert errs["pred_ligand_pos"] < PAD_POS_TOL and errs["pred_ligand_v"] < PAD_LOGIT_TOL and errs["pred_bond"] < PAD_LOGIT_TOL
    return whole, each


def test_ragged_forward_equals_per_sample_forward_and_the_oracle():
    parts = samples()
    assert len({int(p["batch_protein"].numel()) for p in parts}) == 3 and len({int(p["batch_ligand"].numel()) for p in parts}) == 3
    assert max(int(p["batch_ligand"].numel()) for p in parts) > 64
    whole, _ = check_collated("lin", parts, "lin head, 8 classes")
    cfg, sd = GU.weights(0)
    o_l = o_b = 0
    for i, b in enumerate(parts):
        with torch.no_grad():
            want = OM.forward(sd, cfg, b["protein_pos"], b["protein_v"], b["batch_protein"], b["init_ligand_pos"], b["init_ligand_v"],
                              b["ligand_v_aux"], b["batch_ligand"], b["ligand_fc_bond_index"], b["init_ligand_fc_bond_type"])
        nl = int(b["batch_ligand"].numel())
        nb = nl * (nl - 1)
        errs = {"pred_ligand_pos": maxabs(whole["pred_ligand_pos"][o_l:o_l + nl], want["pred_ligand_pos"]),
                "pred_ligand_v": maxabs(whole["pred_ligand_v"][o_l:o_l + nl], want["pred_ligand_v"]),
                "pred_bond": maxabs(whole["pred_bond"][o_b:o_b + nb], want["pred_bond"])}
        print(f"ragged forward, sample {i} (NL={nl}) vs the oracle: " + ", ".join(f"{k} {v:.3g}" for k, v in errs.items()))
        assert errs["pred_ligand_pos"] < POS_TOL and errs["pred_ligand_v"] < LOGIT_TOL and errs["pred_bond"] < LOGIT_TOL
        o_l, o_b = o_l + nl, o_b + nb


def test_ragged_forward_pre_att_bond_head():
    check_collated("pre_att", samples(), "pre_att head")


def test_ragged_forward_13_atom_classes():
    parts = samples(nc=13)
    assert max(int(p["init_ligand_v"].max()) for p in parts) >= 8
    check_collated("nc13", parts, "13 classes")


def test_ragged_forward_honours_ligand_atom_mask():
    parts = samples()
    n = sum(int(p["batch_ligand"].numel()) for p in parts)
    plain = fwd(model("lin"), synth.concat_sampling_batches(parts))
    masked, _ = check_collated("lin", parts, "all-True ligand_atom_mask", ligand_atom_mask=torch.ones(n, dtype=torch.bool, device=dev()))
    assert all(torch.equal(plain[k], masked[k]) for k in KEYS)            # an all-True mask is None (as in the dense path)
    mask = torch.ones(n, dtype=torch.bool, device=dev())
    mask[3] = False
    with pytest.raises(RuntimeError):                                      # what the dense forward does with such a mask
        fwd(model("lin"), synth.concat_sampling_batches(parts), ligand_atom_mask=mask)
    with pytest.raises(ValueError):
        fwd(model("lin"), synth.concat_sampling_batches(parts), ligand_atom_mask=mask[:-1])


def test_ragged_forward_with_a_sample_below_knn_plus_one_atoms(monkeypatch):
    """A 26-atom sample (kNN lists shorter than the others'): one dense call per size group -- here the per-sample calls
    themselves, so the outputs are bit-identical.  DD_RAGGED_MODE=groups sends any ragged batch the same way."""
    parts = samples("TINY")
    assert min(int(p["batch_protein"].numel()) + int(p["batch_ligand"].numel()) for p in parts) < model("lin").config.knn + 1
    whole, each = check_collated("lin", parts, "size-group fallback")
    assert all(torch.equal(whole[k], each[k]) for k in KEYS)
    monkeypatch.setenv("DD_RAGGED_MODE", "groups")
    whole, each = check_collated("lin", samples(), "DD_RAGGED_MODE=groups")
    assert all(torch.equal(whole[k], each[k]) for k in KEYS)


def test_no_grad_loss_on_the_ragged_batch_keeps_the_grouped_path(monkeypatch):
    """get_diffusion_loss under torch.no_grad() still runs one dense fused forward per size group (training.network_grouped) and
    forward() never sees the ragged batch.  Pinned in two ways:
      * the network output of the call is, bit for bit, the grouped path called here on the very tensors the objective handed to it
        (one dense fused forward per size group, the same launches on the same inputs);
      * the losses and predictions equal those of the grouped path run from scratch (`training.diffusion_loss` with the fused
        forward as the network) within the bounds tests/test_gpu_training.py uses between two evaluations of one objective
        (test_validation_loss_uses_the_fused_forward_and_agrees: losses 1e-5 relative to max(1, |loss|), coordinates 2e-5).  Two
        runs from scratch are not bit-identical: for samples of different sizes the objective centres the batch with ATen's
        index_add_ (atomic adds, order of summation not fixed), so the network inputs may differ in the last bit."""
    m = model("lin")
    b = synth.concat_sampling_batches(samples())
    d = lambda t: t.to(dev()) if torch.is_tensor(t) else t
    B = int(b["batch_protein"].max()) + 1
    kw = dict(protein_pos=d(b["protein_pos"]), protein_v=d(b["protein_v"]), batch_protein=d(b["batch_protein"]),
              protein_group_idx=d(b["protein_group_idx"]), ligand_pos=d(b["init_ligand_pos"]), ligand_v=d(b["init_ligand_v"]),
              ligand_v_aux=d(b["ligand_v_aux"]), batch_ligand=d(b["batch_ligand"]), ligand_group_idx=d(b["ligand_group_idx"]),
              prior_centers=d(b["prior_centers"]), prior_stds=d(b["prior_stds"]), prior_num_atoms=d(b["prior_num_atoms"]),
              batch_prior=d(b["batch_prior"]), prior_group_idx=d(b["prior_group_idx"]),
              ligand_decomp_batch=d(b["ligand_decomp_batch"]), ligand_decomp_index=d(b["ligand_decomp_index"]),
              ligand_fc_bond_index=d(b["ligand_fc_bond_index"]), ligand_fc_bond_type=d(b["init_ligand_fc_bond_type"]),
              batch_ligand_bond=d(b["batch_ligand_bond"]), time_step=torch.tensor([700, 40, 333][:B], device=dev()))
    calls, seen = [], []
    inner = m._forward_heterogeneous
    monkeypatch.setattr(m, "_forward_heterogeneous", lambda *a, **k: (calls.append(1), inner(*a, **k))[1], raising=False)
    grouped = training.network_grouped

    def recording(net, model_, *args, **kwargs):
        out = grouped(net, model_, *args, **kwargs)
        seen.append((args, kwargs, out))
        return out

    def net(model_, p_pos, p_v, b_p, x_t, v_t, aux, b_l, fc, b_t):          # the fused forward on ONE dense size group
        assert not model_._is_ragged(b_p, b_l)
        return model_.forward(p_pos, p_v, b_p, None, x_t, v_t, aux, b_l, None, None, None, None, None, fc, b_t)
    with torch.no_grad():
        monkeypatch.setattr(training, "network_grouped", recording)
        torch.manual_seed(3)
        got = m.get_diffusion_loss(**kw)
        monkeypatch.setattr(training, "network_grouped", grouped)
        assert len(seen) == 1 and not calls
        args, kwargs, out = seen[0]
        again = grouped(net, m, *args, **kwargs)                              # same inputs, the grouped path called directly
        torch.manual_seed(3)
        want = training.diffusion_loss(m, kw["protein_pos"], kw["protein_v"], kw["batch_protein"], kw["ligand_pos"], kw["ligand_v"],
                                       kw["ligand_v_aux"], kw["batch_ligand"], kw["prior_centers"], kw["prior_stds"],
                                       kw["prior_num_atoms"], kw["batch_prior"], kw["ligand_decomp_batch"],
                                       kw["ligand_fc_bond_index"], kw["ligand_fc_bond_type"], kw["batch_ligand_bond"],
                                       time_step=kw["time_step"], network_fn=net)
    assert not calls
    assert torch.equal(got["pred_ligand_pos"], out["pred_ligand_pos"]) and torch.equal(got["pred_ligand_v"], out["pred_ligand_v"])
    for k in KEYS:
        assert torch.equal(out[k], again[k]), k
    for k in ("pos", "v", "bond"):
        a, w = float(got["losses"][k]), float(want["losses"][k])
        print(f"no-grad loss {k}: {a:.7g} (grouped path from scratch {w:.7g})")
        assert torch.isfinite(got["losses"][k]) and abs(a - w) < 1e-5 * max(1.0, abs(w))
    e_pos, e_v = maxabs(got["pred_ligand_pos"], want["pred_ligand_pos"]), maxabs(got["pred_ligand_v"], want["pred_ligand_v"])
    print(f"no-grad loss, two runs from scratch: pred_ligand_pos {e_pos:.3g}, pred_ligand_v {e_v:.3g}")
    assert e_pos < 2e-5 and e_v < 2e-5
