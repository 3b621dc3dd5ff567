"""GPU cases of the narrow bond layer (h_node_in_bond_net = False).  Two kinds of evidence:

* fixtures from the reference itself (tools/make_hnode_golden.py) at the bounds of tests/test_gpu_parity.py -- forward, single
  steps, the bench-shape chains, a 20-step chain, the combination with pre_att + x2h_out_fc + sync_twoup;
* the zero-extension identity, which needs no fixture: a WIDE model carrying the narrow weights with zero atom columns
  (tests/test_hnode_host.py zero_extend) adds exact zeros where the narrow path adds nothing, and a GEMM output element does not
  depend on how many other columns its launch forms -- so the two models must agree bit for bit on every output, at every shape
  that takes another kernel variant or tile edge, dense and padded, eager and captured.

Run by tests/test_gpu_hnode.py in a process of their own; `pytest -m gpu tests/hnode_cases.py` runs them directly."""
import json

import numpy as np
import pytest
import torch

import golden_utils as GU
from decompdiff_amd import DecompScorePosNet3D, harness, shipped_config, synth
from noise_param_cases import _step_case
from test_gpu_configs import _fixture_chain
from test_gpu_parity import LOGIT_TOL, POS_TOL, _forward_hip, _sample_hip, dev, maxabs
from test_gpu_parity import model as lin_model
from test_hnode_host import narrow_config, zero_extend

pytestmark = pytest.mark.gpu

KEYS = ("pred_ligand_pos", "pred_ligand_v", "pred_bond")
B8_STD = [1.0, 0.9, 0.8, 1.1, 1.0, 0.95, 1.05, 0.85]
REPUL = [dict(type="armsca_prox", min_d=1.2, max_d=1.9), dict(type="arms_repul", max_d=3.5, mode="min")]
_PAIRS = {}


def _load(cfg, sd, nc=8):
    m = DecompScorePosNet3D(cfg, 29, nc + 2, nc)
    full = m.state_dict()
    full.update(sd)
    m.load_state_dict(full, strict=True)
    return m.to(dev())


def pair(nc=8, **over):
    """(narrow model, the wide model with the same weights zero-extended), built once per configuration."""
    key = (nc,) + tuple(sorted(over.items()))
    if key not in _PAIRS:
        cfg = narrow_config(**over)
        sd = synth.synthetic_state_dict(cfg, 0, ligand_atom_feature_dim=nc + 2, num_classes=nc)
        _PAIRS[key] = (_load(cfg, sd, nc), _load(shipped_config(**over), zero_extend(sd), nc))
    return _PAIRS[key]


def narrow_model(**over):
    return pair(**over)[0]


# ------------------------------------------------------------------------------------ the reference's fixtures
def _forward_fixture(name, m, label):
    g = GU.load(name)
    b = GU.batch_from_npz(g)
    assert b["init_ligand_pos"].shape[0] == 2 * 12 and b["protein_pos"].shape[0] == 2 * 44
    out = _forward_hip(m, b)
    torch.cuda.synchronize()
    errs = {k: maxabs(out[k], g["out_" + k]) for k in KEYS}
    print(f"hnode {label} forward (NP=44, NL=12, B=2): " + ", ".join(f"{k} {v:.3g}" for k, v in errs.items()))
    assert errs["pred_ligand_pos"] < POS_TOL and errs["pred_ligand_v"] < LOGIT_TOL and errs["pred_bond"] < LOGIT_TOL
    return g, b


def test_forward_hnode_reference_golden():
    g, b = _forward_fixture("forward_hnode", narrow_model(), "lin")
    # a wide model with synthetic weights of its own computes something else
    lin = _forward_hip(lin_model(0), b)
    assert maxabs(lin["pred_bond"], g["out_pred_bond"]) > 1e-2


def test_forward_hnode_with_pre_att_out_fc_and_sync_twoup_reference_golden():
    _forward_fixture("forward_hnode_preatt_outfc", narrow_model(bond_net_type="pre_att", x2h_out_fc=True, sync_twoup=True),
                     "pre_att + out_fc + sync_twoup")


@pytest.mark.parametrize("t_start", [999, 500, 1, 0])
@pytest.mark.parametrize("tag", ["plain", "drift"])
def test_single_steps_hnode_reference_golden(t_start, tag):
    g = GU.load("steps_hnode")
    p = f"t{t_start}_{tag}_"
    b, drift, noise = _step_case(g, t_start, tag)
    r = _sample_hip(narrow_model(), b, 1, drift, noise, t_start)
    e_pos = maxabs(r["pos"], g[p + "pos"])
    e_lp = max(maxabs(r["vt_traj"][0], g[p + "log_v_prob"]), maxabs(r["bt_traj"][0], g[p + "log_b_prob"]),
               maxabs(r["v0_traj"][0], g[p + "log_v_recon"]))
    nv = int((r["v"].cpu() != torch.from_numpy(g[p + "v"])).sum())
    nb = int((r["bond"].cpu() != torch.from_numpy(g[p + "bond"])).sum())
    print(f"hnode step t={t_start} {tag}: pos {e_pos:.3g} log-probs {e_lp:.3g} v-mismatch {nv} bond-mismatch {nb}")
    assert e_pos < POS_TOL and e_lp < LOGIT_TOL
    assert nv == 0 and nb == 0


def _check_chain(name, label, r, g, steps, n_samples):
    """tests/test_gpu_configs.py _check_chain with the per-sample maxima kept (profiles/parity_full_chain.json)."""
    tp = torch.stack(r["pos_traj"]).numpy().astype(np.float64)
    d = np.abs(tp - g["traj_pos"]).reshape(steps, n_samples, -1).max(2)
    nv = int((torch.stack(r["v_traj"]).numpy() != g["traj_v"]).sum())
    nb = int((torch.stack(r["bond_traj"]).numpy() != g["traj_bond"]).sum())
    err = maxabs(r["pos"], g["out_pos"])
    print(f"hnode {label}: per-step max pos err {' '.join(f'{e:.2g}' for e in d.max(1))}; final {err:.3g}; type mismatches v={nv} bond={nb}")
    GU.record_parity(name, GU.chain_parity_summary(d, 1, tol=POS_TOL, type_mismatches=(nv, nb)))
    assert err < POS_TOL and d.max() < POS_TOL
    assert nv == 0 and nb == 0
    assert np.array_equal(r["v"].cpu().numpy(), g["out_v"]) and np.array_equal(r["bond"].cpu().numpy(), g["out_bond"])


@pytest.mark.parametrize("name,std_scale", [("traj3_hnode_b8_plain", None), ("traj3_hnode_b8_drift", B8_STD)])
def test_sampling_b8_hnode_reference_golden(name, std_scale):
    g, b, noise = _fixture_chain(name, synth.make_pocket_small(8), 8, std_scale)
    assert b["init_ligand_pos"].shape[0] == 8 * 30 and b["protein_pos"].shape[0] == 8 * 300
    r = _sample_hip(narrow_model(), b, 3, json.loads(str(g["drift"])), noise)
    _check_chain(f"h_node_in_bond_net=False 300+30 B=8 3 steps ({name}, reference)", f"({name}: NP=300, NL=30, B=8)", r, g, 3, 8)


def test_sampling_20_steps_hnode_reference_golden():
    g, b, noise = _fixture_chain("traj20_hnode", synth.make_pocket_small(2), 2, [1.0, 0.85])
    r = _sample_hip(narrow_model(), b, 20, json.loads(str(g["drift"])), noise)
    _check_chain("h_node_in_bond_net=False 300+30 B=2 20 steps (traj20_hnode, reference)", "(traj20_hnode: 20 steps, B=2, drift)", r, g, 20, 2)


# ------------------------------------------------------------------------------------ zero extension: forward
# (np, arms, scaffold, B): NL = 2 -- bonds without any triplet; NL = 3 -- one member per triplet segment; 3 x 20 bonds -- a partial
# 16-bond assemble tile that crosses samples; NL = 17; NL = 34 / 50 / 66 -- the first sizes of the 3-, 4- and 8-tile variants
FORWARD_SHAPES = [(40, (1,), 1, 1), (21, (1, 1), 1, 2), (7, (2, 2), 1, 3), (30, (6, 6), 5, 2), (40, (11, 11), 12, 1), (36, (16, 17), 17, 1),
                  (30, (22, 22), 22, 1)]


def _batch(np_, arms, sca, B, seed=9, nc=8):
    torch.manual_seed(seed)
    return synth.build_sampling_batch(synth.make_pocket(11, np_, tuple(arms), sca, num_full_protein=np_ + 10), B, num_classes=nc)


def _same_forward(models, b, label):
    narrow, wide = ({k: v.clone() for k, v in _forward_hip(m, b).items()} for m in models)
    torch.cuda.synchronize()
    diff = {k: maxabs(narrow[k], wide[k]) for k in KEYS}
    print(f"hnode zero extension, forward {label}: " + ", ".join(f"{k} {v:.3g}" for k, v in diff.items()))
    assert all(bool(torch.isfinite(narrow[k]).all()) for k in KEYS)
    for k in KEYS:
        assert torch.equal(narrow[k], wide[k]), (label, k, diff[k])


@pytest.mark.parametrize("np_,arms,sca,B", FORWARD_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_forward_equals_the_zero_extended_wide_model(np_, arms, sca, B):
    b = _batch(np_, arms, sca, B)
    nl = int(b["batch_ligand"].numel()) // B
    assert (B, np_, nl) in [(1, 40, 2), (2, 21, 3), (3, 7, 5), (2, 30, 17), (1, 40, 34), (1, 36, 50), (1, 30, 66)]
    _same_forward(pair(), b, f"B={B} NP={np_} NL={nl}")


@pytest.mark.parametrize("parts", [((40, (3, 3), 4), (30, (1, 1), 2)), ((21, (1, 1), 1), (40, (6, 6), 5), (33, (4, 4), 4))],
                         ids=["40+10,30+4", "21+3,40+17,33+12"])
def test_padded_forward_equals_the_zero_extended_wide_model(parts):
    torch.manual_seed(17)
    each = [synth.build_sampling_batch(synth.make_pocket(60 + i, np_, arms, sca, num_full_protein=np_ + 20), 1)
            for i, (np_, arms, sca) in enumerate(parts)]
    _same_forward(pair(), synth.concat_sampling_batches(each), "padded " + ", ".join(f"{p[0]}+{sum(p[1]) + p[2]}" for p in parts))


# ------------------------------------------------------------------------------------ zero extension: chains
def _chain_inputs(nc=8):
    b = _batch(44, (3, 3), 6, 2, seed=2023, nc=nc)
    assert b["init_ligand_pos"].shape[0] == 2 * 12 and b["protein_pos"].shape[0] == 2 * 44
    torch.manual_seed(5)
    return b, synth.draw_step_noise(3, 24, 2 * 132, num_classes=nc)


def _same_chain(models, b, noise, drift, label, **kw):
    narrow, wide = (_sample_hip(m, b, 3, drift, noise, **kw) for m in models)
    for k in ("pos", "v", "bond"):
        assert torch.equal(narrow[k], wide[k]), (label, k)
    for k in ("pos_traj", "v_traj", "bond_traj", "bt_traj"):
        assert torch.equal(torch.stack(narrow[k]), torch.stack(wide[k])), (label, k)
    assert bool(torch.isfinite(narrow["pos"]).all())
    print(f"hnode zero extension, 3-step chain {label}: bit-identical")
    return narrow


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("drift", [None, GU.DRIFT], ids=["plain", "drift"])
def test_chain_equals_the_zero_extended_wide_model(use_graph, drift):
    b, noise = _chain_inputs()
    _same_chain(pair(), b, noise, drift, f"{'captured' if use_graph else 'eager'} {'drift' if drift else 'plain'}", use_graph=use_graph)


@pytest.mark.parametrize("over", [dict(num_blocks=2), dict(knn=48), dict(bond_net_type="pre_att", x2h_out_fc=True)],
                         ids=["num_blocks=2", "knn=48", "pre_att+out_fc"])
def test_chain_of_other_configurations_equals_the_zero_extended_wide_model(over):
    b, noise = _chain_inputs()
    _same_chain(pair(**over), b, noise, GU.DRIFT, str(over))


def test_chain_with_13_classes_noise_mean_arms_repul_and_start_step():
    """What else a wide model runs: the add_aromatic vocabulary, model_mean_type 'noise', the arms_repul drift, a resumed chain."""
    b, noise = _chain_inputs(nc=13)
    _same_chain(pair(nc=13, model_mean_type="noise"), b, noise, REPUL, "13 classes, noise, arms_repul, start_step=4", start_step=4)


def test_layer0_tables_on_and_off(monkeypatch):
    """The narrow model keeps the layer-0 tables (their ligand rows' first 640 columns): gathered rows equal the GEMMs' rows."""
    b, noise = _chain_inputs()
    m = narrow_model()
    on = _sample_hip(m, b, 3, GU.DRIFT, noise)
    assert m._packed.get("l0_tables") is not None
    monkeypatch.setenv("DD_LAYER0_TABLES", "0")
    off_model = _load(narrow_config(), {k: v.detach().cpu() for k, v in m.state_dict().items()})
    off = _sample_hip(off_model, b, 3, GU.DRIFT, noise)
    assert off_model._packed.get("l0_tables") is None
    for k in ("pos", "v", "bond"):
        assert torch.equal(on[k], off[k]), k
    assert torch.equal(torch.stack(on["bt_traj"]), torch.stack(off["bt_traj"]))
    print("hnode layer-0 tables on / off: bit-identical")


def test_sync_twoup_changes_nothing():
    b, noise = _chain_inputs()
    fb = _batch(30, (6, 6), 5, 2)
    for h_node in (False, True):
        cfg = shipped_config(h_node_in_bond_net=h_node)
        sd = synth.synthetic_state_dict(cfg, 0)
        plain, twoup = _load(cfg, sd), _load(shipped_config(h_node_in_bond_net=h_node, sync_twoup=True), sd)
        fa, fc = _forward_hip(plain, fb), _forward_hip(twoup, fb)
        assert all(torch.equal(fa[k], fc[k]) for k in KEYS)
        ra, rc = _sample_hip(plain, b, 3, GU.DRIFT, noise), _sample_hip(twoup, b, 3, GU.DRIFT, noise)
        assert all(torch.equal(ra[k], rc[k]) for k in ("pos", "v", "bond"))
    print("hnode sync_twoup True / False: bit-identical")


# ------------------------------------------------------------------------------------ harness
def test_harness_records_of_a_narrow_model():
    pocket = synth.make_pocket(31, 70, (3, 2), 4, num_full_protein=150)
    outs = []
    for m in pair():
        torch.manual_seed(5)                              # (the harness draws the initial state from the global CPU generator)
        outs.append(harness.sample_diffusion_ligand_decomp(m, pocket, num_samples=2, batch_size=2, device="cuda:0", num_steps=3, seed=11))
    recs = [harness.to_result_records(o) for o in outs]
    assert len(recs[0]) == 2 and set(recs[0][0]) == set(recs[1][0])
    assert {"pred_pos", "pred_v", "pred_pos_traj", "pred_v_traj", "decomp_mask", "pred_bond_index", "pred_bond_type"} <= set(recs[0][0])
    for a, c in zip(*recs):
        assert a["pred_pos"].shape == (9, 3) and np.isfinite(a["pred_pos"]).all()
        assert np.array_equal(a["pred_pos"], c["pred_pos"]) and np.array_equal(a["pred_v"], c["pred_v"])
        assert np.array_equal(a["pred_bond_type"], c["pred_bond_type"])


# ------------------------------------------------------------------------------------ the wide model beside it
def test_wide_model_unchanged_after_a_narrow_model_ran():
    """In the same process, after the narrow cases and through the same shape: a wide lin model built afterwards still
    reproduces forward_small (no cached chain or table leaks across the widths)."""
    g = GU.load("forward_small")
    b = GU.batch_from_npz(g)
    _forward_hip(narrow_model(), b)
    cfg = shipped_config()
    m = _load(cfg, synth.synthetic_state_dict(cfg, 0))
    out, ref = _forward_hip(m, b), _forward_hip(lin_model(0), b)
    e = max(maxabs(out[k], g["out_" + k]) for k in KEYS)
    print(f"hnode wide lin model after the narrow one: forward {e:.3g}")
    assert e < 2e-4
    assert all(torch.equal(out[k], ref[k]) for k in KEYS)
