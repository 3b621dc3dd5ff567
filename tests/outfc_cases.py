"""GPU cases of the node output MLPs (x2h_out_fc = True): the kernel alone through dd_node_out_fc against the reference formula in
float64, then the model end to end (forward, single steps, chains, graph replay, start_step resumption, ragged forward, harness,
the pre_att pair, a lin model afterwards) against fixtures from the reference itself (tools/make_outfc_golden.py).  Run by
tests/test_gpu_out_fc.py in a process of their own (see there); `pytest -m gpu tests/outfc_cases.py` runs them directly."""
import ctypes
import json

import numpy as np
import pytest
import torch

import golden_utils as GU
import stress_weights as SW
from decompdiff_amd import DecompScorePosNet3D, harness, hip_lib, packing, shipped_config, synth
from noise_param_cases import _step_case
from test_gpu_configs import _check_chain, _fixture_chain
from test_gpu_forward_ragged import PAD_LOGIT_TOL, PAD_POS_TOL, fwd, per_sample, samples
from test_gpu_parity import LOGIT_TOL, POS_TOL, _forward_hip, _sample_hip, dev, maxabs
from test_gpu_parity import model as lin_model
from test_out_fc_host import _reference_update

pytestmark = pytest.mark.gpu

_MODELS = {}
B8_STD = [1.0, 0.9, 0.8, 1.1, 1.0, 0.95, 1.05, 0.85]
KEYS = ("pred_ligand_pos", "pred_ligand_v", "pred_bond")


def _new_model(**over):
    cfg = shipped_config(x2h_out_fc=True, **over)
    m = DecompScorePosNet3D(cfg, 29, 10, 8)
    sd = m.state_dict()
    sd.update(synth.synthetic_state_dict(cfg, 0))
    m.load_state_dict(sd, strict=True)
    return m.to(dev())


def outfc_model(kind="lin"):
    if kind not in _MODELS:
        _MODELS[kind] = _new_model(bond_net_type=kind)
    return _MODELS[kind]


# ------------------------------------------------------------------------------------ the kernel alone
CFG = shipped_config(x2h_out_fc=True)
REGIMES = ("synthetic", "signed_gamma", "wide_affine", "flat_rows")
# every tile edge of the 32-row workgroups: rows no multiple of the tile with a tile across the protein / ligand and the sample
# boundary; all-protein tiles and the smallest ligand; a ligand longer than two tiles
SHAPES = [(2, 21, 5), (1, 130, 2), (3, 7, 66)]
_WEIGHTS = {}


def _flat_node_out(sd):
    """flat_rows of tests/stress_weights.py on the node-output MLPs: a zero first Linear, hence a constant LayerNorm input."""
    sd = {k: v.clone() for k, v in sd.items()}
    for k in sd:
        if ".node_output.net.0." in k:
            sd[k].zero_()
    return sd


def regime_weights(regime):
    if regime not in _WEIGHTS:
        sd = synth.synthetic_state_dict(CFG, 0)
        sd = {"synthetic": lambda s: s, "signed_gamma": SW.signed_gamma, "wide_affine": SW.wide_affine, "flat_rows": _flat_node_out}[regime](sd)
        form = packing.node_out_fc(sd, CFG)
        _WEIGHTS[regime] = (sd, torch.stack([packing.node_out_block(f) for f in form]).to(dev()))
    return _WEIGHTS[regime]


def _inputs(B, NP, NL, seed):
    g = torch.Generator().manual_seed(seed)
    N = NP + NL
    return torch.randn(B * N, 128, generator=g), torch.randn(B * NL, 128, generator=g), torch.randn(B * N, 128, generator=g)


def _run_kernel(blk, A_e, A_b, h, B, NP, NL, np_real=None, nl_real=None, in_place=False):
    d = dev()
    Ae, Ab, hh = A_e.to(d).contiguous(), A_b.to(d).contiguous(), h.to(d).contiguous()
    out = hh if in_place else torch.full_like(hh, float("nan"))
    i32 = lambda v: None if v is None else torch.tensor(v, dtype=torch.int32, device=d)
    npr, nlr = i32(np_real), i32(nl_real)
    hip_lib.check(hip_lib.load().dd_node_out_fc(hip_lib.ptr(Ae), hip_lib.ptr(Ab), hip_lib.ptr(hh), B, NP, NL, hip_lib.ptr(blk),
                                                hip_lib.ptr(npr), hip_lib.ptr(nlr), hip_lib.ptr(out), hip_lib.stream_ptr(d)),
                  "dd_node_out_fc")
    torch.cuda.synchronize()
    return out.cpu()


def _full_ab(A_b, B, NP, NL):
    """The bond aggregate on all rows: zero on protein rows."""
    full = torch.zeros(B, NP + NL, 128)
    full[:, NP:] = A_b.view(B, NL, 128)
    return full.reshape(-1, 128)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_%d+%d" % s)
def test_kernel_against_the_formula_in_float64(regime, shape):
    B, NP, NL = shape
    sd, blocks = regime_weights(regime)
    layer = 4
    p = f"refine_net.base_block.{layer}"
    A_e, A_b, h = _inputs(B, NP, NL, 10 * B + NL)
    full = _full_ab(A_b, B, NP, NL)
    want64 = _reference_update(sd, p, A_e, full, h, torch.float64)
    d32 = float((_reference_update(sd, p, A_e, full, h, torch.float32).double() - want64).abs().max())
    got = _run_kernel(blocks[layer], A_e, A_b, h, B, NP, NL)
    err = float((got.double() - want64).abs().max())
    print(f"out_fc kernel {regime} B={B} NP={NP} NL={NL}: err {err:.3g}, d32 {d32:.3g}, bound {SW.bound(d32):.3g}")
    assert bool(torch.isfinite(got).all())
    assert err < SW.bound(d32)
    if regime == "flat_rows":
        # a constant LayerNorm input gives relu(beta): every row moves by the same vector
        c = lambda k: sd[k].double()
        z = lambda n: torch.relu(c(f"{p}.{n}.node_output.net.1.bias")) @ c(f"{p}.{n}.node_output.net.3.weight").t() + c(f"{p}.{n}.node_output.net.3.bias")
        const = (z("node_layer_with_edge") + z("node_layer_with_bond")) @ c(f"{p}.lin_node.weight").t() + c(f"{p}.lin_node.bias")
        e_flat = float((got.double() - h.double() - const).abs().max())
        print(f"out_fc kernel flat_rows B={B}: |h_new - h - lin(W2 relu(beta) + b2)| {e_flat:.3g}")
        assert e_flat < 1e-5
    assert torch.equal(_run_kernel(blocks[layer], A_e, A_b, h, B, NP, NL, in_place=True), got)


def test_kernel_padded_batch_equals_per_sample_dense_calls():
    B, NP, NL = 2, 21, 5
    np_real, nl_real = [21, 9], [5, 3]
    sd, blocks = regime_weights("synthetic")
    A_e, A_b, h = _inputs(B, NP, NL, 3)
    got = _run_kernel(blocks[0], A_e, A_b, h, B, NP, NL, np_real, nl_real).view(B, NP + NL, 128)
    assert bool(torch.isfinite(got).all())                # padding rows included
    for b in range(B):
        rows = list(range(np_real[b])) + list(range(NP, NP + nl_real[b]))
        sel = lambda t: t.view(B, NP + NL, 128)[b, rows].contiguous()
        ab = A_b.view(B, NL, 128)[b, :nl_real[b]].contiguous()
        one = _run_kernel(blocks[0], sel(A_e), ab, sel(h), 1, np_real[b], nl_real[b])
        assert torch.equal(got[b, rows], one), b


# ------------------------------------------------------------------------------------ forward
def test_forward_outfc_reference_golden():
    g = GU.load("forward_outfc")
    out = _forward_hip(outfc_model(), GU.batch_from_npz(g))
    torch.cuda.synchronize()
    errs = {k: maxabs(out[k], g["out_" + k]) for k in KEYS}
    print("out_fc forward (NP=300, NL=30, B=2): " + ", ".join(f"{k} {v:.3g}" for k, v in errs.items()))
    assert errs["pred_ligand_pos"] < 2e-5 and errs["pred_ligand_v"] < 2e-4 and errs["pred_bond"] < 2e-4
    # the model without the switch computes something else: the node-output stage really is what produced these outputs
    lin = _forward_hip(lin_model(0), GU.batch_from_npz(g))
    assert maxabs(lin["pred_ligand_v"], g["out_pred_ligand_v"]) > 1e-2


def test_forward_outfc_with_pre_att_reference_golden():
    g = GU.load("forward_outfc_preatt")
    b = GU.batch_from_npz(g)
    assert b["init_ligand_pos"].shape[0] == 2 * 12 and b["protein_pos"].shape[0] == 2 * 44
    out = _forward_hip(outfc_model("pre_att"), b)
    torch.cuda.synchronize()
    errs = {k: maxabs(out[k], g["out_" + k]) for k in KEYS}
    print("out_fc + pre_att forward (NP=44, NL=12, B=2): " + ", ".join(f"{k} {v:.3g}" for k, v in errs.items()))
    assert errs["pred_ligand_pos"] < 2e-5 and errs["pred_ligand_v"] < 2e-4 and errs["pred_bond"] < 2e-4


def test_ragged_forward_outfc_equals_per_sample_forward():
    parts = samples()
    m = outfc_model()
    whole = fwd(m, synth.concat_sampling_batches(parts))
    each = per_sample(m, parts)
    torch.cuda.synchronize()
    errs = {k: maxabs(whole[k], each[k]) for k in KEYS}
    print("out_fc ragged forward: collated vs per-sample " + ", ".join(f"{k} {v:.3g}" for k, v in errs.items()))
    assert errs["pred_ligand_pos"] < PAD_POS_TOL and errs["pred_ligand_v"] < PAD_LOGIT_TOL and errs["pred_bond"] < PAD_LOGIT_TOL


# ------------------------------------------------------------------------------------ sampling
@pytest.mark.parametrize("t_start", [999, 500, 1, 0])
@pytest.mark.parametrize("tag", ["plain", "drift"])
def test_single_steps_outfc_reference_golden(t_start, tag):
    g = GU.load("steps_outfc")
    p = f"t{t_start}_{tag}_"
    b, drift, noise = _step_case(g, t_start, tag)
    r = _sample_hip(outfc_model(), b, 1, drift, noise, t_start)
    e_pos = maxabs(r["pos"], g[p + "pos"])
    e_lp = max(maxabs(r["vt_traj"][0], g[p + "log_v_prob"]), maxabs(r["bt_traj"][0], g[p + "log_b_prob"]),
               maxabs(r["v0_traj"][0], g[p + "log_v_recon"]))
    nv = int((r["v"].cpu() != torch.from_numpy(g[p + "v"])).sum())
    nb = int((r["bond"].cpu() != torch.from_numpy(g[p + "bond"])).sum())
    print(f"out_fc step t={t_start} {tag}: pos {e_pos:.3g} log-probs {e_lp:.3g} v-mismatch {nv} bond-mismatch {nb}")
    assert e_pos < POS_TOL and e_lp < LOGIT_TOL
    assert nv == 0 and nb == 0


@pytest.mark.parametrize("name,std_scale", [("traj3_outfc_b8_plain", None), ("traj3_outfc_b8_drift", B8_STD)])
def test_sampling_b8_outfc_reference_golden(name, std_scale):
    g, b, noise = _fixture_chain(name, synth.make_pocket_small(8), 8, std_scale)
    assert b["init_ligand_pos"].shape[0] == 8 * 30 and b["protein_pos"].shape[0] == 8 * 300
    r = _sample_hip(outfc_model(), b, 3, json.loads(str(g["drift"])), noise)
    _check_chain(f"out_fc ({name}: NP=300, NL=30, B=8)", r, g, 3)


def test_sampling_20_steps_outfc_reference_golden():
    g, b, noise = _fixture_chain("traj20_outfc", synth.make_pocket_small(2), 2, [1.0, 0.85])
    r = _sample_hip(outfc_model(), b, 20, json.loads(str(g["drift"])), noise)
    _check_chain("out_fc (traj20_outfc: 20 steps, B=2, drift)", r, g, 20)


def test_outfc_resume_from_the_reference_state_with_start_step():
    """The last 12 steps of traj20_outfc restarted with start_step = 8 from the reference's own state after 8 steps."""
    g, b, noise = _fixture_chain("traj20_outfc", synth.make_pocket_small(2), 2, [1.0, 0.85])
    bb = dict(b)
    bb["init_ligand_pos"] = torch.from_numpy(g["traj_pos"][7].astype(np.float32))
    bb["init_ligand_v"] = torch.from_numpy(g["traj_v"][7].astype(np.int64))
    bb["init_ligand_fc_bond_type"] = torch.from_numpy(g["traj_bond"][7].astype(np.int64))
    r = _sample_hip(outfc_model(), bb, 12, json.loads(str(g["drift"])), {k: v[8:] for k, v in noise.items()}, start_step=8)
    err = maxabs(r["pos"], g["out_pos"])
    print(f"out_fc: steps 8..19 resumed from the reference's step-8 state: final pos err {err:.3g}")
    assert err < POS_TOL
    assert np.array_equal(r["v"].cpu().numpy(), g["out_v"]) and np.array_equal(r["bond"].cpu().numpy(), g["out_bond"])


def test_outfc_graph_replay_equals_eager_launches():
    g, b, noise = _fixture_chain("traj20_outfc", synth.make_pocket_small(2), 2, [1.0, 0.85])
    n5 = {k: v[:5] for k, v in noise.items()}
    drift = json.loads(str(g["drift"]))
    r1 = _sample_hip(outfc_model(), b, 5, drift, n5, use_graph=True)
    r2 = _sample_hip(outfc_model(), b, 5, drift, n5, use_graph=False)
    for k in ("pos", "v", "bond"):
        assert torch.equal(r1[k], r2[k]), k
    assert torch.equal(torch.stack(r1["pos_traj"]), torch.stack(r2["pos_traj"]))
    assert torch.equal(torch.stack(r1["bt_traj"]), torch.stack(r2["bt_traj"]))
    assert maxabs(torch.stack(r1["pos_traj"]), g["traj_pos"][:5]) < POS_TOL


def test_outfc_harness_runs_and_matches_the_model():
    pocket = synth.make_pocket_small(5)
    out = harness.sample_diffusion_ligand_decomp(outfc_model(), pocket, num_samples=2, batch_size=2, device="cuda:0", num_steps=3,
                                                 seed=11)
    assert len(out["pred_pos"]) == 2 and all(np.isfinite(p).all() for p in out["pred_pos"])
    assert all(t.shape[0] == 3 for t in out["pred_b_traj"])


# ------------------------------------------------------------------------------------ the lin model beside it
def test_lin_model_unchanged_after_outfc_ran():
    """In the same process, after the out_fc cases: a lin model without the switch, built afterwards, still reproduces
    forward_small exactly as before (the chain-cache key separates the two)."""
    outfc_model()
    g = GU.load("forward_small")
    b = GU.batch_from_npz(g)
    _forward_hip(outfc_model(), b)                        # the same shape through the out_fc model first
    cfg = shipped_config()
    m = DecompScorePosNet3D(cfg, 29, 10, 8)
    sd = m.state_dict()
    sd.update(synth.synthetic_state_dict(cfg, 0))
    m.load_state_dict(sd, strict=True)
    out = _forward_hip(m.to(dev()), b)
    ref = _forward_hip(lin_model(0), b)
    e = max(maxabs(out[k], g["out_" + k]) for k in KEYS)
    print(f"lin model after out_fc: forward {e:.3g}")
    assert e < 2e-4
    assert all(torch.equal(out[k], ref[k]) for k in KEYS)
