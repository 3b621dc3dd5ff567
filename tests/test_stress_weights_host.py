"""Host side (no GPU) of the weight regimes of tests/stress_weights.py: each transform does what its name says, the model
loads it strictly, the kernel-form packing stays finite on it, the sharp regimes really make the softmaxes selective (measured
with the float64 oracle), and the reference-only conditions of the GPU cases hold: at every (regime, shape) the GPU suite runs,
the fp32 oracle's distance d32 to the float64 oracle is printed and is small enough to judge a kernel by (stress_weights.bound).
Nothing here reads a kernel's output.  Run with -s to see the figures."""
import pytest
import torch

import stress_steps as ST
import stress_weights as SW
from decompdiff_amd import DecompScorePosNet3D, packing, shipped_config, synth
from oracle import model as OM

CFG = shipped_config()
BASE = synth.synthetic_state_dict(CFG, 0)


def _sd(regime):
    return SW.regime_state_dict(regime, CFG)


@pytest.mark.parametrize("regime", SW.REGIMES)
def test_regime_loads_strictly_and_packs_finite(regime):
    sd = _sd(regime)
    assert set(sd) == set(BASE) and all(sd[k].shape == BASE[k].shape and sd[k].dtype == torch.float32 for k in sd)
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
    m = DecompScorePosNet3D(CFG, 29, 10, 8)
    full = m.state_dict()
    full.update(sd)
    m.load_state_dict(full, strict=True)
    arena, _, named = packing.pack_model(sd, CFG, kernel_form=True)
    assert bool(torch.isfinite(arena).all()) and all(bool(torch.isfinite(v).all()) for v in named.values())
    sd2 = _sd(regime)
    assert all(torch.equal(sd[k], sd2[k]) for k in sd), "the transform is deterministic"


@pytest.mark.parametrize("regime", ["signed_gamma", "signed_sharp"])
def test_signed_gamma_counts(regime):
    sd = _sd(regime)
    lns = SW.layer_norms(sd)
    assert len(lns) == 1 + 15 * CFG.num_layers                 # edge_pred_layer + (k, v, q) of five attention sub-layers per layer
    assert all(float(BASE[k].min()) > 0 for k in lns), "the synthetic gammas are all positive"
    for k in lns:
        g = sd[k]
        assert int((g < 0).sum()) == SW.N_NEGATIVE and int((g == 0).sum()) == SW.N_ZERO, k
        keep = g > 0
        assert torch.equal(g[keep], BASE[k][keep]) and torch.equal(g[g < 0], -BASE[k][g < 0])
    others = [k for k in sd if k not in lns and not (regime == "signed_sharp" and ".net.3." in k)]
    assert all(torch.equal(sd[k], BASE[k]) for k in others)


def test_wide_affine_spread():
    sd = _sd("wide_affine")
    for k in SW.layer_norms(sd):
        g, beta, beta0 = sd[k], sd[k[:-6] + "bias"], BASE[k[:-6] + "bias"]
        assert int((g == SW.TINY_GAMMA).sum()) == SW.N_TINY and float(g.min()) > 0
        assert float(g.max() / g.min()) > 1e3                  # columns spanning orders of magnitude
        scaled = beta != beta0
        assert int(scaled.sum()) == 128 // 3 and torch.allclose(beta[scaled], beta0[scaled] * 10.0)
        assert float((beta / g).abs().max()) > 5.0             # (synthetic: below 1) a large beta' = beta / |gamma| reaches the kernels


@pytest.mark.parametrize("regime,factor", [("sharp3", 3.0), ("sharp6", 6.0)])
def test_sharp_scales_query_and_key_mlps(regime, factor):
    sd = _sd(regime)
    hit = [k for k in sd if not torch.equal(sd[k], BASE[k])]
    assert len(hit) == 2 * 10 * CFG.num_layers                 # weight + bias of q and k of five attention sub-layers per layer
    assert all(".net.3." in k and any(t in k for t in (".hq_func.", ".hk_func.", ".xq_func.", ".xk_func.")) for k in hit)
    assert all(torch.equal(sd[k], BASE[k] * factor) for k in hit)


def test_flat_rows_zeroes_one_key_and_one_value_mlp_per_layer():
    sd = _sd("flat_rows")
    pairs = SW.flat_mlps(CFG)
    assert len(pairs) == CFG.num_layers
    zeroed = {n + s for p in pairs for n in p for s in (".net.0.weight", ".net.0.bias")}
    for k in sd:
        if k in zeroed:
            assert float(sd[k].abs().max()) == 0.0
        else:
            assert torch.equal(sd[k], BASE[k])
    # the LayerNorm input of such an MLP is exactly constant (0): its output is relu(beta), whatever the edge
    name = pairs[0][0]
    y = OM.mlp({k: v.double() for k, v in sd.items()}, name, torch.randn(7, sd[name + ".net.0.weight"].size(1)).double())
    want = OM.linear({k: v.double() for k, v in sd.items()}, name + ".net.3", torch.relu(sd[name + ".net.1.bias"].double()))
    assert float((y - want).abs().max()) < 1e-12


def test_hot_heads_scales_the_class_heads():
    sd = _sd("hot_heads")
    hit = sorted(k for k in sd if not torch.equal(sd[k], BASE[k]))
    assert hit == ["bond_inference.2.bias", "bond_inference.2.weight", "v_inference.2.bias", "v_inference.2.weight"]
    assert all(torch.equal(sd[k], BASE[k] * SW.HOT_FACTOR) for k in hit)


def _attention_stats(regime, b):
    stats = []
    SW.oracle_forward(_sd(regime), CFG, b, torch.float64, stats)
    return max(s[0] for s in stats), max(s[1] for s in stats)


def test_sharp_regimes_make_the_softmaxes_selective():
    """Score range and mean largest attention weight over all attention calls of a float64 forward (60 + 12 atoms, B = 2).  The
    transform multiplies q and k by f, i.e. every score by f^2 at equal features: asserted at 2/3 of that (the features
    downstream of a sharper attention differ), and the largest mean attention weight at 3x / 5x the synthetic weights' value."""
    b = SW.pocket_batch(11, 60, (4, 4), 4, 2)
    s0, w0 = _attention_stats("synthetic", b)
    print(f"\nsynthetic: max |score| {s0:.3g}, largest mean top attention weight {w0:.3g}")
    assert s0 < 5.0 and w0 < 0.25, "the synthetic weights' softmaxes are nearly flat"
    for regime, f, wf in (("sharp3", 3.0, 3.0), ("sharp6", 6.0, 5.0), ("signed_sharp", 3.0, 3.0)):
        s, w = _attention_stats(regime, b)
        print(f"{regime}: max |score| {s:.3g} ({s / s0:.1f}x), largest mean top attention weight {w:.3g} ({w / w0:.1f}x)")
        assert s > (2.0 / 3.0) * f * f * s0 and w > wf * w0


def test_float64_oracle_follows_fp32_inputs_and_graph():
    """The float64 mode casts nothing in fp32 (same tensors out as the plain call), returns float64, and uses the fp32 graph."""
    b = SW.SHAPES["tiny_20+3_B2"][0]()
    args = (b["protein_pos"], b["protein_v"], b["batch_protein"], b["init_ligand_pos"], b["init_ligand_v"], b["ligand_v_aux"],
            b["batch_ligand"], b["ligand_fc_bond_index"], b["init_ligand_fc_bond_type"])
    with torch.no_grad():
        plain = OM.forward(BASE, CFG, *args)
        same = OM.forward(BASE, CFG, *args, dtype=torch.float32)
    assert all(torch.equal(plain[k], same[k]) for k in plain)
    w64, w32, d32 = SW.both_oracles(BASE, CFG, b)              # (asserts equal edges and the dtypes)
    assert all(torch.equal(plain[k], w32[k]) for k in plain)
    assert 0 < max(d32.values()) < 1e-4


@pytest.mark.parametrize("regime,shape", sorted(SW.cases()))
def test_fp32_oracle_distance_gives_a_usable_bound(regime, shape):
    """d32 per output at a shape the GPU cases use; bound() raises where a regime is too ill-conditioned to judge (> 1e-3)."""
    b = SW.SHAPES[shape][0]()
    if shape.startswith("padded"):
        w64, _, d32 = SW.step_t0_reference(_sd(regime), CFG, b)
    else:
        w64, _, d32 = SW.both_oracles(_sd(regime), CFG, b)
    assert all(bool(torch.isfinite(v).all()) for v in w64.values())
    bounds = {k: SW.bound(v) for k, v in d32.items()}
    print(f"\nd32 {regime} {shape}: " + " ".join(f"{k}:{d32[k]:.2g}(bound {bounds[k]:.2g})" for k in d32))
    # (bound() has asserted d32 <= 1e-3.)  Only the two regimes built to be ill-conditioned may leave the flat tolerance
    if regime not in ("sharp6", "hot_heads"):
        assert all(v == SW.TOL for v in bounds.values()), bounds


@pytest.mark.parametrize("nc,prior,nl", ST.step_cases())
def test_reverse_step_cases_have_usable_bounds_and_no_near_tie_draw(nc, prior, nl):
    """The reference-only conditions of the dd_reverse_step cases: d32 = the fp32 torch evaluation of the transition formulas
    against float64 gives the bound of every compared tensor (flat 1e-4 at logits x 1 and x 30; at x 1000 one fp32 ulp of a logit is
    6e-5 - 2.4e-4 and log_softmax cannot hold it), and at the seed each transition uses no draw's two best log-prob + Gumbel
    scores lie within twice that bound (never less than 2e-4), so every sampled type is compared on the GPU."""
    m = ST.build_model(nc, prior)
    tab = ST.tables(m)
    b, offset, xt = ST.batch_for(nc, nl)
    near = 0
    for t, scale, base_seed in ST.sub_cases(nc, prior, nl):
        p = ST.prepared(tab, b, xt, offset, nc, t, scale, base_seed)
        thr = {"v": max(2e-4, 2 * p["bounds"]["log_vt"]), "b": max(2e-4, 2 * p["bounds"]["log_bt"])}
        n = int((p["w64"]["v_gap"] <= thr["v"]).sum()) + int((p["w64"]["b_gap"] <= thr["b"]).sum())
        near += n
        print(f"\nstep nc={nc} prior={prior} NL={nl} t={t} scale={scale:g} seed={p['seed']}: near-tie draws {n} (smallest gaps "
              f"{p['gaps']['v']:.2g} / {p['gaps']['b']:.2g}); d32 " + " ".join(f"{k}:{p['d32'][k]:.2g}(bound {p['bounds'][k]:.2g})" for k in ST.COMPARED))
        assert all(bool(torch.isfinite(p["w64"][k]).all()) for k in ST.COMPARED)
        if scale <= 30.0:
            assert all(v == SW.TOL for v in p["bounds"].values()), p["bounds"]
        assert p["bounds"]["log_vt"] == SW.TOL and p["bounds"]["lig_pos"] == SW.TOL       # (the posteriors saturate: only log_softmax itself grows)
        if t == 0:                                 # the reference itself: no eps contribution at t = 0
            other = dict(p["inp"], eps=p["inp"]["eps"] * -3.0 + 1.0)
            assert torch.equal(ST.reference_step(tab, b, xt, offset, other, 0, torch.float64)["lig_pos"], p["w64"]["lig_pos"])
        # the edges are really in the inputs
        assert int((p["inp"]["u_v"] == 0).sum()) > 0 and int((p["inp"]["u_b"] == ST.U_MAX).sum()) > 0 and ST.U_MAX < 1.0
    print(f"step nc={nc} prior={prior} NL={nl}: zero near-tie draws" if near == 0 else f"NEAR TIES: {near}")
    assert near == 0
    if prior == "zero_class":
        assert float(tab["v"]["prior_probs"].reshape(-1)[1]) < -69.0 and float(tab["b"]["prior_probs"].reshape(-1)[1]) < -69.0
