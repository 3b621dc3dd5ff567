"""Edge cases of one reverse transition (dd_reverse_step) on host-made tensors, and its float64 restatement: the transition
math of oracle/diffusion.py (q_v_posterior, log_add_exp, gumbel_argmax, the Gaussian posterior with the t == 0 mask) evaluated
in float64 -- and, for the bound, in fp32 -- from the fp32 schedule tables the kernel reads.  A plain helper module (no tests):
tests/test_stress_weights_host.py checks the reference-only conditions (d32 of the log-probabilities, no near-tie draw),
tests/stress_cases.py runs the kernel."""
import numpy as np
import torch

import stress_weights as SW
from decompdiff_amd import DecompScorePosNet3D, shipped_config, synth
from oracle import diffusion as OD

CLASS_COUNTS = (8, 13, 23)
PRIORS = ("uniform", "skewed", "zero_class")
LIGANDS = {30: (300, (8, 8), 14), 66: (40, (22, 22), 22)}       # NL -> make_pocket(num_protein, arms, scaffold)
T_STARTS = (999, 500, 1, 0)
SCALES = (1.0, 30.0, 1000.0)
B = 2
U_MAX = float(np.float32(1.0) - np.float32(2.0 ** -24))         # the largest float below 1


def step_cases():
    return [(nc, prior, nl) for nc in CLASS_COUNTS for prior in PRIORS for nl in LIGANDS]


def class_prior(kind, n):
    """None (uniform), class probabilities falling by a factor 30 over the classes, or the same with class 1 at exactly 0."""
    if kind == "uniform":
        return None
    p = np.exp(-np.log(30.0) * np.arange(n) / (n - 1))
    if kind == "zero_class":
        p[1] = 0.0
    return p / p.sum()


def build_model(nc, prior):
    cfg = shipped_config()
    m = DecompScorePosNet3D(cfg, 29, nc + 2, nc, prior_atom_types=class_prior(prior, nc), prior_bond_types=class_prior(prior, 5))
    sd = m.state_dict()
    sd.update(synth.synthetic_state_dict(cfg, 0, ligand_atom_feature_dim=nc + 2, num_classes=nc))
    m.load_state_dict(sd, strict=True)
    return m


def tables(m):
    """The fp32 tables the kernel reads (dd_sampler.tab_pos / tab_v / tab_b), from the model's own buffers."""
    cat = lambda tr: {k: getattr(tr, k).detach().cpu().float() for k in
                      ("log_alphas_v", "log_one_minus_alphas_v", "log_alphas_cumprod_v", "log_one_minus_alphas_cumprod_v", "prior_probs")}
    return dict(pos=m.position_step_table().detach().cpu().float().view(3, -1), v=cat(m.atom_type_trans), b=cat(m.bond_type_trans))


def batch_for(nc, nl):
    np_, arms, sca = LIGANDS[nl]
    pocket = synth.make_pocket(11, np_, arms, sca, num_full_protein=np_ + 10)
    torch.manual_seed(13)
    b = synth.build_sampling_batch(pocket, B, num_classes=nc, per_sample_std_scale=[1.0, 0.8])
    NP = pocket.num_protein_atoms
    tot = torch.zeros(B, 3).index_add_(0, torch.arange(B).repeat_interleave(NP), b["protein_pos"])       # (model._prepare_chain)
    offset = tot / float(NP)
    return b, offset, b["init_ligand_pos"] - offset[b["batch_ligand"]]


def draw_inputs(nc, n_lig, n_bond, scale, seed):
    """Logits N(0,1) x scale with a few entries pushed a further 100 apart, x0 of ordinary size, and the step's noise with
    uniforms of exactly 0 and of the largest float below 1 among them."""
    g = torch.Generator().manual_seed(seed)
    lv, lb = torch.randn(n_lig, nc, generator=g) * scale, torch.randn(n_bond, 5, generator=g) * scale
    lv[0::7, 0] += 100.0
    lv[3::7, nc - 1] -= 100.0
    lb[0::11, 4] += 100.0
    lb[5::11, 0] -= 100.0
    x0 = torch.randn(n_lig, 3, generator=g) * 3.0
    u_v, u_b = torch.rand(n_lig, nc, generator=g), torch.rand(n_bond, 5, generator=g)
    u_v[1::5, 2], u_v[2::5, 1], u_v[4::5, nc - 1] = 0.0, U_MAX, U_MAX
    u_b[1::9, 0], u_b[2::9, 3], u_b[4::9, 1] = 0.0, U_MAX, 0.0
    return dict(logits_v=lv, logits_b=lb, x0=x0, u_v=u_v, u_b=u_b, eps=torch.randn(n_lig, 3, generator=g))


def _gumbel(u):
    return -torch.log(-torch.log(u + 1e-30) + 1e-30)                      # oracle.diffusion.gumbel_argmax


def reference_step(tab, b, xt, offset, inp, t, dtype):
    """One reverse transition in `dtype` from fp32 inputs and tables; also the two best log-prob + Gumbel scores' gap per draw."""
    c = lambda x: x.to(dtype)
    n_graphs = int(b["batch_ligand"].max()) + 1
    tt = torch.full((n_graphs,), int(t), dtype=torch.long)
    out = {}
    for name, tk, logits, cur, batch, u in (("v", "v", inp["logits_v"], b["init_ligand_v"], b["batch_ligand"], inp["u_v"]),
                                            ("b", "b", inp["logits_b"], b["init_ligand_fc_bond_type"], b["batch_ligand_bond"], inp["u_b"])):
        tb = {k: c(v) for k, v in tab[tk].items()}
        log0 = torch.log_softmax(c(logits), -1)
        log_cur = c(OD.index_to_log_onehot(cur, logits.size(-1)))
        logp = OD.q_v_posterior(tb, log0, log_cur, tt, batch)
        score = _gumbel(c(u)) + logp
        top = score.topk(2, -1).values
        out.update({f"log_{name}0": log0, f"log_{name}t": logp, f"{name}_next": score.argmax(-1), f"{name}_gap": top[:, 0] - top[:, 1]})
    c0, ct, logvar = (c(tab["pos"][i, int(t)]) for i in range(3))
    mean = c0 * c(inp["x0"]) + ct * c(xt)
    std = c(b["prior_stds"])[b["ligand_decomp_batch"]]
    out["lig_pos"] = mean + (0.0 if int(t) == 0 else 1.0) * torch.exp(0.5 * logvar) * c(inp["eps"]) * std
    out["traj_pos"] = out["lig_pos"] + c(offset)[b["batch_ligand"]]
    return out


COMPARED = ("log_v0", "log_vt", "log_bt", "lig_pos", "traj_pos")


def prepared(tab, b, xt, offset, nc, t, scale, base_seed):
    """Inputs of one sub-case with the first seed >= base_seed at which no draw is a near tie, its float64 reference, d32 and
    bounds.  A draw whose two best scores lie within twice its log-probabilities' bound (at least 2e-4) could flip between two
    correct implementations; such seeds are passed over, so that every sampled type is compared.  Reads no kernel output."""
    n_lig, n_bond = b["init_ligand_pos"].size(0), b["init_ligand_fc_bond_type"].size(0)
    for seed in range(base_seed, base_seed + 200):
        inp = draw_inputs(nc, n_lig, n_bond, scale, seed)
        w64 = reference_step(tab, b, xt, offset, inp, t, torch.float64)
        w32 = reference_step(tab, b, xt, offset, inp, t, torch.float32)
        d32 = {k: float((w64[k] - w32[k].double()).abs().max()) for k in COMPARED}
        bounds = {k: SW.bound(d32[k]) for k in COMPARED}
        gaps = {"v": float(w64["v_gap"].min()), "b": float(w64["b_gap"].min())}
        if gaps["v"] > 2 * bounds["log_vt"] and gaps["b"] > 2 * bounds["log_bt"]:
            return dict(seed=seed, inp=inp, w64=w64, d32=d32, bounds=bounds, gaps=gaps)
    raise AssertionError("no seed without a near-tie draw")


def sub_cases(nc, prior, nl):
    """(t, scale, base seed) of the 12 transitions run per case."""
    k = 1000 * (CLASS_COUNTS.index(nc) * 6 + PRIORS.index(prior) * 2 + list(LIGANDS).index(nl))
    return [(t, s, k + 20 * (i * 3 + j)) for i, t in enumerate(T_STARTS) for j, s in enumerate(SCALES)]
