"""Named weight regimes: deterministic transforms of the synthetic weights (synth.synthetic_state_dict) that leave the
distribution every other test runs at -- LayerNorm gammas of either sign, of exactly zero and of widely different sizes, large
betas, selective softmaxes, constant LayerNorm rows, saturated class logits.  Each returns a complete state dict of the
learnable tensors: the model loads it with strict=True over its own buffers, the oracle consumes it unchanged.  A plain helper
module (no tests): tests/test_stress_weights_host.py checks the transforms, tests/stress_cases.py runs the kernels on them."""
import zlib

import numpy as np
import torch

from decompdiff_amd import shipped_config, synth
from oracle import diffusion as OD
from oracle import model as OM
from oracle import ops as OO

REGIMES = ("signed_gamma", "wide_affine", "sharp3", "sharp6", "flat_rows", "hot_heads", "signed_sharp")
N_NEGATIVE, N_ZERO = 40, 5                      # of the 128 channels of every LayerNorm (signed_gamma)
N_TINY, TINY_GAMMA = 4, 1e-3                    # wide_affine
HOT_FACTOR = 30.0
_QK = (".hq_func.", ".hk_func.", ".xq_func.", ".xk_func.")
_KEY_MLPS = ("node_layer_with_edge.hk_func", "node_layer_with_bond.hk_func", "bond_layer.hk_func",
             "pos_layer_with_edge.xk_func", "pos_layer_with_bond.xk_func")
_VALUE_MLPS = ("node_layer_with_edge.hv_func", "node_layer_with_bond.hv_func", "bond_layer.hv_func",
               "pos_layer_with_edge.xv_func", "pos_layer_with_bond.xv_func")


def _rng(seed, key, salt):
    return np.random.default_rng([int(seed), zlib.crc32(key.encode("utf-8")), int(salt)])


def layer_norms(sd):
    """Names of all LayerNorm gammas: the attention MLPs k / v / q of every layer and refine_net.edge_pred_layer."""
    return sorted(k for k in sd if k.endswith(".net.1.weight"))


def signed_gamma(sd, seed=0):
    sd = {k: v.clone() for k, v in sd.items()}
    for k in layer_norms(sd):
        perm = torch.from_numpy(_rng(seed, k, 1).permutation(sd[k].numel()))
        g = sd[k]
        g[perm[:N_NEGATIVE]] = -g[perm[:N_NEGATIVE]].abs()
        g[perm[N_NEGATIVE:N_NEGATIVE + N_ZERO]] = 0.0
    return sd


def wide_affine(sd, seed=0):
    sd = {k: v.clone() for k, v in sd.items()}
    for k in layer_norms(sd):
        r = _rng(seed, k, 2)
        n = sd[k].numel()
        g = sd[k].double() * torch.from_numpy(np.exp(r.standard_normal(n)))
        perm = torch.from_numpy(r.permutation(n))
        g[perm[:N_TINY]] = TINY_GAMMA
        beta = sd[k[:-len("weight")] + "bias"]
        beta[perm[N_TINY:N_TINY + n // 3]] *= 10.0
        sd[k] = g.float()
    return sd


def sharp(sd, factor):
    """Second Linear (weight and bias) of every query and key MLP times `factor`: every attention score times factor^2."""
    sd = {k: v.clone() for k, v in sd.items()}
    for k in sd:
        if ".net.3." in k and any(t in k for t in _QK):
            sd[k] *= float(factor)
    return sd


def flat_mlps(cfg):
    """The key and the value MLP of each layer whose first Linear flat_rows zeroes (every kind is hit over the 9 layers)."""
    return [(f"refine_net.base_block.{l}.{_KEY_MLPS[l % 5]}", f"refine_net.base_block.{l}.{_VALUE_MLPS[(l + 2) % 5]}")
            for l in range(cfg.num_layers)]


def flat_rows(sd, cfg):
    sd = {k: v.clone() for k, v in sd.items()}
    for pair in flat_mlps(cfg):
        for name in pair:
            sd[name + ".net.0.weight"].zero_()
            sd[name + ".net.0.bias"].zero_()
    return sd


def hot_heads(sd):
    sd = {k: v.clone() for k, v in sd.items()}
    for k in ("v_inference.2.weight", "v_inference.2.bias", "bond_inference.2.weight", "bond_inference.2.bias"):
        sd[k] *= HOT_FACTOR
    return sd


def regime_state_dict(name, cfg=None, seed=0):
    cfg = cfg or shipped_config()
    sd = synth.synthetic_state_dict(cfg, seed)
    if name == "synthetic":
        return sd
    if name == "signed_gamma":
        return signed_gamma(sd, seed)
    if name == "wide_affine":
        return wide_affine(sd, seed)
    if name == "sharp3":
        return sharp(sd, 3.0)
    if name == "sharp6":
        return sharp(sd, 6.0)
    if name == "flat_rows":
        return flat_rows(sd, cfg)
    if name == "hot_heads":
        return hot_heads(sd)
    if name == "signed_sharp":
        return sharp(signed_gamma(sd, seed), 3.0)
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ shapes and oracles
def lattice_batch():
    """Degenerate geometry: 12 ligand atoms on an integer lattice next to a 40-atom pocket (exactly collinear triples -- angles 0
    and pi --, many equal distances -- kNN ties) with atoms 0 and 1 at the same position (distance 0, atan2(0, 0))."""
    pocket = synth.make_pocket(17, 40, (4, 4), 4, num_full_protein=60)
    torch.manual_seed(4)
    b = synth.build_sampling_batch(pocket, 2)
    c = torch.from_numpy(pocket.prior_centers[-1]).round()
    grid = torch.tensor([[i, j, k] for i in range(3) for j in range(2) for k in range(2)], dtype=torch.float32)   # 12 points
    grid[1] = grid[0]
    b["init_ligand_pos"] = (c + grid).repeat(2, 1).contiguous()
    return b


def hetero_batch():
    """Two ligand sizes (9 and 37 atoms) and two pocket sizes in one batch: the model runs it as one padded dense launch."""
    torch.manual_seed(4)
    parts = []
    for i, (nl, np_) in enumerate(((9, 150), (37, 260))):
        arm = max(2, nl // 4)
        p = synth.make_pocket(seed=300 + i, num_protein=np_, arm_atoms=(arm, arm), scaffold_atoms=nl - 2 * arm, num_full_protein=np_ + 150)
        parts.append(synth.build_sampling_batch(p, 1))
    return synth.concat_sampling_batches(parts)


def pocket_batch(seed, np_, arms, sca, B):
    pocket = synth.make_pocket(seed, np_, arms, sca, num_full_protein=np_ + 10)
    torch.manual_seed(9)
    return synth.build_sampling_batch(pocket, B)


# name -> (builder, regimes that run on it)
SHAPES = {
    "bench_300+30_B2": (lambda: pocket_batch(11, 300, (8, 8), 14, 2), REGIMES),
    "tiny_20+3_B2": (lambda: pocket_batch(11, 20, (1, 1), 1, 2), REGIMES),
    "nl34_60+34": (lambda: pocket_batch(11, 60, (11, 11), 12, 1), ("signed_sharp", "sharp6")),
    "nl66_40+66": (lambda: pocket_batch(11, 40, (22, 22), 22, 1), ("signed_sharp", "sharp6")),
    "padded_9+37": (hetero_batch, ("signed_sharp",)),
    "lattice_40+12_B2": (lattice_batch, ("synthetic", "signed_sharp")),
}


def cases():
    return [(r, s) for s, (_, regs) in SHAPES.items() for r in regs]


def oracle_forward(sd, cfg, b, dtype, stats=None):
    """(preds, trace) of the oracle in `dtype` (torch.float32: the suite's reference as it is; torch.float64: the yardstick)."""
    trace = []
    with torch.no_grad():
        preds = OM.forward(sd, cfg, b["protein_pos"], b["protein_v"], b["batch_protein"], b["init_ligand_pos"], b["init_ligand_v"],
                           b["ligand_v_aux"], b["batch_ligand"], b["ligand_fc_bond_index"], b["init_ligand_fc_bond_type"],
                           trace=trace, dtype=None if dtype == torch.float32 else dtype, stats=stats)
    return preds, trace


OUTPUTS = ("pred_ligand_pos", "pred_ligand_v", "pred_bond")
TRACED = ("h", "h_bond", "x", "e_w")
TOL = 1e-4                     # POS_TOL = LOGIT_TOL of the GPU suite
D32_FLAT, D32_MAX = 2.5e-5, 1e-3


def both_oracles(sd, cfg, b, stats=None):
    """fp64 and fp32 oracle on one input -> (want64: outputs + final h / h_bond / x and e_w, want32 likewise, d32 per tensor).
    Asserts that both runs saw the same edges."""
    p64, t64 = oracle_forward(sd, cfg, b, torch.float64, stats)
    p32, t32 = oracle_forward(sd, cfg, b, torch.float32)
    assert torch.equal(t64[0]["edge_index"], t32[0]["edge_index"]), "the fp64 run must use the fp32 kNN graph"
    assert all(v.dtype == torch.float64 for v in p64.values()) and all(v.dtype == torch.float32 for v in p32.values())
    w64 = dict(p64, h=t64[-1]["h"], h_bond=t64[-1]["h_bond"], x=t64[-1]["x"], e_w=t64[0]["e_w"], edge_index=t64[0]["edge_index"])
    w32 = dict(p32, h=t32[-1]["h"], h_bond=t32[-1]["h_bond"], x=t32[-1]["x"], e_w=t32[0]["e_w"], edge_index=t32[0]["edge_index"])
    d32 = {k: float((w64[k] - w32[k].double()).abs().max()) for k in OUTPUTS + TRACED}
    return w64, w32, d32


def step_t0_reference(sd, cfg, b):
    """One reverse step at t = 0 of a (possibly ragged) batch, in float64 and in fp32: the centred forward, the Gaussian
    posterior mean (no noise at t = 0) moved back by the protein centroid, log_softmax of the atom logits and the bond
    posterior, from the fp32 schedule tables -> (want64, want32, d32) over pos / log_v0 / log_bt."""
    offset = OO.scatter_mean(b["protein_pos"], b["batch_protein"], dim=0)             # (an fp32 input transformation on both sides)
    cb = dict(b, protein_pos=b["protein_pos"] - offset[b["batch_protein"]], init_ligand_pos=b["init_ligand_pos"] - offset[b["batch_ligand"]])
    pt, bt = OD.position_tables(cfg), OD.categorical_tables(cfg, cfg.num_bond_classes)
    t = torch.zeros(int(b["batch_protein"].max()) + 1, dtype=torch.long)
    res = {}
    for dtype in (torch.float64, torch.float32):
        preds, _ = oracle_forward(sd, cfg, cb, dtype)
        mean = pt["posterior_mean_c0_coef"][0].to(dtype) * preds["pred_ligand_pos"] + \
            pt["posterior_mean_ct_coef"][0].to(dtype) * cb["init_ligand_pos"].to(dtype)
        tab = {k: v.to(dtype) for k, v in bt.items()}
        log_b = OD.index_to_log_onehot(b["init_ligand_fc_bond_type"], cfg.num_bond_classes).to(dtype)
        res[dtype] = dict(pos=mean + offset[b["batch_ligand"]].to(dtype), log_v0=torch.log_softmax(preds["pred_ligand_v"], -1),
                          log_bt=OD.q_v_posterior(tab, torch.log_softmax(preds["pred_bond"], -1), log_b, t, b["batch_ligand_bond"]))
    w64, w32 = res[torch.float64], res[torch.float32]
    return w64, w32, {k: float((w64[k] - w32[k].double()).abs().max()) for k in w64}


def bound(d32):
    """Section 'bounds' of the stress tests: the flat project tolerance where the fp32 oracle itself is within a quarter of it of
    the fp64 one, else twice the fp32 oracle's own distance (an fp32 implementation with another summation order may lose
    twice what the reference's fp32 arithmetic loses on that input); a regime beyond 1e-3 is too ill-conditioned to judge."""
    assert d32 <= D32_MAX, f"fp32 oracle is {d32:.3g} from fp64: tame the regime"
    return TOL if d32 <= D32_FLAT else max(TOL, 2.0 * d32)
