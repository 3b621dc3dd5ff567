"""Fixtures of the num_blocks > 1 tests: one place for the configurations, pockets and seeds that tests/blocks_cases.py (GPU)
runs and tests/test_blocks_host.py (CPU) vets.

A refine net with several blocks rebuilds its kNN graph from coordinates that two implementations know only to ~1e-6.  Where
some centre's K-th and (K+1)-th neighbour are almost equally far away, one flipped neighbour changes the output far beyond
any tolerance -- in the reference as well.  So every fixture here has a CONDITION: at every block boundary the smallest gap
between the K-th and the (K+1)-th neighbour distance over all real centres is at least MIN_GAP = 5e-4 A (5 x POS_TOL).
`boundary_gaps` measures it on the oracle's own run; the host test asserts it for every fixture, so no GPU case ever has to
leave a sample out.  Samples whose graph is complete (N - 1 <= K) have no (K+1)-th neighbour and are exempt."""
import contextlib

import torch

import golden_utils as GU
from decompdiff_amd import shipped_config, synth
from oracle import diffusion as OD
from oracle import model as OM

MIN_GAP = 5e-4
KEYS = ("pred_ligand_pos", "pred_ligand_v", "pred_bond")

# name -> blocks x layers, configuration overrides, pocket (seed, protein atoms, arm atoms, scaffold atoms), samples, batch seed
FORWARD = {
    "2x3": dict(nb=2, L=3, over={}, pocket=(1, 48, (4, 4), 4), B=2, seed=31),
    "3x3": dict(nb=3, L=3, over={}, pocket=(2, 48, (4, 4), 4), B=2, seed=62),               # odd L, 9 steps > 8
    "2x6": dict(nb=2, L=6, over={}, pocket=(1, 48, (4, 4), 4), B=2, seed=43),
    "2x6_nl36": dict(nb=2, L=6, over={}, pocket=(3, 60, (12, 12), 12), B=1, seed=64),        # 36-atom ligand: the 3-tile node kernel
    "2x3_k48": dict(nb=2, L=3, over=dict(knn=48), pocket=(2, 58, (4, 4), 4), B=2, seed=65),  # 70 atoms, 48 neighbours
    "2x3_preatt": dict(nb=2, L=3, over=dict(bond_net_type="pre_att"), pocket=(1, 48, (4, 4), 4), B=2, seed=36),
    "2x3_outfc": dict(nb=2, L=3, over=dict(x2h_out_fc=True), pocket=(2, 48, (4, 4), 4), B=2, seed=37),
}
# samples of different sizes (one batch, padded launch): all above knn + 1 = 33 atoms; TINY: the second one below (size groups)
RAGGED = [(1, 48, (4, 4), 4), (2, 40, (3, 3), 3), (5, 52, (5, 5), 6)]
TINY = [(1, 48, (4, 4), 4), (2, 20, (2, 2), 2), (5, 52, (5, 5), 6)]
RAGGED_SEED, TINY_SEED, RAGGED_CHAIN_SEED = 51, 71, 251
# frozen coordinates, padded: two samples of different sizes
FROZEN_RAGGED = [(1, 48, (4, 4), 4), (2, 40, (3, 3), 3)]
# frozen coordinates, dense, 130 + 12 = 142 atoms per sample: more than 128, the second candidate class of the graph kernel
FROZEN_LARGE, FROZEN_LARGE_SEED = (4, 130, (4, 4), 4), 83
# sampling: pocket, samples, noise seed
SAMPLING = dict(nb=2, L=3, pocket=(1, 48, (4, 4), 4), B=2, seed=321)
# training: a dense batch and one of two sizes
TRAINING = dict(nb=2, L=3, pocket=(2, 48, (4, 4), 4), B=2, seed=101, time_step=(700, 150))
TRAINING_RAGGED = dict(nb=2, L=3, pockets=[(1, 48, (4, 4), 4), (2, 40, (3, 3), 3)], seed=61, time_step=(600, 250))


def config(nb, L, **over):
    return shipped_config(num_blocks=nb, num_layers=L, **over)


def pocket(spec):
    seed, n_p, arms, sca = spec
    return synth.make_pocket(seed, n_p, arms, sca, num_full_protein=n_p + 20)


def batch(spec, B, seed):
    torch.manual_seed(seed)
    return synth.build_sampling_batch(pocket(spec), B)


def forward_batch(name):
    f = FORWARD[name]
    return batch(f["pocket"], f["B"], f["seed"])


def ragged_parts(specs, seed=RAGGED_SEED):
    torch.manual_seed(seed)
    return [synth.build_sampling_batch(pocket(s), 1) for s in specs]


def oracle_forward(sd, cfg, b, trace=None):
    with torch.no_grad():
        return OM.forward(sd, cfg, b["protein_pos"], b["protein_v"], b["batch_protein"], b["init_ligand_pos"], b["init_ligand_v"],
                          b["ligand_v_aux"], b["batch_ligand"], b["ligand_fc_bond_index"], b["init_ligand_fc_bond_type"], trace=trace)


def knn_gap(x, batch_vec, K):
    """Smallest (K+1)-th minus K-th neighbour distance over the centres of every sample with more than K + 1 atoms (inf if none)."""
    worst = float("inf")
    x = x.detach().double()
    for b in range(int(batch_vec.max()) + 1):
        xb = x[batch_vec == b]
        n = xb.shape[0]
        if n - 1 <= K:
            continue
        d = torch.cdist(xb, xb)
        d.fill_diagonal_(float("inf"))
        ds = d.sort(dim=1).values
        worst = min(worst, float((ds[:, K] - ds[:, K - 1]).min()))
    return worst


@contextlib.contextmanager
def boundary_gaps(K):
    """While active, every run of the oracle's refine net (forward, sampling loop, autograd) records, for each block after the
    first, the kNN gap of the coordinates that block's graph is built from -- read from the oracle's own `trace`.  Yields the
    list of gaps."""
    gaps = []
    inner = OM.refine_net

    def traced(sd, cfg, h, x, bond_index, h_bond, mask_ligand, mask_ligand_atom, batch, trace=None, stats=None):
        tr = [] if trace is None else trace
        n0 = len(tr)
        out = inner(sd, cfg, h, x, bond_index, h_bond, mask_ligand, mask_ligand_atom, batch, tr, stats)
        mine = tr[n0:]
        starts = [i for i, e in enumerate(mine) if "edge_index" in e]
        assert len(starts) == cfg.num_blocks
        for i in starts[1:]:
            gaps.append(knn_gap(mine[i - 1]["x"], batch, K))     # x behind the previous block's last layer
        return out
    OM.refine_net = traced
    try:
        yield gaps
    finally:
        OM.refine_net = inner


def sampling_inputs():
    s = SAMPLING
    b = batch(s["pocket"], s["B"], s["seed"])
    noise = synth.draw_step_noise(10, b["init_ligand_pos"].size(0), b["init_ligand_fc_bond_type"].size(0))
    return b, noise


def ragged_chain_inputs(steps=3):
    """The samples of RAGGED with their own step noise: (parts, noises), and collated by `collate_chain`."""
    parts = ragged_parts(RAGGED, RAGGED_CHAIN_SEED)
    noises = [synth.draw_step_noise(steps, p["init_ligand_pos"].size(0), p["init_ligand_fc_bond_type"].size(0)) for p in parts]
    return parts, noises


def oracle_chain(sd, cfg, b, noise, steps, drift=None, t_start=None):
    n = {k: v[:steps] for k, v in noise.items()}
    return OD.sample_diffusion(sd, cfg, num_steps=steps, energy_drift_opt=drift, noise=n, t_start=t_start, **b)


def loss_kwargs(b, time_step, device):
    d = lambda t: t.to(device) if torch.is_tensor(t) else t
    return dict(protein_pos=d(b["protein_pos"]), protein_v=d(b["protein_v"]), batch_protein=d(b["batch_protein"]),
                protein_group_idx=d(b["protein_group_idx"]), ligand_pos=d(b["init_ligand_pos"]), ligand_v=d(b["init_ligand_v"]),
                ligand_v_aux=d(b["ligand_v_aux"]), batch_ligand=d(b["batch_ligand"]), ligand_group_idx=d(b["ligand_group_idx"]),
                prior_centers=d(b["prior_centers"]), prior_stds=d(b["prior_stds"]), prior_num_atoms=d(b["prior_num_atoms"]),
                batch_prior=d(b["batch_prior"]), prior_group_idx=d(b["prior_group_idx"]),
                ligand_decomp_batch=d(b["ligand_decomp_batch"]), ligand_decomp_index=d(b["ligand_decomp_index"]),
                ligand_fc_bond_index=d(b["ligand_fc_bond_index"]), ligand_fc_bond_type=d(b["init_ligand_fc_bond_type"]),
                batch_ligand_bond=d(b["batch_ligand_bond"]), time_step=torch.tensor(time_step, dtype=torch.long, device=device))


def training_batch(ragged=False):
    if ragged:
        t = TRAINING_RAGGED
        return synth.concat_sampling_batches(ragged_parts(t["pockets"], t["seed"])), t
    t = TRAINING
    return batch(t["pocket"], t["B"], t["seed"]), t


def perturbed_network_inputs(model, kw, noise_seed):
    """What get_diffusion_loss hands to the score network for `kw` (training.objective's forward diffusion, on the tensors' own
    device; pure torch): the arguments of oracle.model.forward.  The draws follow training.prepare_batch on the CPU generator."""
    from decompdiff_amd import training as T
    torch.manual_seed(noise_seed)
    prep = T.prepare_batch(model, kw["protein_pos"], kw["protein_v"], kw["batch_protein"], kw["ligand_pos"], kw["ligand_v"],
                           kw["ligand_v_aux"], kw["batch_ligand"], kw["prior_centers"], kw["prior_stds"], kw["prior_num_atoms"],
                           kw["batch_prior"], kw["ligand_decomp_batch"], kw["ligand_fc_bond_index"], kw["ligand_fc_bond_type"],
                           kw["batch_ligand_bond"], time_step=kw["time_step"])
    t, bl, blb = prep["time_step"], kw["batch_ligand"], kw["batch_ligand_bond"]
    a = model.alphas_cumprod.index_select(0, t)[bl].unsqueeze(-1)
    centers, stds = kw["prior_centers"][kw["ligand_decomp_batch"]], kw["prior_stds"][kw["ligand_decomp_batch"]]
    pos = a.sqrt() * (kw["ligand_pos"] - centers) + (1.0 - a).sqrt() * prep["pos_noise"] * stds + centers
    gumbel = lambda u: -torch.log(-torch.log(u + 1e-30) + 1e-30)
    v = (gumbel(prep["u_v"]) + T._Trans(model.atom_type_trans).pred(T._log_onehot(kw["ligand_v"], model.num_classes), t, bl)).argmax(-1)
    bt = (gumbel(prep["u_b"]) + T._Trans(model.bond_type_trans).pred(T._log_onehot(kw["ligand_fc_bond_type"], model.num_bond_classes),
                                                                    t, blb)).argmax(-1)
    B = int(kw["batch_protein"].max()) + 1
    off = torch.zeros(B, 3).index_add_(0, kw["batch_protein"].cpu(), kw["protein_pos"].cpu())
    off = (off / torch.bincount(kw["batch_protein"].cpu(), minlength=B).view(B, 1)).to(pos.device)
    return dict(protein_pos=kw["protein_pos"] - off[kw["batch_protein"]], protein_v=kw["protein_v"], batch_protein=kw["batch_protein"],
                init_ligand_pos=pos - off[bl], init_ligand_v=v, ligand_v_aux=kw["ligand_v_aux"], batch_ligand=bl,
                ligand_fc_bond_index=kw["ligand_fc_bond_index"], init_ligand_fc_bond_type=bt)
