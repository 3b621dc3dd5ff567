"""Chain init (``sample_diffusion(init=...)``, dd_chain_init / k_chain_init): the chain's first state drawn on the device with the
chain's own Philox addressing -- from the prior, or a known ligand noised to the level the first step expects.

Every comparison is ``torch.equal`` unless stated: the state is recomputed from the exposed draws (dd_debug_philox kinds 5 / 6 / 9)
op by op in fp32, a chain with ``init`` is the chain started from the zero-step state, and a keyed sample's state and chain are
those of the sample alone.  Shapes: those of the sample-key tests (pockets of 40-48 atoms, ligands of 6 / 8 / 9 atoms, B <= 4,
0-3 steps) plus one 24-atom ligand at B = 4 whose 288 coordinates cross a 256-thread block, and one 13-class case (four Philox
class blocks)."""
import numpy as np
import pytest
import torch

import golden_utils as GU
from decompdiff_amd import harness, hip_lib, synth
from decompdiff_amd.pocket_data import PocketData
from test_gpu_parity import dev, model, to_dev
from test_gpu_sample_keys import KEYS, POCKETS, TRAJ, assert_same, model_nc, run, single, split

pytestmark = pytest.mark.gpu

GIVEN = ("init_ligand_pos", "init_ligand_v", "init_ligand_fc_bond_type")
POCKETS[24] = synth.make_pocket_tiny(14, num_protein=48, arm_atoms=(8, 8), scaffold_atoms=8)
ATOM_PRIOR = torch.tensor([0.05, 0.4, 0.15, 0.2, 0.05, 0.05, 0.05, 0.05])
BOND_PRIOR = torch.tensor([0.7, 0.15, 0.05, 0.03, 0.07])


def bare(b):
    """The batch without a first state: what a call with ``init`` takes."""
    return dict(b, **{k: None for k in GIVEN})


def noised(b, **over):
    """``init`` that noises the batch's own host-drawn state as the known ligand."""
    return dict(mode="noised", pos=b["init_ligand_pos"], v=b["init_ligand_v"], bond=b["init_ligand_fc_bond_type"], **over)


def started_from(b, state):
    return dict(b, init_ligand_pos=state["pos"], init_ligand_v=state["v"], init_ligand_fc_bond_type=state["bond"])


def draw(seed, word, rows, kind, nc=8):
    """dd_debug_philox: [rows, classes] uniforms (kinds 1-6) or [rows] normals (7-9), fp32 on the host."""
    sid = kind & 0xff
    cols = 1 if sid in (7, 8, 9) else (5 if sid in (2, 4, 6) else nc)
    out = torch.empty(rows * cols, device=dev())
    hip_lib.check(hip_lib.load().dd_debug_philox(seed, word, rows, sid | ((nc << 8) if sid in (1, 3, 5) and nc != 8 else 0),
                                                 hip_lib.ptr(out), hip_lib.stream_ptr()), "dd_debug_philox")
    torch.cuda.synchronize()
    return out.cpu().view(rows, cols) if cols > 1 else out.cpu()


def offsets(b):
    """The per-sample protein centroid as the dense path computes it (fp32 accumulation in row order / count)."""
    B = int(b["batch_protein"].max()) + 1
    NP = b["batch_protein"].numel() // B
    tot = torch.zeros(B, 3).index_add_(0, torch.arange(B).repeat_interleave(NP), b["protein_pos"].float())
    return (tot / float(NP))[b["batch_ligand"]]


def gumbel64(u):
    u = u.double()
    return -torch.log(-torch.log(u + 1e-30) + 1e-30)


def check_classes(got, scores, margin, share, what):
    """``got`` equals the arg-max of ``scores`` on every row whose two largest scores differ by more than ``margin``; those
    rows are at least ``share`` of all."""
    top = scores.topk(2, dim=-1).values
    clear = (top[:, 0] - top[:, 1]) > margin
    assert float(clear.double().mean()) >= share, (what, float(clear.double().mean()))
    assert torch.equal(got[clear], scores.argmax(-1)[clear]), what


# ------------------------------------------------------------------------------------------------ 1: the exact state
@pytest.mark.parametrize("nl,B,nc", [(8, 1, 8), (8, 4, 8), (8, 4, 13), (24, 4, 8)], ids=["B1", "B4", "B4-13classes", "B4-24atoms"])
def test_prior_state_is_the_exposed_draws(nl, B, nc):
    m = model_nc(nc)
    b = synth.concat_sampling_batches([single(nl, 600 + s, nc) for s in range(B)]) if B > 1 else single(nl, 600, nc)
    seed, T = 0xC3A5C85C97CB3127, m.num_timesteps
    n, nb = B * nl, B * nl * (nl - 1)
    r = run(m, bare(b), 0, seed=seed, init=dict(mode="prior"))
    assert set(r) == {"pos", "v", "bond"} and r["pos"].shape == (n, 3) and r["v"].shape == (n,) and r["bond"].shape == (nb,)
    e = draw(seed, T, 3 * n, 9).view(n, 3)
    off = offsets(b)
    cen, std = b["prior_centers"][b["ligand_decomp_batch"]], b["prior_stds"][b["ligand_decomp_batch"]]
    assert torch.equal(r["pos"], ((cen - off) + e * std) + off)
    # uniform priors: the first arg-max of the uniforms (the Gumbel map is monotone)
    check_classes(r["v"], draw(seed, T, n, 5, nc).double(), 1e-6, 0.99, "atom classes")
    check_classes(r["bond"], draw(seed, T, nb, 6).double(), 1e-6, 0.99, "bond classes")
    assert int(r["v"].max()) < nc and len(r["v"].unique()) > 1 and len(r["bond"].unique()) > 1


def test_prior_state_with_priors_and_centres_of_its_own():
    m, B, nl = model(0), 4, 8
    b = synth.concat_sampling_batches([single(nl, 610 + s) for s in range(B)])
    seed, T = 77, m.num_timesteps
    n, nb = B * nl, B * nl * (nl - 1)
    centers, stds = b["prior_centers"] + 0.75, b["prior_stds"] * 1.5
    r = run(m, bare(b), 0, seed=seed, init=dict(mode="prior", centers=centers, stds=stds, atom_prior=ATOM_PRIOR, bond_prior=BOND_PRIOR))
    e = draw(seed, T, 3 * n, 9).view(n, 3)
    off = offsets(b)
    assert torch.equal(r["pos"], ((centers[b["ligand_decomp_batch"]] - off) + e * stds[b["ligand_decomp_batch"]]) + off)
    lp_v, lp_b = torch.log(ATOM_PRIOR / ATOM_PRIOR.sum()).float().double(), torch.log(BOND_PRIOR / BOND_PRIOR.sum()).float().double()
    check_classes(r["v"], gumbel64(draw(seed, T, n, 5)) + lp_v, 1e-4, 0.98, "atom classes")
    check_classes(r["bond"], gumbel64(draw(seed, T, nb, 6)) + lp_b, 1e-4, 0.98, "bond classes")


@pytest.mark.parametrize("level", ["first", "middle"])
def test_noised_state_is_the_forward_process_of_the_known_ligand(level):
    m, B, nl = model(0), 4, 8
    b = synth.concat_sampling_batches([single(nl, 620 + s) for s in range(B)])
    seed, T = 991, m.num_timesteps
    start_step = T - 1 if level == "first" else T // 2
    l = T - 1 - start_step
    n, nb = B * nl, B * nl * (nl - 1)
    r = run(m, bare(b), 0, seed=seed, start_step=start_step, init=noised(b))
    e = draw(seed, l, 3 * n, 9).view(n, 3)
    off = offsets(b)
    cc, std = b["prior_centers"][b["ligand_decomp_batch"]] - off, b["prior_stds"][b["ligand_decomp_batch"]]
    tab = m.fixed_step_table().cpu()
    A, S = tab[0, l], tab[1, l]
    x0c = b["init_ligand_pos"] - off
    assert torch.equal(r["pos"], ((A * (x0c - cc) + (S * e) * std) + cc) + off)
    if level == "first":                                       # level 0 keeps almost every class, the middle level moves many
        assert float((r["v"] == b["init_ligand_v"]).double().mean()) > 0.9
    for got, v0, kind, rows, tr in ((r["v"], b["init_ligand_v"], 5, n, m.atom_type_trans), (r["bond"], b["init_ligand_fc_bond_type"], 6, nb, m.bond_type_trans)):
        nc = tr.prior_probs.numel()
        lca, l1mca = tr.log_alphas_cumprod_v.float().cpu().double()[l], tr.log_one_minus_alphas_cumprod_v.float().cpu().double()[l]
        lp = tr.prior_probs.reshape(-1).float().cpu().double()
        onehot = torch.nn.functional.one_hot(v0, nc).bool()
        log_onehot = torch.where(onehot, torch.tensor(0.0, dtype=torch.float64), torch.tensor(-69.07755278982137, dtype=torch.float64))
        q0 = torch.logaddexp(log_onehot + lca, (l1mca + lp).expand(rows, nc))
        check_classes(got, gumbel64(draw(seed, l, rows, kind)) + q0, 1e-4, 0.98, f"kind {kind}")


# ------------------------------------------------------------------------------------------------ 2: only the first state changes
def _fixed(b, mode):
    """The first three atoms of every sample held at values of their own."""
    n, nb = b["batch_ligand"].numel(), b["init_ligand_fc_bond_type"].numel()
    g = torch.Generator().manual_seed(9)
    mask = torch.zeros(n, dtype=torch.bool)
    mask.view(-1, 8)[:, :3] = True
    return dict(mask=mask, pos=b["prior_centers"][b["ligand_decomp_batch"]] + 0.3 * torch.randn(n, 3, generator=g),
                v=torch.randint(0, 8, (n,), generator=g), bond=torch.randint(0, 5, (nb,), generator=g), mode=mode)


@pytest.mark.parametrize("variant", ["streamed", "eager", "captured", "hold", "replace", "resample"])
@pytest.mark.parametrize("mode", ["prior", "noised"])
def test_a_chain_with_init_is_the_chain_started_from_the_drawn_state(mode, variant):
    """3 steps with ``init`` and seed k = 3 steps from the zero-step state with seed k: results and all six trajectories.  (Model
    frame: no offset is re-added and subtracted in between.)"""
    m = model(0)
    b = synth.concat_sampling_batches([single(8, 630), single(8, 631)])
    k = KEYS[6]
    kw = dict(center_pos_mode="none", seed=k)
    if variant == "eager":
        kw["use_graph"] = False
    if variant == "captured":
        kw["keep_traj"] = False
    if variant in ("hold", "replace", "resample"):
        kw["fixed"] = _fixed(b, "hold" if variant == "hold" else "replace")
    if variant == "resample":
        kw["resample"] = dict(jump_length=2, n_resample=2)
    init = dict(mode="prior")
    if mode == "noised":                                       # (replace draws its held rows' level itself: start_step == 0)
        kw["start_step"] = 0 if variant in ("replace", "resample") else 500
        init = noised(b)
    zero = run(m, bare(b), 0, init=init, **{x: y for x, y in kw.items() if x != "resample"})
    if "fixed" in kw:                                          # the held rows of the first state are dd_fixed_init's
        fx = kw["fixed"]
        held_b = fx["mask"][b["ligand_fc_bond_index"][0]] & fx["mask"][b["ligand_fc_bond_index"][1]]
        if variant == "hold":
            assert torch.equal(zero["pos"][fx["mask"]], fx["pos"][fx["mask"]]) and torch.equal(zero["v"][fx["mask"]], fx["v"][fx["mask"]])
            assert torch.equal(zero["bond"][held_b], fx["bond"][held_b])
        free = run(m, bare(b), 0, init=init, **{x: y for x, y in kw.items() if x not in ("resample", "fixed")})
        assert torch.equal(zero["pos"][~fx["mask"]], free["pos"][~fx["mask"]]) and torch.equal(zero["v"][~fx["mask"]], free["v"][~fx["mask"]])
        assert torch.equal(zero["bond"][~held_b], free["bond"][~held_b]) and not torch.equal(zero["pos"], free["pos"])
    got = run(m, bare(b), 3, init=init, **kw)
    want = run(m, started_from(b, zero), 3, **kw)
    assert (variant == "captured") != all(t in got for t in TRAJ)
    assert_same(got, want, f"{mode}, {variant}")
    assert not torch.equal(got["pos"], zero["pos"])


# ------------------------------------------------------------------------------------------------ 3: batch independence
@pytest.mark.parametrize("mode", ["prior", "noised"])
def test_dense_batch_of_four_equals_each_sample_alone(mode):
    m, steps = model(0), 2
    singles = [single(8, 640 + s) for s in range(4)]
    ini = (lambda b: dict(mode="prior")) if mode == "prior" else noised
    kw = dict(start_step=300) if mode == "noised" else {}
    alone = [run(m, bare(singles[s]), steps, seed=KEYS[s], init=ini(singles[s]), **kw) for s in range(4)]
    assert not torch.equal(alone[0]["pos"] - offsets(singles[0]), alone[1]["pos"] - offsets(singles[1]))
    for order in ([0, 1, 2, 3], [3, 2, 1, 0]):
        batch = synth.concat_sampling_batches([singles[s] for s in order])
        parts = split(run(m, bare(batch), steps, sample_keys=[KEYS[s] for s in order], init=ini(batch), **kw), [8] * 4)
        for pos, s in enumerate(order):
            assert_same(parts[pos], alone[s], f"{mode}: sample {s} at position {pos}")
        zero = split(run(m, bare(batch), 0, sample_keys=[KEYS[s] for s in order], init=ini(batch), **kw), [8] * 4)
        for pos, s in enumerate(order):
            assert_same(zero[pos], run(m, bare(singles[s]), 0, seed=KEYS[s], init=ini(singles[s]), **kw), f"{mode}: first state of {s}")


@pytest.mark.parametrize("mode", ["prior", "noised"])
def test_ragged_batch_padded_grouped_and_alone_agree(mode, monkeypatch):
    """Ligands of 8, 6, 9 and 6 atoms as one padded batch (a 6-atom ligand's rows inside a width of 9: its padding rows are not
    drawn and reach no result), as size groups one after the other, as size groups round-robin, and each sample alone."""
    m, steps = model(0), 2
    n_l = [8, 6, 9, 6]
    singles = [single(n, 650 + s) for s, n in enumerate(n_l)]
    batch = synth.concat_sampling_batches(singles)
    keys = KEYS[:4]
    ini = (lambda b: dict(mode="prior", atom_prior=ATOM_PRIOR)) if mode == "prior" else noised
    kw = dict(start_step=300) if mode == "noised" else {}
    alone = [run(m, bare(s), steps, seed=k, init=ini(s), **kw) for s, k in zip(singles, keys)]
    first = [run(m, bare(s), 0, seed=k, init=ini(s), **kw) for s, k in zip(singles, keys)]
    for rmode, concurrent in (("padded", "0"), ("groups", "0"), ("groups", "1")):
        monkeypatch.setenv("DD_RAGGED_MODE", rmode)
        monkeypatch.setenv("DD_RAGGED_CONCURRENT", concurrent)
        parts = split(run(m, bare(batch), steps, sample_keys=keys, init=ini(batch), **kw), n_l)
        zero = split(run(m, bare(batch), 0, sample_keys=keys, init=ini(batch), **kw), n_l)
        for s in range(4):
            assert_same(parts[s], alone[s], f"{mode}, {rmode} (concurrent {concurrent}), sample {s}")
            assert_same(zero[s], first[s], f"{mode}, {rmode} (concurrent {concurrent}), first state of sample {s}")
            assert bool(torch.isfinite(parts[s]["pos"]).all()) and int(parts[s]["v"].max()) < 8 and int(parts[s]["bond"].max()) < 5


# ------------------------------------------------------------------------------------------------ 4: determinism and separation
def test_determinism_and_streams_of_their_own():
    m = model(0)
    b = synth.concat_sampling_batches([single(8, 660), single(8, 661)])
    T = m.num_timesteps
    for init, kw in ((dict(mode="prior"), {}), (noised(b), dict(start_step=400))):
        a = run(m, bare(b), 0, seed=5, init=init, **kw)
        assert_same(run(m, bare(b), 0, seed=5, init=init, **kw), a, "the same call twice")
        other = run(m, bare(b), 0, seed=6, init=init, **kw)
        assert not torch.equal(other["pos"], a["pos"]) and not torch.equal(other["bond"], a["bond"])
        keyed = run(m, bare(b), 0, sample_keys=KEYS[:2], init=init, **kw)
        assert not torch.equal(run(m, bare(b), 0, sample_keys=[KEYS[0], KEYS[2]], init=init, **kw)["pos"][8:], keyed["pos"][8:])
        assert torch.equal(run(m, bare(b), 0, sample_keys=[KEYS[0], KEYS[2]], init=init, **kw)["pos"][:8], keyed["pos"][:8])
    # the draws are no step's and no jump's: another stream at the same key, row and time word
    for word in (T, T - 1, 599):
        z9 = draw(5, word, 48, 9)
        assert not torch.equal(z9, draw(5, word, 48, 7)) and not torch.equal(z9, draw(5, word, 48, 8))
        assert float((z9 == draw(5, word, 48, 7)).double().mean()) < 0.05 and float((z9 == draw(5, word, 48, 8)).double().mean()) < 0.05
        u5, u6 = draw(5, word, 16, 5), draw(5, word, 112, 6)
        for other in (1, 3):
            assert float((u5 == draw(5, word, 16, other)).double().mean()) < 0.05
        for other in (2, 4):
            assert float((u6 == draw(5, word, 112, other)).double().mean()) < 0.05
    assert torch.equal(draw(5, T, 48, 9), draw(5, T, 48, 9)) and not torch.equal(draw(5, T, 48, 9), draw(5, T - 1, 48, 9))


# ------------------------------------------------------------------------------------------------ 5: stream statistics
def test_chain_init_streams_statistics():
    """Kinds 5 / 6 / 9 with the moments and the Kolmogorov-Smirnov check of test_philox_noise_statistics, its sample sizes and
    its bounds."""
    from scipy import stats
    u = draw(2021, 1000, 125000, 5).double().numpy().reshape(-1)
    ub = draw(2021, 1000, 200000, 6).double().numpy().reshape(-1)
    z = draw(2021, 1000, 1000000, 9).double().numpy()
    for name, a in (("u_v", u), ("u_b", ub)):
        ks = stats.kstest(a, "uniform").statistic
        print(f"{name}: mean {a.mean():.5f} var {a.var():.5f} min {a.min():.3g} max {a.max():.8f} KS {ks:.2g}")
        assert a.min() >= 0.0 and a.max() < 1.0
        assert abs(a.mean() - 0.5) < 1e-3 and abs(a.var() - 1.0 / 12.0) < 1e-3 and ks < 2.5e-3
    ks = stats.kstest(z, "norm").statistic
    m4 = float((z ** 4).mean())
    print(f"eps: mean {z.mean():.5f} var {z.var():.5f} 4th moment {m4:.4f} max |z| {np.abs(z).max():.2f} KS {ks:.2g}")
    assert abs(z.mean()) < 3e-3 and abs(z.var() - 1.0) < 5e-3 and abs(m4 - 3.0) < 0.05 and ks < 2.5e-3
    assert np.isfinite(z).all() and np.abs(z).max() < 6.0
    uu = u.reshape(-1, 8)
    assert abs(np.corrcoef(uu[:, 0], uu[:, 4])[0, 1]) < 5e-3 and abs(np.corrcoef(uu[:-1, 7], uu[1:, 0])[0, 1]) < 5e-3
    assert len(np.unique(u)) > 0.97 * len(u)
    for other in (draw(2021, 999, 125000, 5), draw(2022, 1000, 125000, 5), draw(2021, 1000, 125000, 1)):
        o = other.double().numpy().reshape(-1)
        assert abs(np.corrcoef(u, o)[0, 1]) < 5e-3 and not np.array_equal(u, o)


# ------------------------------------------------------------------------------------------------ 6: the harness
def test_harness_job_is_the_same_per_sample_under_any_batching():
    """6 samples, 2 steps, init="device" in a mode that draws the atom counts: batch sizes 1 / 2 / 3 / 6, pooled batches and a run
    split in two calls agree per sample on every output list; the caller's generators are left alone."""
    f = GU.make_pocket_fields(5, beta=True)
    pocket = PocketData(**{k: f[k] for k in ("protein_pos", "protein_element", "protein_is_backbone", "protein_atom_to_aa_type",
                                             "pocket_atom_masks", "num_arms", "num_scaffold", "arms_prior", "scaffold_prior",
                                             "ligand_atom_mask", "ligand_pos", "full_protein_pos")})
    m = model(0)
    job = lambda n=6, **kw: harness.sample_diffusion_ligand_decomp(m, pocket, num_samples=n, device="cuda:0", num_steps=2, init="device",
                                                                   sample_key_seed=7, prior_mode="beta_prior", num_atoms_mode="old",
                                                                   use_graph=kw.pop("use_graph", False), **kw)
    torch.manual_seed(11)
    np.random.seed(12)
    t0, n0 = torch.get_rng_state(), np.random.get_state()
    want = job(batch_size=1)
    assert torch.equal(torch.get_rng_state(), t0) and np.array_equal(np.random.get_state()[1], n0[1]) and np.random.get_state()[2] == n0[2]
    lists = [k for k in want if k != "time_list"]
    assert {"pred_pos", "pred_v", "pred_bond_type", "pred_pos_traj", "pred_v_traj", "pred_v0_traj", "pred_vt_traj", "pred_b_traj",
            "pred_bt_traj"} <= set(lists)
    sizes = [len(v) for v in want["pred_v"]]
    assert len(set(sizes)) >= 2 and all(t.shape == (2, n, 3) for t, n in zip(want["pred_pos_traj"], sizes))
    halves = [job(3, batch_size=2, first_sample_index=0), job(3, batch_size=3, first_sample_index=3)]
    runs = {"2": job(batch_size=2), "3": job(batch_size=3), "6 (captured)": job(batch_size=6, use_graph=True),
            "pooled": job(batch_size=2, pool_batches=2), "two calls": {k: halves[0][k] + halves[1][k] for k in lists}}
    for name, got in runs.items():
        for k in lists:
            assert len(got[k]) == 6, (name, k)
            for s in range(6):
                assert np.array_equal(got[k][s], want[k][s]), (name, k, s)
    assert not np.array_equal(want["pred_pos"][0][:4], want["pred_pos"][1][:4])
