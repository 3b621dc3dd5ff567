"""Resampling (``sample_diffusion(fixed=..., resample=dict(jump_length=j, n_resample=r))``, dd_resample_jump /
dd_sample_steps_resample / dd_graph_create_resample / dd_sampler_reset_resample) on the GPU.

References.  The jump: this file's float64 restatement of the header's formulas (`jump64`) fed with the draws that dd_debug_philox
returns for the documented (stream, time word).  Whole chains: the oracle loop of the fixed-atom tests, one oracle step per position
with that position's device draws, and `jump64` at every jump.  Compositions (eager / captured / padded / grouped / alone) are
``torch.equal``.  Shapes as in tests/test_gpu_fixed_atoms.py; ranges are 6 steps with j = 2, r = 2 (12 positions, 3 jumps) unless
stated otherwise."""
import ctypes
import functools
import math

import pytest
import torch

import golden_utils as GU
from decompdiff_amd import batch_layout as BL
from decompdiff_amd import harness, hip_lib, pocket_data, resample_schedule, synth
from test_gpu_fixed_atoms import (assert_same, fixed_rows, forward_level, held_bonds, known, offsets, oracle_loop, pair, ragged_case,
                                  scaffold, ulp)
from test_gpu_parity import POS_TOL, dev, maxabs, model
from test_gpu_sample_keys import KEYS, TRAJ, model_nc, run, single, split, to_dev

pytestmark = pytest.mark.gpu
LOG_ZERO = math.log(1e-30)
RS = dict(jump_length=2, n_resample=2)


def rrun(m, b, steps=6, center_pos_mode="protein", **kw):
    """`run` that keeps ``t_traj``."""
    r = m.sample_diffusion(num_steps=steps, center_pos_mode=center_pos_mode, **to_dev(b), **kw)
    out = {k: r[k].cpu() for k in ("pos", "v", "bond")}
    out.update({k: torch.stack(r[k]) for k in TRAJ if len(r[k])})
    if "t_traj" in r:
        out["t_traj"] = r["t_traj"]
    return out


def without_t(r):
    return {k: v for k, v in r.items() if k != "t_traj"}


def times(t_hi, steps, j=2, r=2):
    return [o[1] for o in resample_schedule(t_hi, t_hi - steps + 1, j, r) if o[0] == "step"]


def draws(seed, word, n, nb, nc=8, jump=False):
    """The device's draws of one reverse step (streams 1, 2, 7) or one jump (3, 4, 8) at Philox time word `word`."""
    lib = hip_lib.load()
    kinds = (3, 4, 8) if jump else (1, 2, 7)
    out = []
    for kind, rows, width in ((kinds[0] | (nc << 8), n, nc), (kinds[1], nb, 5), (kinds[2], 3 * n, 1)):
        t = torch.empty(rows * width, device=dev())
        hip_lib.check(lib.dd_debug_philox(seed, word, rows, kind, hip_lib.ptr(t), hip_lib.stream_ptr()), "dd_debug_philox")
        out.append(t)
    torch.cuda.synchronize()
    return {"u_v": out[0].cpu().view(n, nc), "u_b": out[1].cpu().view(nb, 5), "eps": out[2].cpu().view(n, 3)}


def keyed_draws(keys, n_l, word, nc=8, jump=False):
    """Per-sample keys: sample b draws with keys[b] at the rows of its own enumeration."""
    parts = [draws(k, word, n, n * (n - 1), nc, jump) for k, n in zip(keys, n_l)]
    return {k: torch.cat([p[k] for p in parts]) for k in ("u_v", "u_b", "eps")}


# ------------------------------------------------------------------------------------------------ float64 restatement of the jump
def jump64(m, b, xc, v, bond, l, j, d, off):
    """q(x_m | x_l), m = l + j, for EVERY row (include/decompdiff_hip.h, dd_resample) in float64 from the centred fp32 coordinates
    `xc` [n,3], the classes `v` [n] / `bond` [n_bond] and one jump's draws `d`: new xc, v, bond, the smallest gap between the two
    best scores of a row (atoms, bonds), the largest magnitude that enters the coordinate formula, and the stay probabilities."""
    mm = l + j
    ac = torch.cat([torch.ones(1, dtype=torch.float64), m.alphas_cumprod.detach().double().cpu()])
    a = ac[mm + 1] / ac[l + 1]
    A, S = a.sqrt(), (1.0 - a).sqrt()
    off_l = off[b["batch_ligand"]]
    cc = (b["prior_centers"].float()[b["ligand_decomp_batch"]] - off_l).double()
    std = b["prior_stds"].double()[b["ligand_decomp_batch"]]
    x = xc.double()
    noise = S * d["eps"].double() * std
    x2 = A * (x - cc) + noise + cc
    big = max(float(t.abs().max()) for t in (x, cc, x - cc, noise, x2))

    def classes(tr, cur, u):
        K = u.shape[-1]
        lc = torch.cat([torch.zeros(1, dtype=torch.float64), tr.log_alphas_cumprod_v.detach().double().cpu()])
        lr = lc[mm + 1] - lc[l + 1]
        l1mr = torch.log(1.0 - torch.exp(lr))
        log_cur = torch.full((cur.numel(), K), LOG_ZERO, dtype=torch.float64)
        log_cur[torch.arange(cur.numel()), cur] = 0.0
        p, q = log_cur + lr, l1mr + tr.prior_probs.detach().double().cpu().reshape(-1)
        mx = torch.max(p, q)
        score = -torch.log(-torch.log(u.double() + 1e-30) + 1e-30) + mx + torch.log(torch.exp(p - mx) + torch.exp(q - mx))
        top = score.topk(2, dim=-1).values
        stay = torch.exp(lr) + (1.0 - torch.exp(lr)) * tr.prior_probs.detach().double().cpu().reshape(-1).exp()
        return score.argmax(-1), top[:, 0] - top[:, 1], stay
    v2, gap_v, stay_v = classes(m.atom_type_trans, v, d["u_v"])
    b2, gap_b, stay_b = classes(m.bond_type_trans, bond, d["u_b"])
    return dict(xc=x2, v=v2, bond=b2, gap=min(float(gap_v.min()), float(gap_b.min())), big=big, A=float(A), S=float(S),
                stay_v=stay_v, stay_b=stay_b, cc=cc, std=std)


# ------------------------------------------------------------------------------------------------ 5: no jumps -- the plain chain
@pytest.mark.parametrize("mode", ["hold", "replace"])
def test_one_pass_and_a_jump_longer_than_the_range_are_the_plain_chain(mode):
    m, b = model(0), pair(101)
    fx = known(b, scaffold(b), 102, mode)
    for kw in (dict(), dict(use_graph=False), dict(keep_traj=False)):           # captured + streamed, eager, captured
        want = run(m, b, 4, seed=77, fixed=fx, **kw)
        for rs in (dict(jump_length=2, n_resample=1), dict(jump_length=5, n_resample=3)):
            got = rrun(m, b, 4, seed=77, fixed=fx, resample=rs, **kw)
            assert got["t_traj"].tolist() == [m.num_timesteps - 1 - i for i in range(4)] and got["t_traj"].dtype == torch.int64
            assert_same(without_t(got), want, f"{mode} {rs} {kw}")
    assert "t_traj" not in rrun(m, b, 2, seed=77, fixed=fx)


# ------------------------------------------------------------------------------------------------ 6: the jump alone
def prepared(m, b, fx, l, j, **kw):
    """A chain prepared at level l with device noise (l = -1: through the step at t = 0), its dd_sampler and buffers, and the three
    structs of dd_resample_jump built from them."""
    T = m.num_timesteps
    if l >= 0:
        m.sample_diffusion(num_steps=0, center_pos_mode="protein", start_step=T - 1 - l, fixed=fx, resample=dict(jump_length=j, n_resample=2),
                           **to_dev(b), **kw)
    else:
        m.sample_diffusion(num_steps=1, center_pos_mode="protein", start_step=T - 1, fixed=fx, resample=dict(jump_length=j, n_resample=1),
                           keep_traj=False, **to_dev(b), **kw)
    s, bufs = m._last
    pw = m._packed_weights()
    tab = m.resample_jump_table(j).to(dev())
    fxs = hip_lib.fixed_struct(fx["mode"], bufs["fx_mask"], bufs["fx_v0"], bufs["fx_b0"], bufs["fx_x0c"], bufs["fx_cc"],
                               pw["tab_fixed"] if fx["mode"] == "replace" else None)
    rss = hip_lib.resample_struct(j, tab, bufs["epoch"])
    return s, bufs, fxs, rss, tab


def device_jump(s, bufs, fxs, rss, keyed):
    lib = hip_lib.load()
    hip_lib.check(lib.dd_resample_jump(ctypes.byref(s), hip_lib.ptr(bufs["sample_keys"]) if keyed else None, ctypes.byref(fxs),
                                       ctypes.byref(rss), hip_lib.stream_ptr()), "dd_resample_jump")
    torch.cuda.synchronize()


def state_of(bufs, rows_l=None, rows_b=None):
    pick = lambda t, r: t.cpu() if r is None else t.cpu()[r]
    return pick(bufs["lig_pos"].view(-1, 3), rows_l).clone(), pick(bufs["lig_v"], rows_l).long(), pick(bufs["lig_bond"], rows_b).long()


JUMP_CASES = [  # (id, atom classes, mode, level l, jump length j, seed)
    ("clean-to-j-1", 8, "replace", -1, 3, 11), ("middle", 8, "replace", 480, 40, 12), ("to-T-1", 8, "replace", 994, 5, 13),
    ("hold-middle", 8, "hold", 300, 7, 14), ("hold-clean", 8, "hold", -1, 1, 15), ("nc13-middle", 13, "replace", 620, 25, 16),
    ("nc13-hold-to-T-1", 13, "hold", 899, 100, 17)]


@pytest.mark.parametrize("name,nc,mode,l,j,seed", JUMP_CASES, ids=[c[0] for c in JUMP_CASES])
def test_the_jump_alone_against_float64(name, nc, mode, l, j, seed):
    """Coordinates: the library forms x' from fp32 table entries with six fp32 operations (sub, three mul, two add) -- eight
    roundings of at most half an ulp of the largest magnitude `big` that enters: 4 ulp(big), the bound of the replace test.
    Classes: exact, the restatement's two best scores are more than 1e-3 apart in EVERY row (asserted)."""
    m, b = model_nc(nc), pair(110 + seed, nc=nc)
    T = m.num_timesteps
    mask = scaffold(b)
    mask[0] = True
    hb = held_bonds(b, mask)
    fx = known(b, mask, 120 + seed, mode, nc=nc, **(dict(init="given") if mode == "replace" else {}))
    s, bufs, fxs, rss, tab = prepared(m, b, fx, l, j, seed=seed)
    x0, v0, b0 = state_of(bufs)
    rs0 = bufs["step_counter"].cpu().tolist()
    assert rs0[1] - rs0[0] == l and int(bufs["epoch"].item()) == 0
    device_jump(s, bufs, fxs, rss, False)
    x1, v1, b1 = state_of(bufs)
    rs1 = bufs["step_counter"].cpu().tolist()
    assert rs1[0] == rs0[0] and rs1[1] == rs0[1] + j and rs1[2:] == rs0[2:] and int(bufs["epoch"].item()) == 1
    assert l + j <= T - 1 and (name != "to-T-1" or l + j == T - 1)
    d = draws(seed, (l + j) + 65536, 16, 112, nc, jump=True)
    w = jump64(m, b, x0, v0, b0, l, j, d, offsets(b))
    print(f"\nJUMP {name}: A {w['A']:.4f} S {w['S']:.4f}, smallest score gap {w['gap']:.3g}, "
          f"{int((w['v'] != v0).sum())} / 16 atoms and {int((w['bond'] != b0).sum())} / 112 bonds leave their class")
    assert w["gap"] > 1e-3
    moved_a, moved_b = (~mask, ~hb) if mode == "hold" else (torch.ones_like(mask), torch.ones_like(hb))
    assert torch.equal(v1, torch.where(moved_a, w["v"], v0)) and torch.equal(b1, torch.where(moved_b, w["bond"], b0))
    err, bound = float((x1.double() - w["xc"])[moved_a].abs().max()), 4 * ulp(w["big"])
    print(f"JUMP {name}: coordinates vs float64, error / bound {err / bound:.3f}")
    assert err <= bound, (err, bound)
    if mode == "hold":                                                          # held atoms and bonds keep their bits
        assert torch.equal(x1[mask], x0[mask]) and torch.equal(v1[mask], v0[mask]) and torch.equal(b1[hb], b0[hb])
        assert torch.equal(v1[mask], fx["v"][mask]) and torch.equal(b1[hb], fx["bond"][hb])
    assert not torch.equal(x1[moved_a], x0[moved_a])
    # the table on the device is the module's; a second jump draws at the next epoch: other bits
    assert torch.equal(tab.cpu(), m.resample_jump_table(j))
    if l + 2 * j <= T - 1:
        device_jump(s, bufs, fxs, rss, False)
        x2, v2, b2 = state_of(bufs)
        d2 = draws(seed, (l + 2 * j) + 2 * 65536, 16, 112, nc, jump=True)
        w2 = jump64(m, b, x1, v1, b1, l + j, j, d2, offsets(b))
        assert int(bufs["epoch"].item()) == 2 and bufs["step_counter"].cpu().tolist()[1] == rs0[1] + 2 * j
        if w2["gap"] > 1e-3:
            assert torch.equal(v2, torch.where(moved_a, w2["v"], v1)) and torch.equal(b2, torch.where(moved_b, w2["bond"], b1))
        assert float((x2.double() - w2["xc"])[moved_a].abs().max()) <= 4 * ulp(w2["big"])


@pytest.mark.parametrize("layout", ["dense", "padded"])
def test_the_jump_with_sample_keys_addresses_rows_like_the_step(layout, monkeypatch):
    """Per-sample keys: every sample draws with its key at the rows of its OWN enumeration -- in a padded batch the bond rows of a
    6-atom ligand inside a width of 9 (`noise_addr`)."""
    monkeypatch.setenv("DD_RAGGED_MODE", "padded")
    m = model(0)
    l, j = 200, 30
    if layout == "dense":
        n_l, n_p = [8, 8], [48, 48]
        b = pair(131)
        mask = scaffold(b)
        keys = KEYS[:2]
    else:
        n_l, singles, b, fx0 = ragged_case("replace")
        n_p, mask, keys = [48, 40, 44], fx0["mask"], KEYS[:3]
        assert BL.fits_padded(BL.BatchLayout(n_p, n_l), m.config.knn)
    for mode in ("replace", "hold"):
        fx = known(b, mask, 132, mode, **(dict(init="given") if mode == "replace" else {}))
        hb = held_bonds(b, mask)
        s, bufs, fxs, rss, _ = prepared(m, b, fx, l, j, sample_keys=keys)
        rows_l = rows_b = None
        if layout == "padded":
            _, rows_l, rows_b = BL.BatchLayout(n_p, n_l).padded_rows()
        x0, v0, b0 = state_of(bufs, rows_l, rows_b)
        device_jump(s, bufs, fxs, rss, True)
        x1, v1, b1 = state_of(bufs, rows_l, rows_b)
        w = jump64(m, b, x0, v0, b0, l, j, keyed_draws(keys, n_l, (l + j) + 65536, jump=True), offsets(b))
        assert w["gap"] > 1e-3, w["gap"]
        moved_a, moved_b = (~mask, ~hb) if mode == "hold" else (torch.ones_like(mask), torch.ones_like(hb))
        assert torch.equal(v1, torch.where(moved_a, w["v"], v0)) and torch.equal(b1, torch.where(moved_b, w["bond"], b0)), (layout, mode)
        assert float((x1.double() - w["xc"])[moved_a].abs().max()) <= 4 * ulp(w["big"])
        assert torch.equal(x1[~moved_a], x0[~moved_a])


# ------------------------------------------------------------------------------------------------ 7: whole chains, oracle loop
def oracle_resample_loop(m, b, fx, t_hi, steps, j, r, seed, start):
    """`oracle_loop` with the schedule: one oracle step per position with that position's device draws (time word
    t + 65536 * epoch), held rows overwritten as the mode says, and `jump64` (epoch + 1, the jump's streams) at every jump."""
    n, nb = b["init_ligand_pos"].shape[0], b["init_ligand_fc_bond_type"].numel()
    off = offsets(b)
    off_l = off[b["batch_ligand"]]
    mask, hb = fx["mask"], held_bonds(b, fx["mask"])
    state = {k: v.clone() for k, v in start.items()}
    out = {k: [] for k in ("pos", "v", "bond", "t")}
    gap, epoch = 9.0, 0
    for op in resample_schedule(t_hi, t_hi - steps + 1, j, r):
        if op[0] == "step":
            t = op[1]
            d = draws(seed, t + 65536 * epoch, n, nb)
            o = oracle_loop(m, b, fx, 1, {k: v[None] for k, v in d.items()}, t, start=state)
            state = dict(pos=o["pos"][0], v=o["v"][0], bond=o["bond"][0])
            gap = min([gap] + o["gap"])
            for k in ("pos", "v", "bond"):
                out[k].append(state[k].clone())
            out["t"].append(t)
        else:
            epoch += 1
            d = draws(seed, op[2] + 65536 * epoch, n, nb, jump=True)
            w = jump64(m, b, (state["pos"].float() - off_l), state["v"], state["bond"], op[1], j, d, off)
            gap = min(gap, w["gap"])
            pos2 = (w["xc"] + off_l.double()).float()
            if fx["mode"] == "hold":
                pos2[mask], w["v"][mask], w["bond"][hb] = state["pos"][mask], state["v"][mask], state["bond"][hb]
            state = dict(pos=pos2, v=w["v"], bond=w["bond"])
    return {k: (torch.stack(v) if k != "t" else v) for k, v in out.items()}, gap


@functools.lru_cache(maxsize=None)
def chain_case(which):
    m, b = model(0), pair(141)
    T, seed = m.num_timesteps, 4321
    mask = scaffold(b)
    hb = held_bonds(b, mask)
    if which == "low":                                                          # t = 5 .. 0: the jump out of the clean level
        fx = known(b, mask, 142, "replace", init="given")
        t_hi = 5
        start = dict(pos=b["init_ligand_pos"].clone(), v=b["init_ligand_v"].clone(), bond=b["init_ligand_fc_bond_type"].clone())
    else:
        fx = known(b, mask, 142, which)
        t_hi = T - 1
        start = dict(pos=b["init_ligand_pos"].clone(), v=b["init_ligand_v"].clone(), bond=b["init_ligand_fc_bond_type"].clone())
        if which == "replace":                                                  # init='draw': level T - 1 at Philox time T, epoch 0
            d0 = draws(seed, T, 16, 112)
            lv = forward_level(m, b, fx, T - 1, d0["u_v"], d0["u_b"], d0["eps"], offsets(b))
            off_l = offsets(b)[b["batch_ligand"]].double()
            start["pos"][mask], start["v"][mask], start["bond"][hb] = (lv["xc"] + off_l)[mask].float(), lv["v"][mask], lv["bond"][hb]
    got = rrun(m, b, 6, seed=seed, fixed=fx, resample=RS, start_step=T - 1 - t_hi)
    want, gap = oracle_resample_loop(m, b, fx, t_hi, 6, 2, 2, seed, start)
    return m, b, fx, got, want, gap, t_hi


@pytest.mark.parametrize("which", ["hold", "replace", "low"])
def test_whole_chain_against_the_oracle_loop_with_the_schedule(which):
    m, b, fx, got, want, gap, t_hi = chain_case(which)
    assert got["t_traj"].tolist() == want["t"] == times(t_hi, 6) and len(want["t"]) == 12
    assert all(got[k].shape[0] == 12 for k in TRAJ)
    assert gap > 1e-3, gap
    assert torch.equal(got["v_traj"], want["v"]) and torch.equal(got["bond_traj"], want["bond"])
    err = maxabs(got["pos_traj"], want["pos"])
    print(f"\nRESAMPLE {which}: all rows vs oracle loop over 12 positions and 3 jumps, max |dpos| {err:.3g} (tol {POS_TOL:g})")
    assert err < POS_TOL
    assert torch.equal(got["pos"], got["pos_traj"][-1]) and torch.equal(got["v"], got["v_traj"][-1])
    if which == "low":                                                          # the last step runs at t = 0: the clean values
        mask, hb = fx["mask"], held_bonds(b, fx["mask"])
        assert torch.equal(got["v"][mask], fx["v"][mask]) and torch.equal(got["bond"][hb], fx["bond"][hb])


# ------------------------------------------------------------------------------------------------ 8: revisits draw afresh
def test_revisited_times_draw_afresh():
    m, b, fx, got, _, _, _ = chain_case("replace")
    mask = fx["mask"]
    tt = got["t_traj"].tolist()
    assert tt[0] == tt[2] and tt[4] == tt[6]
    for p, q in ((0, 2), (1, 3), (4, 6), (5, 7), (8, 10)):
        assert tt[p] == tt[q] and not torch.equal(got["pos_traj"][p][mask], got["pos_traj"][q][mask]), (p, q)
        assert not torch.equal(got["pos_traj"][p][~mask], got["pos_traj"][q][~mask]), (p, q)
    m, b, fx, got, _, _, _ = chain_case("hold")
    mask, hb = fx["mask"], held_bonds(b, fx["mask"])
    for p in range(12):
        assert torch.equal(got["pos_traj"][p][mask], got["pos_traj"][0][mask]), p
    assert bool((got["v_traj"][:, mask] == fx["v"][mask]).all()) and bool((got["bond_traj"][:, hb] == fx["bond"][hb]).all())
    off_l = offsets(b)[b["batch_ligand"]]
    assert torch.equal(got["pos"][mask], ((fx["pos"] - off_l) + off_l)[mask])
    assert not torch.equal(got["pos_traj"][0][~mask], got["pos_traj"][2][~mask])


# ------------------------------------------------------------------------------------------------ 9: compositions
@pytest.mark.parametrize("mode", ["hold", "replace"])
def test_eager_captured_and_captured_without_trajectories_agree(mode):
    m, b = model(0), pair(151)
    fx = known(b, scaffold(b), 152, mode)
    streamed = rrun(m, b, 6, seed=9, fixed=fx, resample=RS)                      # captured graph, trajectories streamed
    assert streamed["t_traj"].tolist() == times(m.num_timesteps - 1, 6) and streamed["pos_traj"].shape[0] == 12
    assert_same(rrun(m, b, 6, seed=9, fixed=fx, resample=RS, use_graph=False), streamed, "eager launches")
    bare = rrun(m, b, 6, seed=9, fixed=fx, resample=RS, keep_traj=False)
    assert_same(bare, {k: streamed[k] for k in ("pos", "v", "bond", "t_traj")}, "captured, no trajectories")
    assert not torch.equal(streamed["pos"], run(m, b, 6, seed=9, fixed=fx)["pos"])   # the jumps did something


@pytest.mark.parametrize("mode", ["hold", "replace"])
def test_padded_batch_with_masks_and_keys_equals_each_sample_alone(mode, monkeypatch):
    monkeypatch.setenv("DD_RAGGED_MODE", "padded")
    m = model(0)
    n_l, singles, b, fx = ragged_case(mode)
    keys = KEYS[:3]
    alone = [without_t(rrun(m, s, 6, seed=k, fixed=fixed_rows(fx, n_l, i), resample=RS)) for i, (s, k) in enumerate(zip(singles, keys))]
    whole = rrun(m, b, 6, sample_keys=keys, fixed=fx, resample=RS)
    assert whole["t_traj"].tolist() == times(m.num_timesteps - 1, 6)
    parts = split(without_t(whole), n_l)
    for i in range(3):
        assert_same(parts[i], alone[i], f"{mode}, sample {i}")
    order = [2, 0, 1]
    b2 = synth.concat_sampling_batches([singles[i] for i in order])
    fx2 = {k: torch.cat([fixed_rows(fx, n_l, i)[k] for i in order]) for k in ("mask", "pos", "v", "bond")}
    fx2["mode"] = mode
    parts = split(without_t(rrun(m, b2, 6, sample_keys=[keys[i] for i in order], fixed=fx2, resample=RS)), [n_l[i] for i in order])
    for p, i in enumerate(order):
        assert_same(parts[p], alone[i], f"{mode}, sample {i} at position {p}")


@pytest.mark.parametrize("mode", ["hold", "replace"])
def test_grouped_route_equals_the_padded_route(mode, monkeypatch):
    m = model(0)
    n_l, singles, b, fx = ragged_case(mode)
    b = synth.concat_sampling_batches(singles + [single(6, 70)])               # two samples share a size group
    fx = known(b, torch.cat([fx["mask"], torch.tensor([True, False, True, False, False, True])]), 162, mode)
    keys = KEYS[:4]
    monkeypatch.setenv("DD_RAGGED_MODE", "padded")
    want = rrun(m, b, 6, sample_keys=keys, fixed=fx, resample=RS)
    assert want["pos_traj"].shape[0] == 12
    for concurrent in ("0", "1"):
        monkeypatch.setenv("DD_RAGGED_MODE", "groups")
        monkeypatch.setenv("DD_RAGGED_CONCURRENT", concurrent)
        assert_same(rrun(m, b, 6, sample_keys=keys, fixed=fx, resample=RS), want, f"{mode}, groups (concurrent {concurrent})")


# ------------------------------------------------------------------------------------------------ 10: one graph for every (j, r)
def test_cached_graph_serves_other_jump_lengths_but_not_the_plain_chain(monkeypatch):
    m, b = model(0), pair(171)
    fx = known(b, scaffold(b), 172, "replace")
    monkeypatch.setenv("DD_CHAIN_CACHE", "1")
    m._evict_chain_cache(0)
    ra = rrun(m, b, 6, seed=1, fixed=fx, resample=RS)
    assert len(m._chain_cache) == 1
    ent = next(iter(m._chain_cache.values()))
    graph, graph_id = ent["graph"].value, ent["graph_id"]
    assert graph and ent["fixed"] == "replace" and ent["resample"]["j"] == 2
    rb = rrun(m, b, 6, seed=1, fixed=fx, resample=dict(jump_length=3, n_resample=2))
    assert len(m._chain_cache) == 1 and next(iter(m._chain_cache.values())) is ent
    assert ent["graph"].value == graph and ent["graph_id"] == graph_id          # the very graph, replayed
    assert rb["t_traj"].tolist() == times(m.num_timesteps - 1, 6, 3, 2) and rb["pos_traj"].shape[0] == 12
    assert_same(rb, rrun(m, b, 6, seed=1, fixed=fx, resample=dict(jump_length=3, n_resample=2), use_graph=False), "j = 3, eager")
    assert_same(ra, rrun(m, b, 6, seed=1, fixed=fx, resample=RS, use_graph=False), "j = 2, eager")
    assert not torch.equal(ra["pos"], rb["pos"])
    ro = run(m, b, 6, seed=1, fixed=fx)                                         # without resample: captured again
    ent = next(iter(m._chain_cache.values()))
    assert len(m._chain_cache) == 1 and ent["graph_id"] != graph_id and not ent["resample"]
    assert_same(ro, run(m, b, 6, seed=1, fixed=fx, use_graph=False), "plain, eager")
    m._evict_chain_cache(0)


# ------------------------------------------------------------------------------------------------ 11: statistics of the jump
def test_jump_statistics_with_device_noise():
    """B = 8, NL = 64: 14 jumps 400 -> 600 from one prepared state, each at an epoch of its own (the run state is reset in between, the
    epoch is not).  21 504 normals: the standardised residual (x' - A (x - cc) - cc) / (S std) has |mean| <= 4 / sqrt(n) and
    |var - 1| <= 4 sqrt(2 / n); 451 584 bond rows and 7 168 atom rows: of the rows that start in class c the fraction that stays is
    within 4 sqrt(p (1 - p) / n) of p = exp(lr) + (1 - exp(lr)) prior_c.  Deterministic: a failure is a bias, not a seed."""
    m = model(0)
    lib = hip_lib.load()
    torch.manual_seed(181)
    pocket = synth.make_pocket_tiny(182, num_protein=72, arm_atoms=(24, 24), scaffold_atoms=16)
    b = synth.build_sampling_batch(pocket, 8)
    n, nb = 8 * 64, 8 * 64 * 63
    assert b["init_ligand_pos"].shape[0] == n and b["init_ligand_fc_bond_type"].numel() == nb
    l, j, jumps = 400, 200, 14
    fx = known(b, torch.zeros(n, dtype=torch.bool), 183, "replace", init="given")
    s, bufs, fxs, rss, _ = prepared(m, b, fx, l, j, seed=184)
    x0, v0, b0 = state_of(bufs)
    keep = {k: bufs[k].clone() for k in ("lig_pos", "lig_v", "lig_bond")}
    w = jump64(m, b, x0, v0, b0, l, j, dict(u_v=torch.full((n, 8), 0.5), u_b=torch.full((nb, 5), 0.5), eps=torch.zeros(n, 3)), offsets(b))
    res, stay_v, stay_b = [], torch.zeros(8), torch.zeros(5)
    for e in range(jumps):
        for k, t in keep.items():
            bufs[k].copy_(t)
        hip_lib.check(lib.dd_sampler_reset(ctypes.byref(s), hip_lib.stream_ptr()), "dd_sampler_reset")
        device_jump(s, bufs, fxs, rss, False)
        assert int(bufs["epoch"].item()) == e + 1
        x1, v1, b1 = state_of(bufs)
        res.append(((x1.double() - (w["A"] * (x0.double() - w["cc"]) + w["cc"])) / (w["S"] * w["std"])).reshape(-1))
        stay_v += torch.bincount(v0[v1 == v0], minlength=8)
        stay_b += torch.bincount(b0[b1 == b0], minlength=5)
    res = torch.cat(res)
    nn = res.numel()
    assert nn >= 20000 and jumps * nb >= 30000
    mean, var = float(res.mean()), float(res.var(unbiased=False))
    print(f"\nJUMP statistics: n {nn}, residual mean {mean:+.4f} (bound {4 / math.sqrt(nn):.4f}), var {var:.4f} "
          f"(bound {4 * math.sqrt(2 / nn):.4f})")
    assert abs(mean) <= 4 / math.sqrt(nn) and abs(var - 1) <= 4 * math.sqrt(2 / nn)
    for name, start, stay, p in (("bond", b0, stay_b, w["stay_b"]), ("atom", v0, stay_v, w["stay_v"])):
        cnt = torch.bincount(start, minlength=stay.numel()).double() * jumps
        for c in range(stay.numel()):
            if cnt[c] == 0:
                continue
            f, pc = float(stay[c] / cnt[c]), float(p[c])
            bound = 4 * math.sqrt(pc * (1 - pc) / float(cnt[c]))
            print(f"JUMP statistics: {name} class {c}: {int(cnt[c])} rows, stay {f:.4f} vs p {pc:.4f} (bound {bound:.4f})")
            assert abs(f - pc) <= bound, (name, c, f, pc, bound)


# ------------------------------------------------------------------------------------------------ 12: the harness
def test_harness_with_resample_returns_the_scaffold_and_n_total_positions():
    m = model(0)
    f = GU.make_pocket_fields(5)
    data = pocket_data.PocketData(**{k: f[k] for k in ("protein_pos", "protein_element", "protein_is_backbone", "protein_atom_to_aa_type",
                                                       "pocket_atom_masks", "num_arms", "num_scaffold", "arms_prior", "scaffold_prior",
                                                       "ligand_atom_mask", "ligand_pos", "full_protein_pos")})
    decomp, ref_pos = data.ligand_atom_mask, data.ligand_pos
    n = decomp.numel()
    sca = decomp == -1
    g = torch.Generator().manual_seed(91)
    ref_v, ref_b = torch.randint(0, 8, (n,), generator=g), torch.randint(0, 5, (n * (n - 1),), generator=g)
    fixed_fn = lambda index, d: dict(mask=d == -1, pos=ref_pos, v=ref_v, bond=ref_b)
    T = m.num_timesteps
    torch.manual_seed(92)
    # `replace` returns the clean scaffold only from the step at t = 0: the whole chain, one jump point (600 <= T - 1 < 1200)
    rs = dict(jump_length=600, n_resample=2)
    out = harness.sample_diffusion_ligand_decomp(m, data, num_samples=2, batch_size=2, device=dev(), num_steps=T, prior_mode="subpocket",
                                                 num_atoms_mode="ref", sample_key_seed=5, fixed_fn=fixed_fn, fixed_mode="replace",
                                                 resample=rs)
    n_total = T + 1 * 600 * (T // 600)
    assert len(out["pred_pos"]) == 2 and n_total == 1600
    off = data.protein_pos.mean(0)
    bound = ulp(max(float(ref_pos[sca].abs().max()), float((ref_pos - off)[sca].abs().max())))
    fc = out["pred_bond_index"][0]
    hb = sca[torch.from_numpy(fc[0])] & sca[torch.from_numpy(fc[1])]
    for k in range(2):
        for key in ("pred_pos_traj", "pred_v_traj", "pred_v0_traj", "pred_vt_traj", "pred_b_traj", "pred_bt_traj"):
            assert len(out[key][k]) == n_total, key
        assert torch.equal(torch.from_numpy(out["pred_v"][k])[sca], ref_v[sca])
        assert torch.equal(torch.from_numpy(out["pred_bond_type"][k])[hb], ref_b[hb])
        diff = float((torch.from_numpy(out["pred_pos"][k]).float() - ref_pos)[sca].abs().max())
        assert diff <= bound, (k, diff, bound)
        # ... and it was noised on the way: at the first position the held scaffold is far from its clean coordinates
        assert float((torch.from_numpy(out["pred_pos_traj"][k][0]).float() - ref_pos)[sca].abs().max()) > 0.1
    assert not torch.equal(torch.from_numpy(out["pred_pos"][0])[~sca], torch.from_numpy(out["pred_pos"][1])[~sca])
