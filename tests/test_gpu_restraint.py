"""Distance restraints (the ``restraint`` entry of ``energy_drift_opt``; dd_drift_restraint, dd_sample_steps_guided /
dd_graph_create_guided) on the GPU.

1. The kernel through the C ABI at the cases of tests/restraint_cases.py against the gradient of the energy under float64 autograd
   (bounds from the float64 / fp32 oracle pair, never from the kernel), with dist / winner, accumulate = 0 onto NaN and = 1 onto a
   known buffer, and the refusals.
2. The time window: exact zeros outside, both edges inside.
3. One reverse step of the sampler: positions = the same call without the term minus the float64 gradient (times pos_score_coef[t]
   with ``scale``), within 4 ulp of the largest coordinate; also beside armsca_prox.
4. Compositions by ``torch.equal`` on chains of 6 steps at the small shapes of the per-sample-key tests.
5. The harness: ``restraints_fn`` with ``init="device"`` gives the same sample under batch sizes 1 and 3."""
import ctypes
import math

import pytest
import torch

import restraint_cases as RC
from decompdiff_amd import DecompScorePosNet3D, RESTRAINT_ANY, harness, hip_lib, synth
from test_gpu_parity import _sample_hip, dev, maxabs, model
from test_gpu_sample_keys import KEYS, POCKETS, TRAJ, assert_same, single, split

pytestmark = pytest.mark.gpu
CASES = RC.all_cases()


def ulp(x):
    return 2.0 ** (math.floor(math.log2(x)) - 23)


# ------------------------------------------------------------------------------------------------ 1: the kernel
def launch(case, out, accumulate, dist=None, winner=None, run_state=None, t_min=0, t_max=999, NL=None, decomp="case", R=None):
    """dd_drift_restraint on the case -> status (synchronised).  run_state: (steps done, t_start) or None."""
    lib, d = hip_lib.load(), dev()
    i32 = lambda t: t.to(device=d, dtype=torch.int32).contiguous()
    f32 = lambda t: t.to(device=d, dtype=torch.float32).contiguous()
    x = f32(case["pos"])
    dec = case["decomp"] if decomp == "case" else decomp
    dec = None if dec is None else i32(dec)
    nlr = None if case["nl_real"] is None else i32(torch.tensor(case["nl_real"]))
    arrays = [i32(case["ptr"]), f32(case["point"]), f32(case["min_d"]), f32(case["max_d"]), f32(case["weight"]), i32(case["atom"]),
              i32(case["group"])]
    rs = hip_lib.restraints_struct(case["R"] if R is None else R, *arrays, False, t_min, t_max)
    ctr = None if run_state is None else i32(torch.tensor([run_state[0], run_state[1], 0, 0]))
    rc = lib.dd_drift_restraint(hip_lib.ptr(x), hip_lib.ptr(dec), hip_lib.ptr(nlr), case["B"], case["NL"] if NL is None else NL,
                                ctypes.byref(rs), hip_lib.ptr(ctr), hip_lib.ptr(out), accumulate, hip_lib.ptr(dist), hip_lib.ptr(winner),
                                hip_lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("name", RC.NAMES)
def test_kernel_vs_float64_autograd(name):
    case, ref = CASES[name], RC.reference(name)
    n, R = case["B"] * case["NL"], case["R"]
    out = torch.full((n, 3), float("nan"), device=dev())                 # accumulate = 0 must write every row
    dist = torch.full((R,), float("nan"), device=dev())
    win = torch.full((R,), -7, dtype=torch.int32, device=dev())
    hip_lib.check(launch(case, out, 0, dist, win), name)
    buf = RC.known_buffer(name, (n, 3))
    acc = buf.to(dev()).contiguous()                                     # accumulate = 1 adds onto what is there
    hip_lib.check(launch(case, acc, 1), name)
    out, acc, dist, win = out.cpu(), acc.cpu(), dist.cpu(), win.cpu().long()
    finite = bool(torch.isfinite(out).all()) and bool(torch.isfinite(acc).all())
    err = maxabs(out, ref["g64"]) if finite else float("nan")
    err_acc = maxabs(acc, buf.double() + ref["g64"]) if finite else float("nan")
    bnd = ref["bound"]
    bnd_acc = bnd + float(buf.abs().max()) * 2.0 ** -23                  # buffer + gradient is rounded once more, at the buffer's size
    fin = torch.isfinite(ref["dist"])
    err_d = maxabs(dist[fin], ref["dist"][fin]) if bool(fin.any()) else 0.0
    bnd_d = RC.dist_bound(ref)
    RC.report(name, err, ref["d32"], bnd, f" err_acc={err_acc:.3g} bound_acc={bnd_acc:.3g} err_dist={err_d:.3g} bound_dist={bnd_d:.3g} "
                                          f"|g|={float(ref['g64'].abs().max()):.3g} R={R}")
    assert finite, (name, out[~torch.isfinite(out).all(1)][:4])
    assert err < bnd, (name, err, bnd)
    assert err_acc < bnd_acc, (name, err_acc, bnd_acc)
    assert torch.equal(win, ref["winner"]), (name, win, ref["winner"])
    assert err_d <= bnd_d, (name, err_d, bnd_d)
    assert bool(torch.isinf(dist[~fin]).all()) and bool((dist[~fin] > 0).all())       # an empty group: +inf (and winner -1 above)
    NL = case["NL"]
    if "empty_sample" in case:                                            # a sample without restraints: zeros over the NaN
        rows = slice(case["empty_sample"] * NL, (case["empty_sample"] + 1) * NL)
        assert torch.equal(out[rows], torch.zeros(NL, 3)) and torch.equal(acc[rows], buf[rows])
    if case["nl_real"] is not None:                                       # padding rows: zeros, never a gradient
        for b, nr in enumerate(case["nl_real"]):
            assert torch.equal(out[b * NL + nr:(b + 1) * NL], torch.zeros(NL - nr, 3)), (name, b)
    if "expect" in case:
        assert maxabs(out, torch.tensor(case["expect"], dtype=torch.float64)) < bnd, (name, out)


def test_runs_are_bitwise_reproducible():
    case = CASES["random_nl128_b3"]
    outs = []
    for _ in range(3):
        out = torch.full((case["B"] * case["NL"], 3), float("nan"), device=dev())
        hip_lib.check(launch(case, out, 0), "dd_drift_restraint")
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_bad_arguments_are_refused_and_nothing_is_written():
    case = CASES["groups_b3"]
    n = case["B"] * case["NL"]

    def refused(**kw):
        out = torch.full((kw.pop("rows", n), 3), 7.0, device=dev())
        rc = launch(kw.pop("case", case), out, 0, **kw)
        return rc == -1 and bool((out == 7.0).all())
    big = dict(case, NL=129, pos=torch.zeros(3 * 129, 3), decomp=torch.zeros(3 * 129, dtype=torch.long))
    assert refused(case=big, rows=3 * 129)                                # NL = 129
    assert refused(decomp=None)                                           # scaffold / arm groups without decomp
    assert refused(case=dict(case, atom=torch.where(case["atom"] >= 0, torch.full_like(case["atom"], 6), case["atom"])))   # atom == NL
    assert refused(case=dict(case, atom=torch.full_like(case["atom"], -2)))
    assert refused(case=dict(case, group=torch.full_like(case["group"], -2)))
    assert refused(R=case["R"] - 1) and refused(R=case["R"] + 1)          # ptr does not end at R
    assert refused(case=dict(case, ptr=torch.tensor([0, 9, 8, 9])))       # ptr not monotone
    assert refused(t_min=5, t_max=4)
    out = torch.full((n, 3), 7.0, device=dev())
    hip_lib.check(launch(case, out, 0), "the case itself")
    assert not bool((out == 7.0).any())


# ------------------------------------------------------------------------------------------------ 2: the time window
@pytest.mark.parametrize("name", ["random_nl65_b3", "hinge_values"])
def test_time_window_reads_the_run_state(name):
    case, ref = CASES[name], RC.reference(name)
    n = case["B"] * case["NL"]
    t_min, t_max = 200, 600

    def at(t, steps, accumulate=0):
        out = torch.full((n, 3), float("nan"), device=dev()) if not accumulate else RC.known_buffer(name, (n, 3)).to(dev())
        dist = torch.full((case["R"],), float("nan"), device=dev())
        hip_lib.check(launch(case, out, accumulate, dist, None, run_state=(steps, t + steps), t_min=t_min, t_max=t_max), name)
        return out.cpu(), dist.cpu()
    always = torch.full((n, 3), float("nan"), device=dev())
    hip_lib.check(launch(case, always, 0), name)
    always = always.cpu()
    assert float(always.abs().max()) > 0.1
    for t, steps in ((400, 0), (400, 599), (200, 3), (600, 0)):           # inside, and both edges
        out, dist = at(t, steps)
        assert torch.equal(out, always), (name, t)
    for t, steps in ((199, 0), (601, 2), (0, 999), (999, 0)):             # outside: exact zeros over the NaN, dist still reported
        out, dist = at(t, steps)
        assert torch.equal(out, torch.zeros(n, 3)), (name, t)
        fin = torch.isfinite(ref["dist"])
        assert maxabs(dist[fin], ref["dist"][fin]) <= RC.dist_bound(ref)
        acc, _ = at(t, steps, accumulate=1)
        assert torch.equal(acc, RC.known_buffer(name, (n, 3)))            # accumulate = 1 adds the zeros


# ------------------------------------------------------------------------------------------------ 3: one reverse step
def armsca_gradient(case, min_d, max_d):
    lib = hip_lib.load()
    x = case["pos"].to(dev()).contiguous()
    dec = case["decomp"].to(device=dev(), dtype=torch.int32).contiguous()
    out = torch.zeros_like(x)
    hip_lib.check(lib.dd_drift_armsca(hip_lib.ptr(x), hip_lib.ptr(dec), case["B"], case["NL"], min_d, max_d, hip_lib.ptr(out), 0,
                                      hip_lib.stream_ptr()), "dd_drift_armsca")
    torch.cuda.synchronize()
    return out.cpu().double()


@pytest.mark.parametrize("variant", ["alone", "scaled", "with_armsca"])
def test_one_reverse_step_subtracts_the_gradient(variant):
    b, entry, case = RC.sampler_case(scale=variant == "scaled")
    m, t = model(0), 500
    h, w = RC.margins(case)
    assert h >= RC.HINGE_MARGIN and w >= RC.WINNER_MARGIN and RC.same_branches(case)
    g64 = RC.grad(case, torch.float64)[0]
    assert float(g64.abs().max()) > 0.3
    noise = synth.draw_step_noise(1, b["init_ligand_pos"].size(0), b["init_ligand_fc_bond_type"].size(0))
    armsca = [dict(type="armsca_prox", min_d=1.2, max_d=1.9)] if variant == "with_armsca" else []
    plain = _sample_hip(m, b, 1, None, noise, t)
    got = _sample_hip(m, b, 1, armsca + [entry], noise, t)
    want = plain["pos"].cpu().double() - g64 * (float(m.pos_score_coef[t]) if variant == "scaled" else 1.0)
    if armsca:
        want = want - armsca_gradient(case, 1.2, 1.9)
    big = max(float(plain["pos"].abs().max()), float(got["pos"].abs().max()))
    err, tol = maxabs(got["pos"], want), 4.0 * ulp(big)
    print(f"\nRESTRAINT step {variant}: err={err:.3g} tol={tol:.3g} (largest coordinate {big:.3g}) |g|={float(g64.abs().max()):.3g} "
          f"coef={float(m.pos_score_coef[t]):.3g}")
    assert err <= tol, (variant, err, tol)
    assert torch.equal(got["v"], plain["v"]) and torch.equal(got["bond"], plain["bond"])
    # dist / winner of the final state, in the CALLER's restraint order, against the oracle on the positions that came back
    fin = RC.centred_case(b, entry, pos=got["pos"].cpu())
    _, dist, win, _ = RC.grad(fin, torch.float64)
    flat = torch.tensor([wr + int(s) * fin["NL"] if wr >= 0 else -1 for wr, s in zip(win, fin["sample"])])
    assert torch.equal(got["restraint_atom"][fin["order"]], flat)
    assert maxabs(got["restraint_dist"][fin["order"]], torch.tensor(dist)) < 1e-4     # (the offset is re-added and re-subtracted: POS_TOL)


# ------------------------------------------------------------------------------------------------ 4: compositions
STEPS = 6


def sub_entry(entry, k, n_l):
    """Sample k's share of an entry over samples of n_l[b] atoms, as an entry for that sample alone."""
    keep = (entry["sample"] == k).nonzero()[:, 0]
    a0 = sum(n_l[:k])
    e = {key: (v[keep] if torch.is_tensor(v) else v) for key, v in entry.items()}
    e["sample"] = torch.zeros_like(e["sample"])
    e["atom"] = torch.where(e["atom"] >= 0, e["atom"] - a0, e["atom"])
    return e


def run_rs(m, b, entry, steps=STEPS, center_pos_mode="protein", **kw):
    r = m.sample_diffusion(num_steps=steps, center_pos_mode=center_pos_mode, energy_drift_opt=None if entry is None else [entry],
                           **{k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in b.items()}, **kw)
    out = {k: r[k].cpu() for k in ("pos", "v", "bond")}
    out.update({k: torch.stack(r[k]) for k in TRAJ if len(r[k])})
    return out, r


def pair(seed, nl=8):
    torch.manual_seed(seed)
    return synth.build_sampling_batch(POCKETS[nl], 2)


def test_eager_captured_and_streamed_agree_and_the_term_acts(monkeypatch):
    m, b = model(0), pair(31)
    e = RC.batch_entry(b, 31, weight=(0.1, 0.3), scale=True)
    eager, _ = run_rs(m, b, e, seed=5, use_graph=False)
    streamed, _ = run_rs(m, b, e, seed=5, use_graph=True)
    monkeypatch.setenv("DD_TRAJ_STREAMING", "0")
    captured, _ = run_rs(m, b, e, seed=5, use_graph=True)
    monkeypatch.delenv("DD_TRAJ_STREAMING")
    assert_same(captured, eager, "captured")
    assert_same(streamed, eager, "streamed")
    notraj, _ = run_rs(m, b, e, seed=5, use_graph=True, keep_traj=False)
    assert torch.equal(notraj["pos"], eager["pos"])
    none, _ = run_rs(m, b, None, seed=5)
    assert maxabs(none["pos"], eager["pos"]) > 1e-3 and all(k in eager for k in TRAJ)      # (scaled by pos_score_coef near t = T: small, not rounding)
    # R = 0: bit for bit the call without the entry
    empty = dict(type="restraint", sample=torch.zeros(0, dtype=torch.long), point=torch.zeros(0, 3), min_d=0.0, max_d=1.0)
    for use_graph in (False, True):
        zero, r = run_rs(m, b, empty, seed=5, use_graph=use_graph)
        assert_same(zero, none, "R = 0")
        assert r["restraint_dist"].shape == (0,) and r["restraint_atom"].shape == (0,)


def test_padded_grouped_and_alone_agree(monkeypatch):
    """Ligands of 9 and 8 atoms (the second is padded by one atom) and 6: as one padded batch, as size groups, and each sample alone
    in its own dense batch -- the same chain per sample, the same restraint results."""
    m = model(0)
    n_l = [9, 8, 6]
    singles = [single(n, 300 + k) for k, n in enumerate(n_l)]
    batch = synth.concat_sampling_batches(singles)
    e = RC.batch_entry(batch, 32, per_sample=(3, 4, 2), weight=(0.1, 0.3))
    keys = KEYS[:3]
    alone = [run_rs(m, s, sub_entry(e, k, n_l), seed=keys[k]) for k, s in enumerate(singles)]
    padded, rp = run_rs(m, batch, e, sample_keys=keys)
    monkeypatch.setenv("DD_RAGGED_MODE", "groups")
    grouped, rg = run_rs(m, batch, e, sample_keys=keys)
    monkeypatch.delenv("DD_RAGGED_MODE")
    for what, got, r in (("padded", padded, rp), ("grouped", grouped, rg)):
        for k, part in enumerate(split(got, n_l)):
            assert_same(part, alone[k][0], f"{what}, sample {k}")
            mine = (e["sample"] == k).nonzero()[:, 0]
            a0 = sum(n_l[:k])
            ra = r["restraint_atom"][mine]
            assert torch.equal(r["restraint_dist"][mine], alone[k][1]["restraint_dist"]), (what, k)
            assert torch.equal(torch.where(ra >= 0, ra - a0, ra), alone[k][1]["restraint_atom"]), (what, k)
    assert bool((rp["restraint_atom"] >= 0).all()) and bool(torch.isfinite(rp["restraint_dist"]).all())
    assert maxabs(padded["pos"], run_rs(m, batch, None, sample_keys=keys)[0]["pos"]) > 1e-2


def test_a_keyed_sample_with_its_restraints_in_a_batch_of_three_is_that_sample_alone():
    m = model(0)
    singles = [single(8, 310 + k) for k in range(3)]
    batch = synth.concat_sampling_batches(singles)
    e = RC.batch_entry(batch, 33, per_sample=(0, 4, 3), weight=(0.1, 0.3), t_min=996)       # sample 0 has none
    got, _ = run_rs(m, batch, e, sample_keys=KEYS[:3])
    for k, part in enumerate(split(got, [8] * 3)):
        alone, _ = run_rs(m, singles[k], sub_entry(e, k, [8] * 3), seed=KEYS[k])
        assert_same(part, alone, f"sample {k}")
    plain0, _ = run_rs(m, singles[0], None, seed=KEYS[0])
    assert_same(split(got, [8] * 3)[0], plain0, "the sample without restraints")


def test_a_split_chain_is_the_unsplit_one():
    """(center_pos_mode='none', as test_resumed_chain_is_the_unsplit_chain: re-adding and re-subtracting the frame offset between the
    calls would cost an ulp)"""
    m, b = model(0), pair(34)
    e = RC.batch_entry(b, 34, weight=(0.1, 0.3), t_min=996, t_max=998)    # the window opens after the first step and closes inside the second half
    kw = dict(seed=9, center_pos_mode="none")
    full, _ = run_rs(m, b, e, **kw)
    first, _ = run_rs(m, b, e, steps=3, **kw)
    b2 = dict(b, init_ligand_pos=first["pos"], init_ligand_v=first["v"], init_ligand_fc_bond_type=first["bond"])
    second, _ = run_rs(m, b2, e, steps=3, start_step=3, **kw)
    for k in ("pos", "v", "bond"):
        assert torch.equal(second[k], full[k]), k
    for k in TRAJ:
        assert torch.equal(torch.cat([first[k], second[k]]), full[k]), k
    always, _ = run_rs(m, b, dict(e, t_min=None, t_max=None), **kw)
    plain, _ = run_rs(m, b, None, **kw)
    assert torch.equal(full["pos_traj"][0], plain["pos_traj"][0]) and not torch.equal(always["pos_traj"][0], plain["pos_traj"][0])   # t = 999: outside
    assert not torch.equal(full["pos_traj"][1], plain["pos_traj"][1])                                                          # t = 998: inside


@pytest.mark.parametrize("resample", [None, dict(jump_length=2, n_resample=2)], ids=["hold", "hold_resampled"])
def test_with_fixed_atoms_held_rows_keep_their_bits(resample):
    m, b = model(0), pair(35)
    mask = b["ligand_decomp_index"] == -1
    g = torch.Generator().manual_seed(35)
    n, nb = b["init_ligand_pos"].shape[0], b["init_ligand_fc_bond_type"].numel()
    fx = dict(mask=mask, pos=b["prior_centers"][b["ligand_decomp_batch"]] + 0.8 * torch.randn(n, 3, generator=g),
              v=torch.randint(0, 8, (n,), generator=g), bond=torch.randint(0, 5, (nb,), generator=g), mode="hold")
    e = RC.batch_entry(b, 35, weight=(0.1, 0.3))                          # (its scaffold restraints target held atoms)
    kw = dict(seed=3, fixed=fx) if resample is None else dict(seed=3, fixed=fx, resample=resample)
    with_rs, _ = run_rs(m, b, e, **kw)
    without, _ = run_rs(m, b, None, **kw)
    eager, _ = run_rs(m, b, e, use_graph=False, **kw)
    assert_same(with_rs, eager, "captured = eager")
    for k in ("pos", "v", "pos_traj", "v_traj"):
        sel = (lambda t: t[:, mask]) if k.endswith("traj") else (lambda t: t[mask])
        assert torch.equal(sel(with_rs[k]), sel(without[k])), k
    assert maxabs(with_rs["pos"][~mask], without["pos"][~mask]) > 1e-3
    assert with_rs["pos_traj"].shape[0] == (STEPS if resample is None else STEPS + 2 * (STEPS // 2))


def test_other_restraint_values_replay_the_cached_graph():
    m, b = model(0), pair(36)
    e1 = RC.batch_entry(b, 36, weight=(0.1, 0.3))
    e2 = RC.batch_entry(b, 37, per_sample=(2, 5), weight=(0.2, 0.4))      # other values, another split over the samples, same capacity
    run_rs(m, b, e1, seed=1)
    n_entries, n_graphs = len(DecompScorePosNet3D._chain_cache), DecompScorePosNet3D._graph_counter
    got, _ = run_rs(m, b, e2, seed=2)
    assert len(DecompScorePosNet3D._chain_cache) == n_entries and DecompScorePosNet3D._graph_counter == n_graphs
    eager, _ = run_rs(m, b, e2, seed=2, use_graph=False)
    assert_same(got, eager, "replayed graph")
    assert not torch.equal(got["pos"], run_rs(m, b, e1, seed=2)[0]["pos"])


# ------------------------------------------------------------------------------------------------ 5: the harness
def test_harness_restraints_fn_gives_the_same_sample_under_any_batch_size():
    m, pocket = model(0), POCKETS[8]
    centre = torch.from_numpy(pocket.prior_centers).float().mean(0)

    def fn(g, dec):
        gen = torch.Generator().manual_seed(1000 + g)
        if g == 1:
            return None
        return dict(point=centre + torch.randn(3, 3, generator=gen), min_d=0.5, max_d=torch.tensor([1.0, 1.5, math.inf]),
                    weight=0.2, atom=torch.tensor([int(dec.numel()) - 1, -1, -1]), group=torch.tensor([RESTRAINT_ANY, -1, 0]))
    job = lambda bs: harness.sample_diffusion_ligand_decomp(m, pocket, num_samples=3, batch_size=bs, device="cuda:0", num_steps=3,
                                                            init="device", sample_key_seed=7, restraints_fn=fn,
                                                            restraint_opts=dict(scale=True))
    one, three = job(1), job(3)
    for k in one:
        if k == "time_list":
            continue
        assert len(one[k]) == len(three[k]) == 3, k
        for g in range(3):
            assert (one[k][g] == three[k][g]).all() and one[k][g].shape == three[k][g].shape, (k, g)
    assert one["restraint_dist"][1].shape == (0,) and one["restraint_atom"][0].shape == (3,) and int(one["restraint_atom"][0][0]) == 7
    plain = harness.sample_diffusion_ligand_decomp(m, pocket, num_samples=3, batch_size=3, device="cuda:0", num_steps=3, init="device",
                                                   sample_key_seed=7)
    assert (plain["pred_pos"][1] == one["pred_pos"][1]).all() and not (plain["pred_pos"][0] == one["pred_pos"][0]).all()
