"""GPU cases of the weight regimes of tests/stress_weights.py: DecompScorePosNet3D.forward through the C ABI against the
oracle evaluated in float64 on the same fp32 weights and inputs, at the bench shape, a tiny graph (K = N - 1 < 32, NL = 3), the
first sizes of the 4- and 8-tile segment kernels (NL = 34 / 66), a degenerate lattice geometry, and one padded heterogeneous
batch (one reverse step at t = 0, whose position is the network's x0 and whose v0 trajectory row is log_softmax of its logits:
forward() takes dense batches only, the padded launch exists in the sampler, whose workspace is laid out per padded row -- the
outputs of that step are what a caller of a padded batch can read).  Then dd_reverse_step alone, fed host-made logits at its
edges (tests/stress_steps.py), against the float64 restatement of the transition.
Bounds (stress_weights.bound): the project's 1e-4 where the fp32 oracle itself is within 2.5e-5 of the fp64 one on that input,
else twice the fp32 oracle's own distance -- computed here from the two oracle runs, never from a kernel's output.
Every case builds a further model, so tests/test_gpu_stress.py runs this module in a process of its own (see
tests/test_gpu_knn_wide.py); `pytest -m gpu -s tests/stress_cases.py` runs it directly."""
import ctypes

import numpy as np
import pytest
import torch

import stress_steps as ST
import stress_weights as SW
from decompdiff_amd import DecompScorePosNet3D, hip_lib, shipped_config
from decompdiff_amd.model import _Call
from test_gpu_parity import _forward_hip, _sample_hip, dev, maxabs, to_dev

pytestmark = pytest.mark.gpu
EW_TOL = 1e-5                       # edge weights (a sigmoid): the bound of test_forward_intermediates_vs_dense_spec

_MODEL = {}


def model_for(regime):
    """One regime's model at a time (the cases are ordered by regime)."""
    if regime not in _MODEL:
        _MODEL.clear()
        cfg = shipped_config()
        m = DecompScorePosNet3D(cfg, 29, 10, 8)
        sd = m.state_dict()
        sd.update(SW.regime_state_dict(regime, cfg))
        m.load_state_dict(sd, strict=True)
        _MODEL[regime] = m.to(dev())
    return _MODEL[regime]


def workspace_tensors(m):
    """nbr, e_w, final h / h_bond / x of the last forward, as test_forward_intermediates_vs_dense_spec reads them."""
    s, bufs = m._last
    view = hip_lib.DDWsView()
    hip_lib.check(hip_lib.load().dd_workspace_view(ctypes.byref(s), ctypes.byref(view)))
    B, NP, NL, K = s.B, s.NP, s.NL, s.K
    N = NP + NL

    def grab(ptr, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        base = bufs["workspace"]
        off = (ptr - base.data_ptr()) // 4
        t = base[off:off + n]
        return (t.view(torch.int32) if dtype == torch.int32 else t).view(*shape).cpu()
    h = grab(view.h, (B, N, 128)).clone()
    if view.lin_in_node:                           # W_lin . A_nb of the last layer is still pending on the ligand rows
        h[:, NP:] += grab(view.Anb, (B, NL, 128))
    return dict(nbr=grab(view.nbr, (B, N, K), torch.int32), e_w=grab(view.ew, (B, N, K)), h=h,
                h_bond=grab(view.hb, (B, NL * (NL - 1), 128)), x=grab(view.x, (B, N, 3))), (B, N, K)


def report(regime, shape, errs, d32, bounds):
    """One machine-readable line per case (the wrapper folds them into one parity line per regime), printed before any assert."""
    worst = max(errs, key=lambda k: errs[k] / bounds[k])
    print(f"\nSTRESS {regime} {shape} worst={worst} err={errs[worst]:.3g} bound={bounds[worst]:.3g} d32={d32[worst]:.3g} | "
          + " ".join(f"{k}:{errs[k]:.2g}/{bounds[k]:.2g}(d32 {d32[k]:.2g})" for k in errs))


def _padded_case(regime, shape, monkeypatch):
    cfg = shipped_config()
    sd = SW.regime_state_dict(regime, cfg)
    b = SW.SHAPES[shape][0]()
    want64, want32, d32 = SW.step_t0_reference(sd, cfg, b)
    n_lig, n_bond = b["init_ligand_pos"].size(0), b["init_ligand_fc_bond_type"].size(0)
    g = torch.Generator().manual_seed(3)
    noise = dict(u_v=torch.rand(1, n_lig, 8, generator=g), u_b=torch.rand(1, n_bond, 5, generator=g),
                 eps=torch.randn(1, n_lig, 3, generator=g))
    monkeypatch.setenv("DD_RAGGED_MODE", "padded")
    r = _sample_hip(model_for(regime), b, 1, None, noise, t_start=0)
    got = dict(pos=r["pos"], log_v0=r["v0_traj"][0], log_bt=r["bt_traj"][0])
    errs = {k: maxabs(got[k], want64[k]) for k in got}
    bounds = {k: SW.bound(d32[k]) for k in got}
    report(regime, shape, errs, d32, bounds)
    assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in got.values())
    assert got["pos"].shape == (n_lig, 3)
    for k in got:
        assert errs[k] < bounds[k], (k, errs[k], bounds[k])


@pytest.mark.parametrize("regime,shape", sorted(SW.cases()))
def test_forward_regime_vs_fp64_oracle(regime, shape, monkeypatch):
    if shape.startswith("padded"):
        return _padded_case(regime, shape, monkeypatch)
    cfg = shipped_config()
    sd = SW.regime_state_dict(regime, cfg)
    b = SW.SHAPES[shape][0]()
    want64, want32, d32 = SW.both_oracles(sd, cfg, b)
    m = model_for(regime)
    out = _forward_hip(m, b)
    torch.cuda.synchronize()
    ws, (B, N, K) = workspace_tensors(m)
    got = dict(pred_ligand_pos=out["pred_ligand_pos"], pred_ligand_v=out["pred_ligand_v"], pred_bond=out["pred_bond"],
               h=ws["h"].reshape(B * N, 128), h_bond=ws["h_bond"].reshape(-1, 128), x=ws["x"].reshape(B * N, 3),
               e_w=ws["e_w"].reshape(-1, 1))
    errs = {k: maxabs(got[k], want64[k]) for k in got}
    bounds = {k: (EW_TOL if k == "e_w" else SW.bound(d32[k])) for k in got}
    report(regime, shape, errs, d32, bounds)
    # the kernel and both oracle runs saw the same edges (neighbours of a centre by ascending distance, ties by index)
    src = want64["edge_index"][0].view(B, N, K) - (torch.arange(B) * N).view(B, 1, 1)
    assert torch.equal(ws["nbr"].long(), src), "kNN graph differs from the oracle's"
    for k in got:
        assert bool(torch.isfinite(torch.as_tensor(got[k])).all()), k
        assert errs[k] < bounds[k], (k, errs[k], bounds[k])
    if shape.startswith("lattice"):                # the degenerate geometry also against the suite's own reference, fp32
        e32 = {k: maxabs(got[k], want32[k]) for k in SW.OUTPUTS}
        print(f"\nSTRESS32 {regime} {shape} " + " ".join(f"{k}:{v:.2g}" for k, v in e32.items()))
        assert all(v < SW.TOL for v in e32.values()), e32


# ------------------------------------------------------------------------------------ dd_reverse_step at its edges
def _one_step(m, bd, xt, t, inp, eps, seed=None):
    """A fresh chain at t, one dd_reverse_step on the host-made network outputs -> what it wrote, on the CPU.  `seed`: the step
    draws its own noise on the device with that key (production noise) instead of taking inp's uniforms and `eps`."""
    lib = hip_lib.load()
    noise = dict(u_v=inp["u_v"][None], u_b=inp["u_b"][None], eps=eps[None]) if seed is None else None
    T = m.num_timesteps
    try:
        m.num_timesteps = t + 1                    # (the chain then starts at t: test_gpu_parity._sample_hip)
        c = m._prepare_chain(bd["protein_pos"], bd["protein_v"], bd["batch_protein"], bd["init_ligand_pos"], bd["init_ligand_v"],
                             bd["ligand_v_aux"], bd["batch_ligand"], bd["prior_stds"], bd["ligand_decomp_batch"],
                             bd["ligand_decomp_index"], None, bd["ligand_fc_bond_index"], bd["init_ligand_fc_bond_type"], None, None,
                             _Call(m.num_timesteps, 1, noise=noise, seed=0 if seed is None else seed))
    finally:
        m.num_timesteps = T
    cb = c["bufs"]
    assert torch.equal(cb["lig_pos"].cpu().view(-1, 3), xt), "the chain's x_t is the host's centred ligand"
    assert int(cb["step_counter"][0]) == 0 and int(cb["step_counter"][1]) == t
    lv, lb, x0 = (inp[k].to(dev()).contiguous() for k in ("logits_v", "logits_b", "x0"))
    st = hip_lib.stream_ptr(dev())
    hip_lib.check(lib.dd_reverse_step(ctypes.byref(c["s"]), hip_lib.ptr(lv), hip_lib.ptr(lb), hip_lib.ptr(x0), st), "dd_reverse_step")
    torch.cuda.synchronize()
    nc = lv.size(-1)
    return dict(log_v0=cb["traj_v0"][0].view(-1, nc).cpu(), log_vt=cb["traj_vt"][0].view(-1, nc).cpu(), log_bt=cb["traj_bt"][0].view(-1, 5).cpu(),
                lig_pos=cb["lig_pos"].view(-1, 3).cpu(), traj_pos=cb["traj_pos"][0].view(-1, 3).cpu(), lig_v=cb["lig_v"].cpu().long(),
                lig_bond=cb["lig_bond"].cpu().long(), traj_v=cb["traj_v"][0].cpu().long(), traj_bond=cb["traj_bond"][0].cpu().long(),
                steps_done=int(cb["step_counter"][0]))


@pytest.mark.parametrize("nc,prior,nl", ST.step_cases())
def test_reverse_step_edges_vs_fp64(nc, prior, nl):
    """Per case 12 transitions (t in {999, 500, 1, 0} x logits N(0,1) x {1, 30, 1000}): log_softmax, both posteriors, new positions
    within their bounds, every sampled type exact (stress_steps.prepared passes over seeds with a near-tie draw), step counter
    advanced; at t = 0 the new positions do not depend on eps."""
    m = ST.build_model(nc, prior).to(dev())
    tab = ST.tables(m)
    b, offset, xt = ST.batch_for(nc, nl)
    bd = to_dev(b)
    failures = []
    for t, scale, base_seed in ST.sub_cases(nc, prior, nl):
        p = ST.prepared(tab, b, xt, offset, nc, t, scale, base_seed)
        got = _one_step(m, bd, xt, t, p["inp"], p["inp"]["eps"])
        w = p["w64"]
        errs = {k: maxabs(got[k], w[k]) for k in ST.COMPARED}
        nv = int((got["lig_v"] != w["v_next"]).sum()) + int((got["traj_v"] != w["v_next"]).sum())
        nb = int((got["lig_bond"] != w["b_next"]).sum()) + int((got["traj_bond"] != w["b_next"]).sum())
        worst = max(errs, key=lambda k: errs[k] / p["bounds"][k])
        print(f"\nSTEP nc={nc} prior={prior} NL={nl} t={t} scale={scale:g} seed={p['seed']} worst={worst} err={errs[worst]:.3g} "
              f"bound={p['bounds'][worst]:.3g} d32={p['d32'][worst]:.3g} type-mismatches={nv}+{nb} | "
              + " ".join(f"{k}:{errs[k]:.2g}/{p['bounds'][k]:.2g}" for k in errs))
        finite = all(bool(torch.isfinite(got[k]).all()) for k in ST.COMPARED)
        ok = finite and all(errs[k] < p["bounds"][k] for k in errs) and nv == 0 and nb == 0 and got["steps_done"] == 1
        if t == 0:                                 # no noise at t = 0: another eps, the same positions bit for bit
            again = _one_step(m, bd, xt, t, p["inp"], p["inp"]["eps"] * -3.0 + 1.0)
            ok = ok and torch.equal(again["lig_pos"], got["lig_pos"]) and torch.equal(again["traj_pos"], got["traj_pos"])
        if not ok:
            failures.append((t, scale, errs, nv, nb, got["steps_done"]))
    assert not failures, failures
