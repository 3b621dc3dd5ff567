"""GPU cases of kNN graphs wider than the shipped knn = 32 (33 <= K <= 64 = DD_KNN_MAX) end to end -- the selection kernels
against a brute-force kNN, the fused forward / reverse steps / padded batches / training objective against fixtures from the
reference itself (tools/make_knn_golden.py) and against the oracle, which honours cfg.knn.  Run by tests/test_gpu_knn_wide.py
in a process of their own (see there); `pytest -m gpu tests/knn_wide_cases.py` runs them directly."""
import json

import numpy as np
import pytest
import torch

import golden_utils as GU
from decompdiff_amd import DecompScorePosNet3D, functional, hip_lib, shipped_config, synth
from oracle import model as OM
from test_gpu_configs import _check_chain, _fixture_chain, _hetero_batch
from test_gpu_parity import LOGIT_TOL, POS_TOL, _forward_hip, _sample_hip, dev, maxabs
from test_gpu_training import _loss_kwargs

pytestmark = pytest.mark.gpu

_MODELS = {}


def model_k(knn):
    if knn not in _MODELS:
        cfg = shipped_config(knn=knn)
        m = DecompScorePosNet3D(cfg, 29, 10, 8)
        sd = m.state_dict()
        sd.update(synth.synthetic_state_dict(cfg, 0))
        m.load_state_dict(sd, strict=True)
        _MODELS[knn] = m.to(dev())
    return _MODELS[knn]


def brute_knn(x, K, real=None):
    """x [N,3] fp32 -> [N, K] int64: ascending (d2, index), self excluded, d2 = (dx*dx + dy*dy) + dz*dz as the kernel forms it
    (exact fp32 products and sums, held in float64 for the sort).  real: bool [N], candidates restricted to real atoms."""
    d = x[:, None, :] - x[None, :, :]
    d2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).double()
    d2.fill_diagonal_(float("inf"))
    if real is not None:
        d2[:, ~real] = float("inf")
    return torch.sort(d2, dim=-1, stable=True).indices[:, :K]


def tied_coords(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, N, 3, generator=g) * 12).round(decimals=2)       # coarse grid: many equal distances
    x[:, 1::7] = x[:, 0:1]                                              # exact duplicates of atom 0: ties at d2 = 0 too
    return x.contiguous()


# ------------------------------------------------------------------------------------ selection
@pytest.mark.parametrize("K", [33, 48, 64])
@pytest.mark.parametrize("B,N", [(3, 65), (2, 330), (1, 2048)])
def test_dd_knn_wide_exact(B, N, K):
    x = tied_coords(B, N, seed=N + K)
    xd = x.to(dev())
    nbr = torch.full((B, N, K), -1, dtype=torch.int32, device=dev())
    hip_lib.check(hip_lib.load().dd_knn(hip_lib.ptr(xd), B, N, K, hip_lib.ptr(nbr), hip_lib.stream_ptr()), "dd_knn")
    torch.cuda.synchronize()
    got = nbr.cpu().long()
    for b in range(B):
        assert torch.equal(got[b], brute_knn(x[b], K)), f"sample {b}"


@pytest.mark.parametrize("K", [33, 48, 64])
def test_dd_knn_masked_wide_exact(K):
    B, NP, NL = 3, 300, 40
    np_real, nl_real = [300, 211, 64], [40, 33, 9]
    x = tied_coords(B, NP + NL, seed=K)
    xd = x.to(dev())
    npr = torch.tensor(np_real, dtype=torch.int32, device=dev())
    nlr = torch.tensor(nl_real, dtype=torch.int32, device=dev())
    nbr = torch.full((B, NP + NL, K), -1, dtype=torch.int32, device=dev())
    hip_lib.check(hip_lib.load().dd_knn_masked(hip_lib.ptr(xd), B, NP, NL, K, hip_lib.ptr(npr), hip_lib.ptr(nlr), hip_lib.ptr(nbr),
                                               hip_lib.stream_ptr()), "dd_knn_masked")
    torch.cuda.synchronize()
    got = nbr.cpu().long()
    for b in range(B):
        real = torch.zeros(NP + NL, dtype=torch.bool)
        real[:np_real[b]] = True
        real[NP:NP + nl_real[b]] = True
        want = brute_knn(x[b], K, real)
        assert torch.equal(got[b][real], want[real]), f"sample {b}"


def test_dd_knn_rejects_k_above_64():
    lib = hip_lib.load()
    x = torch.zeros(1, 100, 3, device=dev())
    nbr = torch.zeros(1, 100, 65, dtype=torch.int32, device=dev())
    assert lib.dd_knn(hip_lib.ptr(x), 1, 100, 65, hip_lib.ptr(nbr), hip_lib.stream_ptr()) < 0


@pytest.mark.parametrize("k,B,N", [(48, 2, 330), (64, 3, 65), (64, 2, 40), (33, 1, 20)])
def test_functional_knn_graph_wide(k, B, N):
    """torch_cluster semantics: k > N - 1 gives every other atom of the sample (the last two cases)."""
    x = tied_coords(B, N, seed=k + N)
    batch = torch.arange(B).repeat_interleave(N)
    ei = functional.knn_graph(x.view(-1, 3).to(dev()), k, batch.to(dev())).cpu()
    kk = min(k, N - 1)
    want_src = torch.cat([brute_knn(x[b], kk) + b * N for b in range(B)]).reshape(-1)
    assert ei.shape == (2, B * N * kk)
    assert torch.equal(ei[0], want_src)
    assert torch.equal(ei[1], torch.arange(B * N).repeat_interleave(kk))


# ------------------------------------------------------------------------------------ forward / sampling
def test_forward_k48_reference_golden():
    g = GU.load("forward_k48")
    assert int(g["knn"]) == 48
    out = _forward_hip(model_k(48), GU.batch_from_npz(g))
    torch.cuda.synchronize()
    errs = {k: maxabs(out[k], g["out_" + k]) for k in ("pred_ligand_pos", "pred_ligand_v", "pred_bond")}
    print("forward knn=48 vs reference golden:", {k: f"{v:.3g}" for k, v in errs.items()})
    assert errs["pred_ligand_pos"] < POS_TOL and errs["pred_ligand_v"] < LOGIT_TOL and errs["pred_bond"] < LOGIT_TOL
    assert torch.equal(out["pred_ligand_v"].argmax(-1).cpu(), torch.from_numpy(g["out_pred_ligand_v"]).argmax(-1))
    assert torch.equal(out["pred_bond"].argmax(-1).cpu(), torch.from_numpy(g["out_pred_bond"]).argmax(-1))


@pytest.mark.parametrize("knn", [48, 64])
@pytest.mark.parametrize("np_,arms,sca,B", [(120, (5, 5), 8, 2), (60, (12, 12), 20, 1)])
def test_forward_wide_knn_vs_oracle(knn, np_, arms, sca, B):
    """A 138-atom graph (kNN segments of 3 / 4 full tiles) and a 104-atom graph with a 44-atom ligand (3-tile bond segments)."""
    cfg, sd = GU.weights(0, shipped_config(knn=knn))
    pocket = synth.make_pocket(21, np_, arms, sca, num_full_protein=np_ + 10)
    torch.manual_seed(9)
    b = synth.build_sampling_batch(pocket, B)
    with torch.no_grad():
        want = OM.forward(sd, cfg, b["protein_pos"], b["protein_v"], b["batch_protein"], b["init_ligand_pos"], b["init_ligand_v"],
                          b["ligand_v_aux"], b["batch_ligand"], b["ligand_fc_bond_index"], b["init_ligand_fc_bond_type"])
    out = _forward_hip(model_k(knn), b)
    torch.cuda.synchronize()
    errs = {k: maxabs(out[k], want[k]) for k in want}
    print(f"forward knn={knn} NP={np_} NL={pocket.num_ligand_atoms} B={B}:", {k: f"{v:.3g}" for k, v in errs.items()})
    assert errs["pred_ligand_pos"] < POS_TOL and errs["pred_ligand_v"] < LOGIT_TOL and errs["pred_bond"] < LOGIT_TOL
    assert torch.equal(out["pred_ligand_v"].argmax(-1).cpu(), want["pred_ligand_v"].argmax(-1))
    assert torch.equal(out["pred_bond"].argmax(-1).cpu(), want["pred_bond"].argmax(-1))


@pytest.mark.parametrize("name,std_scale", [("traj3_k64_b4_plain", None), ("traj3_k64_b4_drift", [1.0, 0.9, 0.8, 1.1])])
def test_sampling_k64_reference_golden(name, std_scale):
    g, b, noise = _fixture_chain(name, synth.make_pocket_small(8), 4, std_scale)
    r = _sample_hip(model_k(64), b, 3, json.loads(str(g["drift"])), noise)
    _check_chain(f"knn=64 ({name}: NP=300, NL=30, B=4)", r, g, 3)


def test_padded_heterogeneous_batch_k48_equals_size_groups(monkeypatch):
    """One padded launch sequence at knn = 48 reproduces the per-size dense groups (every sample has >= 49 atoms)."""
    sizes, n_prot = [9, 37, 20, 33], [150, 260, 120, 200]
    b = _hetero_batch(sizes, n_prot, seed=6)
    steps = 3
    noise = synth.draw_step_noise(steps, b["init_ligand_pos"].size(0), b["init_ligand_fc_bond_type"].size(0))
    m = model_k(48)
    outs = {}
    for mode in ("padded", "groups"):
        monkeypatch.setenv("DD_RAGGED_MODE", mode)
        outs[mode] = _sample_hip(m, b, steps, GU.DRIFT, noise)
    p, g = outs["padded"], outs["groups"]
    err = maxabs(p["pos"], g["pos"])
    e_bt = maxabs(torch.stack(p["bt_traj"]), torch.stack(g["bt_traj"]))
    print(f"knn=48 padded vs groups: pos diff {err:.3g}, bond log-prob diff {e_bt:.3g}")
    assert p["pos"].shape == (sum(sizes), 3)
    assert err < 5e-6 and e_bt < 5e-5
    assert torch.equal(p["v"], g["v"]) and torch.equal(p["bond"], g["bond"])


# ------------------------------------------------------------------------------------ training
def test_diffusion_loss_and_gradients_k48_match_reference():
    g = GU.load("loss_grad_k48")
    assert int(g["knn"]) == 48
    m = model_k(48)
    m.train()
    try:
        m.zero_grad(set_to_none=True)
        kw = _loss_kwargs(g)
        torch.manual_seed(int(g["noise_seed"]))
        res = m.get_diffusion_loss(**kw)
        for k in ("pos", "v", "bond"):
            got, want = float(res["losses"][k]), float(g["loss_" + k])
            print(f"knn=48 loss {k}: {got:.7g} (reference {want:.7g})")
            assert abs(got - want) <= 1e-4 * max(1.0, abs(want)) and abs(got - want) <= 2e-3 * abs(want) + 1e-7
        assert maxabs(res["pred_ligand_pos"], g["out_pred_ligand_pos"]) < 1e-4
        assert maxabs(res["pred_ligand_v"], g["out_pred_ligand_v"]) < 1e-4
        assert maxabs(res["x0"], g["out_x0"]) < 1e-5
        loss = res["losses"]["pos"] + 100.0 * res["losses"]["v"] + 100.0 * res["losses"]["bond"]
        loss.backward()
        params = dict(m.named_parameters())
        for key in [k for k in g.files if k.startswith("grad__")]:
            name = key[len("grad__"):].replace("__", ".")
            want = torch.from_numpy(g[key])
            got = params[name].grad.cpu()
            rel = float((got - want).abs().max() / want.abs().max().clamp(min=1e-12))
            assert rel < 2e-3, (name, rel)
        names = [str(n) for n in g["grad_norm_names"]]
        got_norms = np.array([float(params[n].grad.double().norm()) if params[n].grad is not None else 0.0 for n in names])
        rel_n = np.abs(got_norms - g["grad_norms"]) / np.maximum(g["grad_norms"], 1e-6 * g["grad_norms"].max())
        print(f"knn=48: {len(names)} parameter gradients, worst relative norm error {rel_n.max():.2g}")
        assert rel_n.max() < 2e-3
    finally:
        m.zero_grad(set_to_none=True)
        m.eval()
