"""The drift guidance kernels (dd_drift_armsca, dd_drift_clash, dd_drift_arms_repul) through the C ABI at the cases of
tests/drift_cases.py, against the gradient of the oracle's energy under float64 autograd: every size at which a kernel changes
path, constructed winners, exact ties, hinges at exact equality, coincident atoms, samples without arm or scaffold atoms, arm
ids with gaps, an underflowing exponential sum, accumulate = 0 onto NaN and accumulate = 1 onto a known buffer.  Bounds come
from the float64 / fp32 oracle pair (drift_cases.bound), never from a kernel's output; no case and no atom is left out.
Then one reverse step of the sampler with a scaffold atom exactly on an arm atom."""
import pytest
import torch

import drift_cases as DC
import golden_utils as GU
from decompdiff_amd import hip_lib, synth
from oracle import diffusion as OD
from test_gpu_parity import POS_TOL, _sample_hip, dev, maxabs, model

pytestmark = pytest.mark.gpu
CASES = DC.all_cases()


def _launch(case, out, accumulate):
    """The case's kernel on `out` -> status."""
    lib = hip_lib.load()
    B, NL = case["B"], case["NL"]
    xd = case["pos"].to(dev()).contiguous()
    keep = [xd]
    if case["kind"] == "clash":
        off, fp = case["offset"].to(dev()).contiguous(), case["prot"].to(dev()).contiguous()
        keep += [off, fp]
        rc = lib.dd_drift_clash(hip_lib.ptr(xd), hip_lib.ptr(off), hip_lib.ptr(fp), B, NL, case["NF"], case["sigma"], case["gamma"],
                                hip_lib.ptr(out), accumulate, hip_lib.stream_ptr())
    else:
        dec = case["decomp"].to(device=dev(), dtype=torch.int32).contiguous()
        keep.append(dec)
        if case["kind"] == "armsca":
            rc = lib.dd_drift_armsca(hip_lib.ptr(xd), hip_lib.ptr(dec), B, NL, case["min_d"], case["max_d"], hip_lib.ptr(out), accumulate,
                                     hip_lib.stream_ptr())
        else:
            rc = lib.dd_drift_arms_repul(hip_lib.ptr(xd), hip_lib.ptr(dec), B, NL, case["max_d"], {"min": 1, "all": 2}[case["mode"]],
                                         hip_lib.ptr(out), accumulate, hip_lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("name", DC.NAMES)
def test_drift_kernel_vs_float64_autograd(name):
    case = CASES[name]
    g64, _, d32, bnd = DC.reference(name)
    n = case["B"] * case["NL"]
    out = torch.full((n, 3), float("nan"), device=dev())          # accumulate = 0 must write every row
    hip_lib.check(_launch(case, out, 0), name)
    buf = DC.known_buffer(name, (n, 3))
    acc = buf.to(dev()).contiguous()                                # accumulate = 1 adds onto what is there
    hip_lib.check(_launch(case, acc, 1), name)
    out, acc = out.cpu(), acc.cpu()
    finite = bool(torch.isfinite(out).all()) and bool(torch.isfinite(acc).all())
    err = maxabs(out, g64) if finite else float("nan")
    err_acc = maxabs(acc, buf.double() + g64) if finite else float("nan")
    # buffer + gradient is rounded once more, at the buffer's magnitude
    bnd_acc = bnd + float(buf.abs().max()) * 2.0 ** -23
    DC.report(name, err, d32, bnd, f" err_acc={err_acc:.3g} bound_acc={bnd_acc:.3g} |g|={float(g64.abs().max()):.3g}")
    assert finite, (name, out[~torch.isfinite(out).all(1)][:4])
    assert err < bnd, (name, err, bnd)
    assert err_acc < bnd_acc, (name, err_acc, bnd_acc)
    NL = case["NL"]
    for b in case.get("invalid", ()) + ((case["no_arm_sample"],) if "no_arm_sample" in case else ()):
        rows = slice(b * NL, (b + 1) * NL)
        assert torch.equal(out[rows], torch.zeros(NL, 3)), (name, b)            # zeros written over the NaN
        assert torch.equal(acc[rows], buf[rows]), (name, b)                     # and the buffer alone
    if "expect" in case:                                                        # lattice cases: the value is known in closed form
        assert maxabs(out, torch.tensor(case["expect"], dtype=torch.float64)) < bnd, (name, out)


def test_armsca_and_arms_repul_refuse_129_atoms_and_launch_nothing():
    lib = hip_lib.load()
    B, NL = 1, 129
    xd = torch.zeros(B * NL, 3, device=dev())
    dec = torch.zeros(B * NL, dtype=torch.int32, device=dev())
    out = torch.full((B * NL, 3), 7.0, device=dev())
    assert lib.dd_drift_armsca(hip_lib.ptr(xd), hip_lib.ptr(dec), B, NL, 1.2, 1.9, hip_lib.ptr(out), 0, hip_lib.stream_ptr()) != 0
    assert lib.dd_drift_arms_repul(hip_lib.ptr(xd), hip_lib.ptr(dec), B, NL, 1.9, 1, hip_lib.ptr(out), 0, hip_lib.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_reverse_step_with_a_scaffold_atom_on_an_arm_atom_vs_oracle():
    """One reverse step at t = 500 with the project's drift terms on drift_cases.sampler_batch: arm 0's nearest scaffold atom is at
    distance 0 (zero subgradient: the step must stay finite and equal the oracle's)."""
    cfg, sd = GU.weights(0)
    b = DC.sampler_batch()
    assert torch.equal(b["init_ligand_pos"][8], b["init_ligand_pos"][0]) and int(b["ligand_decomp_index"][8]) == -1
    noise = synth.draw_step_noise(1, b["init_ligand_pos"].size(0), b["init_ligand_fc_bond_type"].size(0))
    want = OD.sample_diffusion(sd, cfg, num_steps=1, energy_drift_opt=GU.DRIFT, noise=noise, t_start=500, **b)
    plain = OD.sample_diffusion(sd, cfg, num_steps=1, energy_drift_opt=None, noise=noise, t_start=500, **b)
    got = _sample_hip(model(0), b, 1, GU.DRIFT, noise, 500)
    finite = bool(torch.isfinite(got["pos"]).all())
    err = maxabs(got["pos"], want["pos"]) if finite else float("nan")
    print(f"\nDRIFT sampler step t=500, scaffold atom on an arm atom: finite={finite} pos err {err:.3g} (tol {POS_TOL:g}); "
          f"effect of the drift on the step {maxabs(want['pos'], plain['pos']):.3g}")
    assert bool(torch.isfinite(want["pos"]).all()) and maxabs(want["pos"], plain["pos"]) > 1e-3
    assert finite
    assert err < POS_TOL
    assert torch.equal(got["v"].cpu(), want["v"]) and torch.equal(got["bond"].cpu(), want["bond"])
