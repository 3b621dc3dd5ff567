"""GPU cases: the plain (unfixed) reverse step under PRODUCTION noise draws at the documented Philox addresses.  dd_reverse_step
(k_step_rows<NC, false> twice and k_step_pos) on host-made logits with ``noise=None`` and an explicit chain seed, against
stress_steps.reference_step in float64 fed the draws tests/philox_ref.py derives from the documented contract alone
(step_draws: streams 1 / 2 / 7 at time word t, key = the seed's halves, rows flat over the batch of B = 2, so sample 1's rows
carry a batch offset).

Per case (atom class count, NL) six transitions: t in {999, 1, 0} x two chain seeds, one with bits in the high half of the key.
Logits and x0: stress_steps.draw_inputs at logit scale 1; model, tables and batch: stress_steps, uniform prior.
Near ties: a transition uses the first chain seed >= its base seed (at most 200 candidates) at which the float64 reference's two
best scores of every draw lie further apart than twice the log-probabilities' bound -- the rule of stress_steps.prepared,
decided from the reference alone -- so every sampled atom and bond type is compared and no mismatch is allowed.
Bounds: stress_weights.bound(d32) per output, d32 from the float32 run of the same reference.  The reference's eps is the float64
value of philox_ref's z32; the device's normal may differ from it by the few ulp of its own logf / sqrtf / cosf, so the position
bounds carry a further 4 x d32a x max(std) x exp(0.5 logvar_t) (d32a = philox_ref.contract_d32a(), the bound unit of
tests/test_gpu_philox_contract.py; the term is printed).  At t = 0 the step adds no noise: the term is 0 and the positions equal
the noise-free mean within the plain bound.
The cases build four further models, so tests/test_gpu_philox_contract.py runs this module in a process of its own (see
tests/test_gpu_knn_wide.py); `pytest -m gpu -s tests/philox_step_cases.py` runs it directly."""
import math

import pytest
import torch

import philox_ref as PR
import stress_steps as ST
import stress_weights as SW
from stress_cases import _one_step
from test_gpu_parity import dev, maxabs, to_dev

pytestmark = pytest.mark.gpu

CASES = ((8, 30), (13, 30), (23, 30), (8, 66))          # (atom classes, NL): 2 / 4 / 6 Philox class blocks; 8580 bond rows at NL = 66
TIMES = (999, 1, 0)
BASE_SEEDS = (2021, (0x9E3779B9 << 32) | 77)            # the second has bits in the high key half
POS_KEYS = ("lig_pos", "traj_pos")


def prepared(tab, b, xt, offset, nc, t, base_seed, input_seed):
    """Inputs of one transition with the first chain seed >= base_seed without a near-tie draw, its float64 reference, d32 and bounds.
    Reads no kernel output."""
    n_lig, n_bond = b["init_ligand_pos"].size(0), b["init_ligand_fc_bond_type"].size(0)
    base = ST.draw_inputs(nc, n_lig, n_bond, 1.0, input_seed)
    for seed in range(base_seed, base_seed + 200):
        inp = dict(base, **{k: torch.from_numpy(v) for k, v in PR.step_draws(seed, t, n_lig, n_bond, nc).items()})
        w64 = ST.reference_step(tab, b, xt, offset, inp, t, torch.float64)
        w32 = ST.reference_step(tab, b, xt, offset, inp, t, torch.float32)
        d32 = {k: float((w64[k] - w32[k].double()).abs().max()) for k in ST.COMPARED}
        bounds = {k: SW.bound(d32[k]) for k in ST.COMPARED}
        gaps = {"v": float(w64["v_gap"].min()), "b": float(w64["b_gap"].min())}
        if gaps["v"] > 2 * bounds["log_vt"] and gaps["b"] > 2 * bounds["log_bt"]:
            eps_term = 0.0 if t == 0 else 4.0 * PR.contract_d32a() * float(b["prior_stds"].max()) * math.exp(0.5 * float(tab["pos"][2, t]))
            for k in POS_KEYS:
                bounds[k] += eps_term
            return dict(seed=seed, inp=inp, w64=w64, d32=d32, bounds=bounds, gaps=gaps, eps_term=eps_term)
    raise AssertionError("no chain seed without a near-tie draw")


@pytest.mark.parametrize("nc,nl", CASES)
def test_unfixed_step_draws_at_the_documented_addresses(nc, nl):
    m = ST.build_model(nc, "uniform").to(dev())
    tab = ST.tables(m)
    b, offset, xt = ST.batch_for(nc, nl)
    assert int(b["batch_ligand"].max()) + 1 == 2
    bd = to_dev(b)
    failures = []
    for i, t in enumerate(TIMES):
        for j, base_seed in enumerate(BASE_SEEDS):
            p = prepared(tab, b, xt, offset, nc, t, base_seed, 500 + 10 * i + j)
            got = _one_step(m, bd, xt, t, p["inp"], None, seed=p["seed"])
            w = p["w64"]
            errs = {k: maxabs(got[k], w[k]) for k in ST.COMPARED}
            nv = int((got["lig_v"] != w["v_next"]).sum()) + int((got["traj_v"] != w["v_next"]).sum())
            nb = int((got["lig_bond"] != w["b_next"]).sum()) + int((got["traj_bond"] != w["b_next"]).sum())
            worst = max(errs, key=lambda k: errs[k] / p["bounds"][k])
            print(f"\nPHILOXSTEP nc={nc} NL={nl} t={t} seed={p['seed']:#x} worst={worst} err={errs[worst]:.3g} "
                  f"bound={p['bounds'][worst]:.3g} d32={p['d32'][worst]:.3g} type-mismatches={nv}+{nb} eps-term={p['eps_term']:.3g} | "
                  + " ".join(f"{k}:{errs[k]:.2g}/{p['bounds'][k]:.2g}" for k in errs))
            finite = all(bool(torch.isfinite(got[k]).all()) for k in ST.COMPARED)
            ok = finite and all(errs[k] < p["bounds"][k] for k in errs) and nv == 0 and nb == 0 and got["steps_done"] == 1
            if not ok:
                failures.append((t, hex(p["seed"]), errs, nv, nb, got["steps_done"]))
    assert not failures, failures
