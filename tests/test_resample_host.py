"""Resampling (``sample_diffusion(resample=...)``), host side: the schedule is the documented contract, the jump table is the
float64 composition rounded once, the four entry points are declared, exported and bound without touching the ABI, and every bad
``resample`` raises ValueError before anything reaches the GPU."""
import ctypes
import math
import os
import re

import pytest
import torch

import decompdiff_amd
from decompdiff_amd import DecompScorePosNet3D, harness, hip_lib, resample_schedule, shipped_config, synth
from decompdiff_amd.model import _as_resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESAMPLE_SYMBOLS = ("dd_sample_steps_resample", "dd_graph_create_resample", "dd_resample_jump", "dd_sampler_reset_resample")


# ------------------------------------------------------------------------------------------------ 1: the schedule
def test_schedule_worked_example_literally():
    assert decompdiff_amd.resample_schedule is resample_schedule and "resample_schedule" in decompdiff_amd.__all__
    ops = resample_schedule(999, 994, 2, 2)
    assert [o[1] for o in ops if o[0] == "step"] == [999, 998, 999, 998, 997, 996, 997, 996, 995, 994, 995, 994]
    assert [o for o in ops if o[0] == "jump"] == [("jump", 997, 999), ("jump", 995, 997), ("jump", 993, 995)]
    assert ops == [("step", 999), ("step", 998), ("jump", 997, 999), ("step", 999), ("step", 998), ("step", 997), ("step", 996),
                   ("jump", 995, 997), ("step", 997), ("step", 996), ("step", 995), ("step", 994), ("jump", 993, 995),
                   ("step", 995), ("step", 994)]


GRID = [(n, j, r, t_hi) for t_hi in (999, 500) for n in (1, 2, 6, 7, 12) for j in (1, 2, 3, 5, 6, 7, 12, 13) for r in (1, 2, 3, 4)]
GRID += [(6, 2, 2, 5), (6, 6, 3, 5), (6, 1, 2, 5), (4, 3, 2, 3), (1, 1, 5, 0)]       # ranges that end at level -1


@pytest.mark.parametrize("n,j,r,t_hi", GRID)
def test_schedule_counts_and_shape(n, j, r, t_hi):
    t_lo = t_hi - n + 1
    ops = resample_schedule(t_hi, t_lo, j, r)
    steps = [o[1] for o in ops if o[0] == "step"]
    jumps = [o for o in ops if o[0] == "jump"]
    P = n // j
    assert len(steps) == n + (r - 1) * j * P and len(jumps) == (r - 1) * P
    if r == 1 or j > n:
        assert ops == [("step", t) for t in range(t_hi, t_lo - 1, -1)]            # the plain chain
    assert ops[0] == ("step", t_hi) and ops[-1] == ("step", t_lo) and min(steps) == t_lo and max(steps) == t_hi
    for a, b in zip(ops, ops[1:]):
        if a[0] == "step" and b[0] == "step":
            assert b[1] == a[1] - 1
        elif a[0] == "step":                                                       # a jump leaves the level the step reached ...
            assert b[1] == a[1] - 1 and b[2] == b[1] + j and b[2] <= t_hi
            assert (b[1] - (t_lo - 1)) % j == 0                                    # ... at a point anchored at the last level
        else:                                                                      # ... and the next step runs at its target
            assert b == ("step", a[2])
    # what sample_diffusion runs: the same steps as runs, every run but the last followed by a jump
    rs = _as_resample(dict(jump_length=j, n_resample=r), {}, None, 1000, n, 999 - t_hi)
    assert rs["t_traj"].tolist() == steps and rs["t_traj"].dtype == torch.int64 and rs["n_total"] == len(steps)
    assert sum(k for k, _ in rs["runs"]) == len(steps) and [jp for _, jp in rs["runs"]] == [True] * len(jumps) + [False]
    # streamed pieces: every position once, in order, at most `piece` long, the launches of a piece add up to it
    for piece in (3, 8):
        pcs = DecompScorePosNet3D._pieces(rs["runs"], piece)
        assert pcs[0][0] == 0 and pcs[-1][1] == len(steps) and all(a[1] == b[0] for a, b in zip(pcs, pcs[1:]))
        assert all(0 < hi - lo <= piece and sum(o for o in ops_ if o != "jump") == hi - lo for lo, hi, ops_ in pcs)
        flat = [o for _, _, ops_ in pcs for o in ops_]
        assert flat.count("jump") == len(jumps) and flat[-1] != "jump"


def test_plain_pieces_are_the_equal_pieces_of_before():
    assert DecompScorePosNet3D._pieces([(20, False)], 8) == [(0, 8, [8]), (8, 16, [8]), (16, 20, [4])]
    assert DecompScorePosNet3D._pieces([(16, False)], 8) == [(0, 8, [8]), (8, 16, [8])]


# ------------------------------------------------------------------------------------------------ 2: the jump table
def _model(nc=8):
    return DecompScorePosNet3D(shipped_config(), 29, nc + 2, nc)


@pytest.mark.parametrize("j", [1, 2, 3, 10, 1000])
def test_jump_table_is_the_float64_composition_rounded_once(j):
    m = _model()
    T = m.num_timesteps
    tab = m.resample_jump_table(j)
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (6, T) and tab.is_contiguous()
    ac = m.alphas_cumprod.detach().double()
    lv = m.atom_type_trans.log_alphas_cumprod_v.detach().double()
    lb = m.bond_type_trans.log_alphas_cumprod_v.detach().double()
    lvl = lambda t, l, clean: t[l] if l >= 0 else torch.tensor(clean, dtype=torch.float64)
    for mm in sorted({j - 1, min(T - 1, j), min(T - 1, j + 7), T // 2, T - 2, T - 1}):
        if mm < j - 1:
            continue
        a = ac[mm] / lvl(ac, mm - j, 1.0)
        want = [a.sqrt(), (1.0 - a).sqrt()]
        for lc in (lv, lb):
            lr = lc[mm] - lvl(lc, mm - j, 0.0)
            want += [lr, torch.log(1.0 - torch.exp(lr))]
        assert torch.equal(tab[:, mm], torch.stack(want).float()), mm
    live = tab[:, j - 1:].double()
    # A^2 + S^2 = 1 to fp32 rounding; A[m] sqrt(abar[m - j]) = sqrt(abar[m]) to relative 2^-22; lr < 0 and exp(lr) + exp(l1mr) = 1
    assert float((live[0] ** 2 + live[1] ** 2 - 1).abs().max()) < 3 * 2.0 ** -24
    prev = torch.cat([torch.ones(1, dtype=torch.float64), ac])[:T - j + 1]
    assert float((live[0] * prev.sqrt() / ac[j - 1:].sqrt() - 1).abs().max()) <= 2.0 ** -22
    for row in (2, 4):
        assert bool((live[row] < 0).all()) and float((live[row].exp() + live[row + 1].exp() - 1).abs().max()) < 1e-6
    # out of the clean level: the forward process itself
    fst = m.fixed_step_table()
    assert torch.equal(tab[0, j - 1], fst[0, j - 1]) and torch.equal(tab[1, j - 1], fst[1, j - 1])
    assert torch.equal(tab[2, j - 1], lv[j - 1].float()) and torch.equal(tab[4, j - 1], lb[j - 1].float())
    assert bool((tab[:, :j - 1] == 0).all())                                     # never read


# ------------------------------------------------------------------------------------------------ 3: the entry points
def test_resample_entry_points_are_declared_exported_and_bound():
    import __graft_entry__
    __graft_entry__.build()
    lib = hip_lib.load()
    hdr = open(os.path.join(ROOT, "include", "decompdiff_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for name in RESAMPLE_SYMBOLS:
        assert name in hip_lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert getattr(lib, name).restype is ctypes.c_int
    S, O, F, R = (ctypes.POINTER(t) for t in (hip_lib.DDSampler, hip_lib.DDModelOpts, hip_lib.DDFixed, hip_lib.DDResample))
    V = ctypes.c_void_p
    assert lib.dd_sample_steps_resample.argtypes == [S, O, V, F, R, ctypes.c_int, V]
    assert lib.dd_graph_create_resample.argtypes == [S, O, V, F, R, ctypes.c_int, V, ctypes.POINTER(V)]
    assert lib.dd_resample_jump.argtypes == [S, V, F, R, V] and lib.dd_sampler_reset_resample.argtypes == [S, R, V]
    # the _fixed siblings' lists with the struct after fixed
    assert lib.dd_sample_steps_resample.argtypes[:4] + lib.dd_sample_steps_resample.argtypes[5:] == lib.dd_sample_steps_fixed.argtypes
    assert lib.dd_graph_create_resample.argtypes[:4] + lib.dd_graph_create_resample.argtypes[5:] == lib.dd_graph_create_fixed.argtypes
    body = re.search(r"typedef struct dd_resample \{(.*?)\} dd_resample;", code, flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s*;", body)
    assert fields == [f[0] for f in hip_lib.DDResample._fields_] == ["size", "jump_length", "tab", "epoch"]
    assert ctypes.sizeof(hip_lib.DDResample) == 24
    doc = hdr[hdr.index("Resampling (EXTENSION"):hdr.index("typedef struct dd_resample")]
    for phrase in ("t + 65536 * epoch", "m + 65536 * e", "3 atom types, 4 bond types", "8 coordinates", "t_start += jump_length",
                   "keep their bits", "DD_ERR_BAD_ARG", "every launch", "T <= 65535"):
        assert phrase in doc, phrase
    dbg = open(os.path.join(ROOT, "include", "decompdiff_hip_debug.h")).read()
    assert "Kinds 3, 4 and 8" in dbg


def test_abi_and_struct_layouts_are_unchanged_and_null_calls_are_refused():
    lib = hip_lib.load()
    assert lib.dd_abi_version() == hip_lib.ABI_VERSION == 9
    assert ctypes.sizeof(hip_lib.DDFixed) == 56 and ctypes.sizeof(hip_lib.DDSampler) == 392 and ctypes.sizeof(hip_lib.DDModelOpts) == 32
    assert [f[0] for f in hip_lib.DDFixed._fields_] == ["size", "mode", "mask", "v0", "b0", "x0c", "cc", "tab"]
    assert lib.dd_sample_steps_resample(None, None, None, None, None, 1, None) == -1
    assert lib.dd_graph_create_resample(None, None, None, None, None, 1, None, None) == -1
    assert lib.dd_resample_jump(None, None, None, None, None) == -1
    assert lib.dd_sampler_reset_resample(None, None, None) == -1
    # structs that hold nothing are refused as well: no GPU is needed for the pointer checks
    s, f, r = hip_lib.DDSampler(), hip_lib.DDFixed(), hip_lib.DDResample()
    f.size, f.mode, r.size, r.jump_length = ctypes.sizeof(hip_lib.DDFixed), hip_lib.FIXED_HOLD, ctypes.sizeof(hip_lib.DDResample), 2
    assert lib.dd_resample_jump(ctypes.byref(s), None, ctypes.byref(f), ctypes.byref(r), None) == -1
    assert lib.dd_sampler_reset_resample(ctypes.byref(s), ctypes.byref(r), None) == -1
    assert lib.dd_sample_steps_resample(ctypes.byref(s), None, None, ctypes.byref(f), ctypes.byref(r), 1, None) == -1
    # the debug draws take the three new kinds and a class count, and refuse the rest
    assert lib.dd_debug_philox(1, 0, 0, 3, None, None) != 0 and lib.dd_debug_philox(1, 0, 4, 5, None, None) != 0
    assert lib.dd_debug_philox(1, 0, 4, 4 | (13 << 8), None, None) != 0


# ------------------------------------------------------------------------------------------------ 4: validation
def _batch(n_data=2):
    torch.manual_seed(5)
    return synth.build_sampling_batch(synth.make_pocket_tiny(3), n_data)


def _fixed(b, **over):
    n, nb = b["init_ligand_pos"].shape[0], b["init_ligand_fc_bond_type"].numel()
    f = dict(mask=torch.zeros(n, dtype=torch.bool), pos=torch.zeros(n, 3), v=torch.zeros(n, dtype=torch.long),
             bond=torch.zeros(nb, dtype=torch.long), mode="hold")
    f["mask"][:3] = True
    f.update(over)
    return f


def test_every_bad_resample_raises_value_error_before_the_gpu_is_needed():
    """CPU tensors: a valid call gets as far as the GPU check (RuntimeError: the HIP path needs device tensors), every bad one raises
    ValueError first."""
    m, b = _model(), _batch()
    n, nb = b["init_ligand_pos"].shape[0], b["init_ligand_fc_bond_type"].numel()
    noise = synth.draw_step_noise(4, n, nb)
    ok = dict(jump_length=2, n_resample=2)
    call = lambda resample, fixed, **kw: m.sample_diffusion(num_steps=4, center_pos_mode="protein", fixed=fixed, resample=resample,
                                                            **{**b, **kw})
    bad = [
        (ok, None, {}),                                                              # only together with fixed
        (ok, _fixed(b, mode="replace", init="given"), dict(noise=noise)),            # excludes noise=
        (ok, _fixed(b), dict(noise=noise)),
        (dict(jump_length=2), _fixed(b), {}),                                        # wrong keys
        (dict(jump_length=2, n_resample=2, extra=1), _fixed(b), {}),
        (dict(jump=2, n_resample=2), _fixed(b), {}),
        ((2, 2), _fixed(b), {}),                                                     # wrong types
        ("2x2", _fixed(b), {}),
        (dict(jump_length=2.0, n_resample=2), _fixed(b), {}),
        (dict(jump_length=2, n_resample="2"), _fixed(b), {}),
        (dict(jump_length=True, n_resample=2), _fixed(b), {}),
        (dict(jump_length=0, n_resample=2), _fixed(b), {}),                          # j < 1, r < 1
        (dict(jump_length=-1, n_resample=2), _fixed(b), {}),
        (dict(jump_length=2, n_resample=0), _fixed(b), {}),
        (ok, _fixed(b), dict(prior_centers=None)),                                   # a jump noises around the centres: hold too
        (dict(jump_length=1, n_resample=65537), _fixed(b), {}),                      # more than 65535 jumps
        (ok, _fixed(b), dict(start_step=998)),                                       # range past t = 0
    ]
    for i, (resample, fixed, kw) in enumerate(bad):
        with pytest.raises(ValueError):
            call(resample, fixed, **kw)
            pytest.fail(f"case {i} was accepted")
    good = [(ok, _fixed(b), {}), (ok, _fixed(b, mode="replace"), {}), (dict(jump_length=9, n_resample=1), _fixed(b), {}),
            (ok, _fixed(b, mode="replace", init="given"), dict(start_step=3)), (dict(jump_length=1, n_resample=3), _fixed(b), {})]
    for resample, fixed, kw in good:
        with pytest.raises(RuntimeError) as e:
            call(resample, fixed, **kw)
        assert not isinstance(e.value, (ValueError, NotImplementedError)), e.value
    # the epoch shares the time word with t
    with pytest.raises(ValueError, match="65535"):
        _as_resample(ok, {}, None, 65536, 4, 0)


class RecordingModel:
    """A model with the HIP model's extra keywords that records them and returns its inputs."""
    num_timesteps, num_classes, num_bond_classes = 10, 8, 5

    def __init__(self):
        self.calls = []

    def sample_diffusion(self, noise=None, seed=None, use_graph=True, sample_keys=None, fixed=None, resample=None, num_steps=None,
                         center_pos_mode=None, energy_drift_opt=None, **batch):
        self.calls.append(dict(fixed=fixed, resample=resample))
        return dict(pos=batch["init_ligand_pos"], v=batch["init_ligand_v"], bond=batch["init_ligand_fc_bond_type"], pos_traj=[],
                    v_traj=[], bond_traj=[], v0_traj=[], vt_traj=[], bt_traj=[])


def test_harness_hands_resample_through_with_fixed_only():
    pocket = synth.make_pocket_tiny(3)
    n = pocket.num_ligand_atoms
    rs = dict(jump_length=2, n_resample=3)

    def fixed_fn(index, decomp):
        if index >= 2:
            return None                                                              # the second model call holds nothing
        return dict(mask=torch.ones(n, dtype=torch.bool), pos=torch.zeros(n, 3), v=torch.zeros(n, dtype=torch.long),
                    bond=torch.zeros(n * (n - 1), dtype=torch.long))
    model = RecordingModel()
    harness.sample_diffusion_ligand_decomp(model, pocket, num_samples=4, batch_size=2, device="cpu", num_steps=4, fixed_fn=fixed_fn,
                                           fixed_mode="replace", resample=rs)
    assert len(model.calls) == 2 and model.calls[0]["resample"] == rs and model.calls[0]["fixed"]["mode"] == "replace"
    assert model.calls[1] == dict(fixed=None, resample=None)
    for kw in (dict(), dict(fixed_fn=fixed_fn, noise_fn=lambda *a: None)):
        with pytest.raises(ValueError):
            harness.sample_diffusion_ligand_decomp(RecordingModel(), pocket, num_samples=2, batch_size=2, device="cpu", num_steps=4,
                                                   resample=rs, **kw)
