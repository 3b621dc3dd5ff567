"""Fixed atoms (``sample_diffusion(fixed=...)``), host side: the three entry points are declared, exported and bound without
touching the ABI, ``fixed`` is validated before anything reaches the GPU, the forward-process table is the float64 square root
rounded once, and the sampling harness collates the per-sample dicts of ``fixed_fn`` into one flat ``fixed`` per model call."""
import ctypes
import os
import re

import pytest
import torch

from decompdiff_amd import DecompScorePosNet3D, harness, hip_lib, shipped_config, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXED_SYMBOLS = ("dd_sample_steps_fixed", "dd_graph_create_fixed", "dd_fixed_init")


def test_fixed_entry_points_are_declared_exported_and_bound():
    import __graft_entry__
    __graft_entry__.build()
    lib = hip_lib.load()
    hdr = open(os.path.join(ROOT, "include", "decompdiff_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for name in FIXED_SYMBOLS:
        assert name in hip_lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert getattr(lib, name).restype is ctypes.c_int
    S, O, F = ctypes.POINTER(hip_lib.DDSampler), ctypes.POINTER(hip_lib.DDModelOpts), ctypes.POINTER(hip_lib.DDFixed)
    V = ctypes.c_void_p
    assert lib.dd_sample_steps_fixed.argtypes == [S, O, V, F, ctypes.c_int, V]
    assert lib.dd_graph_create_fixed.argtypes == [S, O, V, F, ctypes.c_int, V, ctypes.POINTER(V)]
    assert lib.dd_fixed_init.argtypes == [S, V, F, V]
    # the _keyed siblings' lists with the struct after sample_keys
    assert lib.dd_sample_steps_fixed.argtypes[:3] + lib.dd_sample_steps_fixed.argtypes[4:] == lib.dd_sample_steps_keyed.argtypes
    assert lib.dd_graph_create_fixed.argtypes[:3] + lib.dd_graph_create_fixed.argtypes[4:] == lib.dd_graph_create_keyed.argtypes
    # the struct of the binding is the header's, the size first
    body = re.search(r"typedef struct dd_fixed \{(.*?)\} dd_fixed;", code, flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s*;", body)
    assert fields == [f[0] for f in hip_lib.DDFixed._fields_] and fields[0] == "size" and fields[1] == "mode"
    assert ctypes.sizeof(hip_lib.DDFixed) == 8 + 6 * 8
    m = re.search(r"enum \{ DD_FIXED_HOLD = (\d+), DD_FIXED_REPLACE = (\d+) \}", code)
    assert (int(m.group(1)), int(m.group(2))) == (hip_lib.FIXED_HOLD, hip_lib.FIXED_REPLACE) == (1, 2)
    # the semantics are written out where a host in another language reads them
    doc = hdr[hdr.index("Fixed atoms (EXTENSION"):hdr.index("typedef struct dd_fixed")]
    for phrase in ("src = sp + (sp >= dst)", "iff BOTH", "drawn at time l + 1", "t_start + 1", "DD_ERR_BAD_ARG", "every launch"):
        assert phrase in doc, phrase


def test_abi_and_struct_layouts_are_unchanged_and_null_calls_are_refused():
    lib = hip_lib.load()
    assert lib.dd_abi_version() == hip_lib.ABI_VERSION == 9
    assert ctypes.sizeof(hip_lib.DDSampler) == 392 and ctypes.sizeof(hip_lib.DDModelOpts) == 32
    assert not any("key" in f[0] or "fixed" in f[0] for f in hip_lib.DDSampler._fields_)
    assert lib.dd_sample_steps_fixed(None, None, None, None, 1, None) == -1
    assert lib.dd_graph_create_fixed(None, None, None, None, 1, None, None) == -1
    assert lib.dd_fixed_init(None, None, None, None) == -1
    # a struct that holds nothing is refused as well (no sampler: refused first; the pointer checks need no GPU either)
    f = hip_lib.DDFixed()
    f.size, f.mode = ctypes.sizeof(hip_lib.DDFixed), hip_lib.FIXED_HOLD
    assert lib.dd_fixed_init(None, None, ctypes.byref(f), None) == -1
    s = hip_lib.DDSampler()
    assert lib.dd_fixed_init(ctypes.byref(s), None, ctypes.byref(f), None) == -1


def _model(nc=8):
    cfg = shipped_config()
    return DecompScorePosNet3D(cfg, 29, nc + 2, nc)


def test_fixed_step_table_is_the_float64_square_root_rounded_once():
    m = _model()
    tab = m.fixed_step_table()
    ac = m.alphas_cumprod.detach().double()
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (2, m.num_timesteps) and tab.is_contiguous()
    assert torch.equal(tab[0], ac.sqrt().float()) and torch.equal(tab[1], (1.0 - ac).sqrt().float())
    # level 0 is nearly clean, the levels get noisier, and A^2 + S^2 = 1 to fp32 rounding
    assert float(tab[0, 0]) > 0.99 and bool((tab[0, 1:] <= tab[0, :-1]).all()) and bool((tab[1, 1:] >= tab[1, :-1]).all())
    assert float((tab[0].double() ** 2 + tab[1].double() ** 2 - 1).abs().max()) < 3 * 2.0 ** -24


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


def test_every_bad_fixed_raises_value_error_before_the_gpu_is_needed():
    """CPU tensors: a valid ``fixed`` gets as far as the GPU check (RuntimeError: the HIP path needs device tensors), every bad one
    raises ValueError first."""
    m, b = _model(), _batch()
    n, nb = b["init_ligand_pos"].shape[0], b["init_ligand_fc_bond_type"].numel()
    noise = synth.draw_step_noise(2, n, nb)
    call = lambda fixed, **kw: m.sample_diffusion(num_steps=2, center_pos_mode="protein", fixed=fixed, **{**b, **kw})
    bad_v, bad_b = torch.zeros(n, dtype=torch.long), torch.zeros(nb, dtype=torch.long)
    bad_v[1] = 8                                                                     # held atom, class out of range
    bad_b[0] = 5                                                                     # bond 1 -> 0: both endpoints held
    assert int(b["ligand_fc_bond_index"][0, 0]) < 3 and int(b["ligand_fc_bond_index"][1, 0]) < 3
    no_centres = dict(b, prior_centers=None)
    bad = [
        (_fixed(b, mask=torch.zeros(n - 1, dtype=torch.bool)), {}),                  # wrong lengths
        (_fixed(b, pos=torch.zeros(n + 1, 3)), {}),
        (_fixed(b, pos=torch.zeros(n, 2)), {}),
        (_fixed(b, v=torch.zeros(n + 2, dtype=torch.long)), {}),
        (_fixed(b, bond=torch.zeros(nb - 1, dtype=torch.long)), {}),
        (_fixed(b, mask=torch.zeros(n, dtype=torch.uint8)), {}),                     # dtype other than bool
        (_fixed(b, mask=torch.zeros(n, dtype=torch.long)), {}),
        (_fixed(b, mode="freeze"), {}),                                              # unknown mode
        (_fixed(b, v=bad_v), {}),                                                    # known type out of range
        (_fixed(b, v=-bad_v), {}),
        (_fixed(b, bond=bad_b), {}),
        (_fixed(b, mode="replace"), dict(prior_centers=None)),                       # replace without usable prior_centers
        (_fixed(b, mode="replace"), dict(prior_centers=b["prior_centers"][:, :2])),
        (_fixed(b), dict(ligand_atom_mask=torch.arange(n) > 0)),                     # a non-trivial ligand_atom_mask
        (_fixed(b, mode="replace"), dict(noise=noise)),                              # init='given' is required ...
        (_fixed(b, mode="replace", init="draw"), dict(noise=noise)),
        (_fixed(b, mode="replace"), dict(start_step=1)),
        (_fixed(b, mode="replace", init="draw"), dict(start_step=1)),
        (_fixed(b, mode="replace", init="later"), {}),
        ("hold", {}),                                                                # not a dict
        ({k: v for k, v in _fixed(b).items() if k != "bond"}, {}),                   # a key is missing
    ]
    assert no_centres["prior_centers"] is None
    for i, (fixed, kw) in enumerate(bad):
        with pytest.raises(ValueError):
            call(fixed, **kw)
            pytest.fail(f"case {i} was accepted")
    # classes at FREE rows are never read: out of range there is fine; an all-True ligand_atom_mask is no mask
    free_v = torch.zeros(n, dtype=torch.long)
    free_v[5] = 99
    good = [(_fixed(b), {}), (_fixed(b, v=free_v), {}), (_fixed(b), dict(ligand_atom_mask=torch.ones(n, dtype=torch.bool))),
            (_fixed(b, mode="replace"), {}), (_fixed(b, mode="replace", init="given"), dict(noise=noise)),
            (_fixed(b, mode="replace", init="given"), dict(start_step=1)), (_fixed(b, mode="hold"), dict(noise=noise))]
    for fixed, kw in good:
        with pytest.raises(RuntimeError) as e:
            call(fixed, **kw)
        assert not isinstance(e.value, (ValueError, NotImplementedError)), e.value


class RecordingModel:
    """A model with the HIP model's extra keywords that records them and returns its inputs."""
    num_timesteps, num_classes, num_bond_classes = 10, 8, 5

    def __init__(self):
        self.calls = []

    def sample_diffusion(self, num_steps=None, center_pos_mode=None, energy_drift_opt=None, noise=None, seed=None, use_graph=True,
                         sample_keys=None, fixed=None, **batch):
        self.calls.append(dict(seed=seed, sample_keys=sample_keys, fixed=fixed, n=int(batch["batch_ligand"].max()) + 1,
                               decomp=batch["ligand_decomp_index"].clone(), pos=batch["init_ligand_pos"].clone()))
        empty = {k: [] for k in ("pos_traj", "v_traj", "bond_traj", "v0_traj", "vt_traj", "bt_traj")}
        return dict(pos=batch["init_ligand_pos"], v=batch["init_ligand_v"], bond=batch["init_ligand_fc_bond_type"], **empty)


class ReferenceSignatureModel(RecordingModel):
    def sample_diffusion(self, num_steps=None, center_pos_mode=None, energy_drift_opt=None, **batch):
        assert "fixed" not in batch and "sample_keys" not in batch
        self.calls.append(dict(n=int(batch["batch_ligand"].max()) + 1))
        return RecordingModel.sample_diffusion(RecordingModel(), **batch)


def _scaffold_fn(seen):
    """Holds the scaffold (arm id -1) of every sample but those with index % 3 == 1; everything it returns carries the sample index."""
    def fn(g, decomp):
        seen.append((g, decomp.clone()))
        if g % 3 == 1:
            return None
        n = decomp.numel()
        return dict(mask=decomp == -1, pos=torch.full((n, 3), float(g)) + torch.arange(n).view(n, 1), v=torch.full((n,), g % 8),
                    bond=torch.full((n * (n - 1),), g % 5))
    return fn


@pytest.mark.parametrize("batch_size,pool", [(2, 1), (3, 1), (2, 2)])
def test_harness_collates_the_fixed_dicts_of_its_output_samples(batch_size, pool):
    pocket = synth.make_pocket_tiny(3)
    n = pocket.num_ligand_atoms
    m, seen = RecordingModel(), []
    torch.manual_seed(0)
    out = harness.sample_diffusion_ligand_decomp(m, pocket, num_samples=5, batch_size=batch_size, device="cpu", num_steps=2,
                                                 pool_batches=pool, sample_key_seed=99, first_sample_index=40,
                                                 fixed_fn=_scaffold_fn(seen), fixed_mode="replace")
    assert len(out["pred_pos"]) == 5 and [g for g, _ in seen] == list(range(40, 45))
    g = 40
    for c in m.calls:
        f = c["fixed"]
        assert c["sample_keys"].numel() == c["n"]                                    # keys and fixed atoms together
        assert f["mode"] == "replace" and f["mask"].dtype == torch.bool and f["pos"].dtype == torch.float32
        assert tuple(f["mask"].shape) == (c["n"] * n,) and tuple(f["pos"].shape) == (c["n"] * n, 3)
        assert tuple(f["v"].shape) == (c["n"] * n,) and tuple(f["bond"].shape) == (c["n"] * n * (n - 1),)
        for k in range(c["n"]):
            a, e = slice(k * n, (k + 1) * n), slice(k * n * (n - 1), (k + 1) * n * (n - 1))
            if g % 3 == 1:                                                           # None: nothing held
                assert not bool(f["mask"][a].any())
            else:
                assert torch.equal(f["mask"][a], c["decomp"][a] == -1) and bool(f["mask"][a].any())
                assert torch.equal(f["pos"][a], torch.full((n, 3), float(g)) + torch.arange(n).view(n, 1).float())
                assert bool((f["v"][a] == g % 8).all()) and bool((f["bond"][e] == g % 5).all())
            g += 1
    assert g == 45
    # the batches' own draws do not depend on fixed_fn
    m2 = RecordingModel()
    torch.manual_seed(0)
    harness.sample_diffusion_ligand_decomp(m2, pocket, num_samples=5, batch_size=batch_size, device="cpu", num_steps=2,
                                           pool_batches=pool, sample_key_seed=99, first_sample_index=40)
    assert all(c["fixed"] is None for c in m2.calls)
    assert all(torch.equal(a["pos"], b["pos"]) for a, b in zip(m.calls, m2.calls))


def test_harness_never_hands_fixed_to_a_bare_signature_model_and_checks_sizes():
    pocket = synth.make_pocket_tiny(3)
    n = pocket.num_ligand_atoms
    m3, seen = ReferenceSignatureModel(), []
    harness.sample_diffusion_ligand_decomp(m3, pocket, num_samples=3, batch_size=2, device="cpu", num_steps=2, fixed_fn=_scaffold_fn(seen))
    assert [c["n"] for c in m3.calls] == [2, 1]
    # every sample None: the model call carries no `fixed`
    m = RecordingModel()
    harness.sample_diffusion_ligand_decomp(m, pocket, num_samples=2, batch_size=2, device="cpu", num_steps=2, fixed_fn=lambda g, d: None)
    assert [c["fixed"] for c in m.calls] == [None]
    for key, shape in (("mask", (n + 1,)), ("pos", (n, 2)), ("v", (n - 1,)), ("bond", (n * n,))):
        def fn(g, decomp, key=key, shape=shape):
            f = dict(mask=torch.zeros(n, dtype=torch.bool), pos=torch.zeros(n, 3), v=torch.zeros(n, dtype=torch.long),
                     bond=torch.zeros(n * (n - 1), dtype=torch.long))
            f[key] = torch.zeros(shape, dtype=f[key].dtype)
            return f
        with pytest.raises(ValueError):
            harness.sample_diffusion_ligand_decomp(m, pocket, num_samples=2, batch_size=2, device="cpu", num_steps=2, fixed_fn=fn)
