"""Per-sample noise keys, host side: the two keyed entry points are declared, exported and bound without touching the ABI,
`sample_keys` is the documented splitmix64, and the sampling harness hands every model call the keys of its output samples."""
import ctypes
import os
import re

import pytest
import torch

import decompdiff_amd
from decompdiff_amd import harness, hip_lib, sample_keys, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYED_SYMBOLS = ("dd_sample_steps_keyed", "dd_graph_create_keyed")
M64 = (1 << 64) - 1


def splitmix64_key(seed: int, index: int) -> int:
    """The documented function on Python integers: the mix of seed + golden * (index + 1), modulo 2**64."""
    z = (seed + 0x9E3779B97F4A7C15 * (index + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def unsigned(t: torch.Tensor):
    return [int(v) & M64 for v in t.reshape(-1).tolist()]


def test_keyed_entry_points_are_declared_exported_and_bound():
    import __graft_entry__
    __graft_entry__.build()
    lib = hip_lib.load()
    hdr = open(os.path.join(ROOT, "include", "decompdiff_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for name in KEYED_SYMBOLS:
        assert name in hip_lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r"\b" + name + r"\s*\(", code), name
        assert getattr(lib, name).restype is ctypes.c_int
    S, O = ctypes.POINTER(hip_lib.DDSampler), ctypes.POINTER(hip_lib.DDModelOpts)
    assert lib.dd_sample_steps_keyed.argtypes == [S, O, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    assert lib.dd_graph_create_keyed.argtypes == [S, O, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
    # the siblings' lists with one more pointer after opts
    assert lib.dd_sample_steps_keyed.argtypes[:2] + lib.dd_sample_steps_keyed.argtypes[3:] == lib.dd_sample_steps_opts.argtypes
    assert lib.dd_graph_create_keyed.argtypes[:2] + lib.dd_graph_create_keyed.argtypes[3:] == lib.dd_graph_create_opts.argtypes
    # the addressing is written out where a host in another language reads it
    for phrase in ("dst * (n - 1) + sp", "3 * i + c", "nl_real[b]", "DD_ERR_BAD_ARG"):
        assert phrase in hdr[hdr.index("Per-sample noise keys"):hdr.rindex("dd_graph_create_keyed")], phrase


def test_abi_and_struct_layouts_are_unchanged():
    lib = hip_lib.load()
    assert lib.dd_abi_version() == hip_lib.ABI_VERSION == 9
    assert ctypes.sizeof(hip_lib.DDSampler) == 392 and ctypes.sizeof(hip_lib.DDModelOpts) == 32
    assert [f[0] for f in hip_lib.DDModelOpts._fields_] == ["size", "bond_head", "node_out", "num_blocks"]
    assert not any("key" in f[0] for f in hip_lib.DDSampler._fields_)
    # NULL arguments are refused before anything is launched (no GPU needed)
    assert lib.dd_sample_steps_keyed(None, None, None, 1, None) == -1
    assert lib.dd_graph_create_keyed(None, None, None, 1, None, None) == -1


def test_sample_keys_is_the_documented_splitmix64():
    assert decompdiff_amd.sample_keys is sample_keys and "sample_keys" in decompdiff_amd.__all__
    # first outputs of a splitmix64 generator seeded with 0 and with 1234567 (Vigna's reference implementation)
    assert splitmix64_key(0, 0) == 0xE220A8397B1DCDAF and splitmix64_key(0, 1) == 0x6E789E6AA1B965F4
    assert splitmix64_key(1234567, 0) == 6457827717110365317 and splitmix64_key(1234567, 1) == 3203168211198807973
    for seed in (0, 1, 2021, (1 << 63) + 5, M64):
        idx = [0, 1, 2, 37, 1000, (1 << 31) + 3]
        got = sample_keys(seed, idx)
        assert got.dtype == torch.int64 and tuple(got.shape) == (len(idx),)
        assert unsigned(got) == [splitmix64_key(seed, i) for i in idx]
    # shapes: an int, a range, a tensor
    assert sample_keys(5, 37).dim() == 0 and unsigned(sample_keys(5, 37)) == [splitmix64_key(5, 37)]
    assert torch.equal(sample_keys(5, range(4, 9)), sample_keys(5, torch.arange(4, 9)))
    assert torch.equal(sample_keys(5, range(4, 9)), sample_keys(5, range(9))[4:])        # a key depends on its own index only
    many = sample_keys(11, range(10000))
    assert torch.equal(many, sample_keys(11, range(10000))) and len(set(many.tolist())) == 10000
    assert not torch.equal(many[:100], sample_keys(12, range(100)))
    with pytest.raises(ValueError):
        sample_keys(0, [-1])
    assert "0x9E3779B97F4A7C15" in sample_keys.__doc__ and "0xBF58476D1CE4E5B9" in sample_keys.__doc__ \
        and "0x94D049BB133111EB" in sample_keys.__doc__


class RecordingModel:
    """A model with the HIP model's extra keywords that records them and returns its inputs."""
    num_timesteps, num_classes, num_bond_classes = 10, 8, 5

    def __init__(self):
        self.calls = []

    def sample_diffusion(self, num_steps=None, center_pos_mode=None, energy_drift_opt=None, noise=None, seed=None, use_graph=True,
                         sample_keys=None, **batch):
        self.calls.append(dict(noise=noise, seed=seed, sample_keys=sample_keys, n=int(batch["batch_ligand"].max()) + 1))
        empty = {k: [] for k in ("pos_traj", "v_traj", "bond_traj", "v0_traj", "vt_traj", "bt_traj")}
        return dict(pos=batch["init_ligand_pos"], v=batch["init_ligand_v"], bond=batch["init_ligand_fc_bond_type"], **empty)


class ReferenceSignatureModel(RecordingModel):
    """... and one with the bare reference signature (no extras)."""

    def sample_diffusion(self, num_steps=None, center_pos_mode=None, energy_drift_opt=None, **batch):
        self.calls.append(dict(n=int(batch["batch_ligand"].max()) + 1))
        return RecordingModel.sample_diffusion(RecordingModel(), **batch)


@pytest.mark.parametrize("batch_size,pool", [(2, 1), (3, 1), (2, 2)])
def test_harness_passes_the_keys_of_its_output_samples(batch_size, pool):
    pocket = synth.make_pocket_tiny(3)
    m = RecordingModel()
    torch.manual_seed(0)
    out = harness.sample_diffusion_ligand_decomp(m, pocket, num_samples=5, batch_size=batch_size, device="cpu", num_steps=2,
                                                 pool_batches=pool, sample_key_seed=99, first_sample_index=40)
    assert len(out["pred_pos"]) == 5 and sum(c["n"] for c in m.calls) == 5
    assert all(c["noise"] is None and c["seed"] is None for c in m.calls)          # keys exclude both
    got = torch.cat([c["sample_keys"] for c in m.calls])
    assert all(c["sample_keys"].numel() == c["n"] for c in m.calls)
    assert torch.equal(got, sample_keys(99, range(40, 45)))                          # output order, whatever the batching
    # unkeyed: as before, seed + batch index and no keys
    m2 = RecordingModel()
    harness.sample_diffusion_ligand_decomp(m2, pocket, num_samples=5, batch_size=batch_size, device="cpu", num_steps=2, seed=7,
                                           pool_batches=pool)
    assert all(c["sample_keys"] is None for c in m2.calls)
    assert [c["seed"] for c in m2.calls] == [7 + i for i in range(0, -(-5 // batch_size), pool)]
    # a model without the extra keywords is never handed keys
    m3 = ReferenceSignatureModel()
    harness.sample_diffusion_ligand_decomp(m3, pocket, num_samples=3, batch_size=2, device="cpu", num_steps=2, sample_key_seed=99)
    assert [c["n"] for c in m3.calls] == [2, 1]
    with pytest.raises(ValueError):
        harness.sample_diffusion_ligand_decomp(m, pocket, num_samples=2, batch_size=2, device="cpu", num_steps=2, sample_key_seed=1,
                                               noise_fn=lambda *a: None)
