"""Per-sample noise keys (``sample_diffusion(sample_keys=...)``, dd_sample_steps_keyed / dd_graph_create_keyed).

The anchor: with keys, sample b receives exactly the draws that a call on that sample alone (B = 1) with ``seed=key_b`` receives,
whatever batch it sits in.  Everything here is ``torch.equal`` -- no tolerance: the network is batch-independent bit for bit
(asserted first, with injected noise rows, where a composition is compared), so any difference is a noise-addressing one.

Shapes: pockets of 40-48 atoms, ligands of 6-9 atoms, knn 32, 3-4 steps, B <= 4 -- the smallest at which the padded and a sample's
own bond enumeration differ (6 / 8 atoms inside a width of 9) and the atom / bond rows of a batch fill more than one block."""
import ctypes

import pytest
import torch

from decompdiff_amd import hip_lib, sample_keys, synth
from test_gpu_parity import dev, model, model_nc, to_dev

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
TRAJ = ("pos_traj", "v_traj", "bond_traj", "v0_traj", "vt_traj", "bt_traj")
KEYS = [int(k) & M64 for k in sample_keys(2024, range(8)).tolist()]      # Python ints in [0, 2**64)
DRIFT = [dict(type="armsca_prox", min_d=1.2, max_d=1.9), dict(type="clash", sigma=2.0, gamma=4.0),
         dict(type="arms_repul", max_d=2.5, mode="min")]
POCKETS = {8: synth.make_pocket_tiny(11, num_protein=48, arm_atoms=(3, 2), scaffold_atoms=3),
           6: synth.make_pocket_tiny(12, num_protein=40, arm_atoms=(2, 2), scaffold_atoms=2),
           9: synth.make_pocket_tiny(13, num_protein=44, arm_atoms=(3, 3), scaffold_atoms=3)}


def single(nl, seed, nc=8):
    """One sample (its own B = 1 batch) of the pocket with `nl` ligand atoms."""
    torch.manual_seed(seed)
    return synth.build_sampling_batch(POCKETS[nl], 1, num_classes=nc)


def run(m, b, steps=3, center_pos_mode="protein", **kw):
    r = m.sample_diffusion(num_steps=steps, center_pos_mode=center_pos_mode, **to_dev(b), **kw)
    out = {k: r[k].cpu() for k in ("pos", "v", "bond")}
    out.update({k: torch.stack(r[k]) for k in TRAJ if len(r[k])})
    return out


def split(r, n_l):
    """Per-sample results of a batch whose samples have n_l[b] ligand atoms."""
    parts, a0, b0 = [], 0, 0
    for n in n_l:
        a1, b1 = a0 + n, b0 + n * (n - 1)
        p = {"pos": r["pos"][a0:a1], "v": r["v"][a0:a1], "bond": r["bond"][b0:b1]}
        for k in TRAJ:
            if k in r:
                p[k] = r[k][:, b0:b1] if k in ("bond_traj", "bt_traj") else r[k][:, a0:a1]
        parts.append(p)
        a0, b0 = a1, b1
    return parts


def assert_same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert torch.equal(got[k], want[k]), (what, k)


def noise_rows(noise, n_l, b):
    a0, b0 = sum(n_l[:b]), sum(n * (n - 1) for n in n_l[:b])
    n = n_l[b]
    return {"u_v": noise["u_v"][:, a0:a0 + n].contiguous(), "u_b": noise["u_b"][:, b0:b0 + n * (n - 1)].contiguous(),
            "eps": noise["eps"][:, a0:a0 + n].contiguous()}


@pytest.mark.parametrize("nc", [8, 13])
def test_anchor_one_sample_keyed_is_that_sample_seeded(nc):
    """B = 1: seed = k and sample_keys = [k] are the same chain, results and all six trajectories (8 classes: two Philox class
    blocks, 13: four).  k has its top bit set: the whole 64 bits reach the kernels."""
    m, b = model_nc(nc), single(8, 1, nc)
    k = 0xE220A8397B1DCDAF
    seeded, keyed = run(m, b, seed=k), run(m, b, sample_keys=[k])
    assert all(t in seeded for t in TRAJ) and seeded["vt_traj"].shape == (3, 8, nc)
    assert_same(keyed, seeded, f"{nc} classes")
    assert_same(run(m, b, sample_keys=torch.tensor([k - (1 << 64)], dtype=torch.int64)), seeded, "int64 tensor")
    assert not torch.equal(run(m, b, sample_keys=[k ^ 1])["pos"], seeded["pos"])


@pytest.mark.parametrize("drift", [None, DRIFT], ids=["plain", "drift"])
def test_dense_batch_of_four_equals_each_sample_alone(drift):
    """B = 4 with keys against each sample alone with seed = key_b, in the given and in the reversed order of the samples.  The
    armsca / arms_repul energies are means over the caller's batch: the single runs normalise by 4 (_drift_norm_batch)."""
    m = model(0)
    singles = [single(8, 100 + b) for b in range(4)]
    n_l, steps = [8] * 4, 3
    noise = synth.draw_step_noise(steps, 32, 4 * 56)
    for order in ([0, 1, 2, 3], [3, 2, 1, 0]):
        batch = synth.concat_sampling_batches([singles[b] for b in order])
        # precondition: with injected noise rows the two compositions agree bit for bit (the network is batch-independent)
        parts = split(run(m, batch, steps, energy_drift_opt=drift, noise=noise), n_l)
        for pos, b in enumerate(order):
            alone = run(m, singles[b], steps, energy_drift_opt=drift, noise=noise_rows(noise, n_l, pos), _drift_norm_batch=4)
            assert_same(parts[pos], alone, f"precondition (injected noise), sample {b} at position {pos}")
        # the property: device noise addressed by key
        parts = split(run(m, batch, steps, energy_drift_opt=drift, sample_keys=[KEYS[b] for b in order]), n_l)
        for pos, b in enumerate(order):
            alone = run(m, singles[b], steps, energy_drift_opt=drift, seed=KEYS[b], _drift_norm_batch=4)
            assert_same(parts[pos], alone, f"sample {b} at position {pos}")


def test_ragged_batch_padded_grouped_and_alone_agree(monkeypatch):
    """Ligands of 8, 6, 9 and 6 atoms in pockets of 48, 40, 44 and 40: as one padded batch (a 6-atom ligand's bond rows inside a
    width of 9), as size groups one after the other (samples 1 and 3 share a group: keys follow their samples), as size groups
    replayed round-robin, and each sample alone -- the same chain per sample."""
    m = model(0)
    n_l, steps = [8, 6, 9, 6], 3
    singles = [single(n, 200 + b) for b, n in enumerate(n_l)]
    batch = synth.concat_sampling_batches(singles)
    keys = KEYS[:4]
    alone = [run(m, s, steps, seed=k) for s, k in zip(singles, keys)]
    from decompdiff_amd import batch_layout as BL
    assert BL.fits_padded(BL.BatchLayout([48, 40, 44, 40], n_l), m.config.knn)
    for mode, concurrent in (("padded", "0"), ("groups", "0"), ("groups", "1")):
        monkeypatch.setenv("DD_RAGGED_MODE", mode)
        monkeypatch.setenv("DD_RAGGED_CONCURRENT", concurrent)
        parts = split(run(m, batch, steps, sample_keys=keys), n_l)
        for b in range(4):
            assert_same(parts[b], alone[b], f"{mode} (concurrent {concurrent}), sample {b}")


def test_eager_captured_streamed_and_resumed_chains_agree():
    m = model(0)
    batch = synth.concat_sampling_batches([single(8, 300), single(8, 301)])
    keys = KEYS[4:6]
    streamed = run(m, batch, 4, sample_keys=keys)                                   # captured graph, trajectories streamed
    assert_same(run(m, batch, 4, sample_keys=keys, use_graph=False), streamed, "eager launches")
    captured = run(m, batch, 4, sample_keys=keys, keep_traj=False)                  # captured graph, no trajectories
    assert_same(captured, {k: streamed[k] for k in ("pos", "v", "bond")}, "captured, no trajectories")
    # a chain split with start_step continues the unsplit chain's noise (model frame: no offset re-added in between)
    full = run(m, batch, 4, center_pos_mode="none", sample_keys=keys)
    first = run(m, batch, 2, center_pos_mode="none", sample_keys=keys)
    b2 = dict(batch)
    b2["init_ligand_pos"], b2["init_ligand_v"], b2["init_ligand_fc_bond_type"] = first["pos"], first["v"], first["bond"]
    rest = run(m, b2, 2, center_pos_mode="none", sample_keys=keys, start_step=2)
    joined = {k: rest[k] for k in ("pos", "v", "bond")}
    joined.update({k: torch.cat([first[k], rest[k]]) for k in TRAJ})
    assert_same(joined, full, "split with start_step")


def test_cached_chain_serves_other_keys_and_unkeyed_calls(monkeypatch):
    """One cached entry and its step graph per shape: the keys are read from device memory at every launch, and a keyed and
    an unkeyed chain never share a captured graph.  Every call equals its uncached (DD_CHAIN_CACHE=0) result."""
    m = model(0)
    batch = synth.concat_sampling_batches([single(8, 400), single(8, 401)])
    calls = {"k1": dict(sample_keys=KEYS[0:2]), "k2": dict(sample_keys=KEYS[2:4]), "seeded": dict(seed=5)}
    monkeypatch.setenv("DD_CHAIN_CACHE", "0")
    want = {name: run(m, batch, 3, **kw) for name, kw in calls.items()}
    assert not torch.equal(want["k1"]["pos"], want["k2"]["pos"])
    monkeypatch.setenv("DD_CHAIN_CACHE", "1")
    for name in ("k1", "k2", "seeded", "k1", "seeded", "seeded", "k2"):
        assert_same(run(m, batch, 3, **calls[name]), want[name], name)


def test_key_behaviour_and_refused_arguments():
    m = model(0)
    one = single(8, 500)
    twins = synth.concat_sampling_batches([one, one])                               # identical initial states
    a, b = split(run(m, twins, 3, sample_keys=[KEYS[0], KEYS[1]]), [8, 8])
    assert not (torch.equal(a["v"], b["v"]) and torch.equal(a["pos"], b["pos"]))
    a, b = split(run(m, twins, 3, sample_keys=[KEYS[0], KEYS[0]]), [8, 8])
    assert_same(a, b, "equal keys on identical initial states")
    s, bufs = m._last
    noise = synth.draw_step_noise(3, 16, 2 * 56)
    for bad in (dict(sample_keys=KEYS[:3]), dict(sample_keys=KEYS[:1]), dict(sample_keys=KEYS[:2], noise=noise),
                dict(sample_keys=KEYS[:2], seed=1), dict(sample_keys=[-1, 0]), dict(sample_keys=[0, 1 << 64]),
                dict(sample_keys=torch.zeros(2, dtype=torch.int32))):
        with pytest.raises(ValueError):
            run(m, twins, 3, **bad)
    # the C entry point refuses keys together with injected noise before anything is launched
    lib = hip_lib.load()
    eps = torch.zeros(3, 16, 3, device=dev())
    s.eps = eps.data_ptr()
    try:
        rc = lib.dd_sample_steps_keyed(ctypes.byref(s), m._model_opts(), hip_lib.ptr(bufs["sample_keys"]), 1, hip_lib.stream_ptr(dev()))
        graph = ctypes.c_void_p()
        rc_g = lib.dd_graph_create_keyed(ctypes.byref(s), m._model_opts(), hip_lib.ptr(bufs["sample_keys"]), 1,
                                         torch.cuda.Stream(dev()).cuda_stream, ctypes.byref(graph))
    finally:
        s.eps = None
    assert rc == -1 and rc_g == -1 and not graph.value                              # DD_ERR_BAD_ARG
