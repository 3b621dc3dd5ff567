"""The distance-aware bond head (bond_net_type = 'pre_att', decompdiff.py:199-211, 323-341) on the host: configuration, weights,
the factorised form the kernels use, and the additive C ABI that carries it."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from decompdiff_amd import DecompScorePosNet3D, hip_lib, packing, shipped_config, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _model(kind="pre_att", seed=0):
    cfg = shipped_config(bond_net_type=kind)
    m = DecompScorePosNet3D(cfg, 29, 10, 8)
    sd = m.state_dict()
    sd.update(synth.synthetic_state_dict(cfg, seed))
    m.load_state_dict(sd, strict=True)
    return cfg, m


def test_pre_att_config_accepted_and_unknown_kinds_raise():
    cfg, m = _model("pre_att")
    assert m.bond_net_type == "pre_att" and m.bond_diffusion
    for bad in ("mlp", "post_att", "PRE_ATT"):
        with pytest.raises(NotImplementedError):
            DecompScorePosNet3D(shipped_config(bond_net_type=bad), 29, 10, 8)
    with pytest.raises(NotImplementedError):
        DecompScorePosNet3D(shipped_config(bond_net_type="pre_att", bond_diffusion=False), 29, 10, 8)


def test_state_dict_layout_and_shapes():
    lin = synth.learnable_param_shapes(shipped_config())
    pre = synth.learnable_param_shapes(shipped_config(bond_net_type="pre_att"))
    assert set(lin) == set(pre)
    assert [k for k in lin if lin[k] != pre[k]] == ["bond_inference.0.weight"]
    assert pre["bond_inference.0.weight"] == (128, 20 + 128)
    _, m = _model("pre_att")
    sd = m.state_dict()
    assert len(sd) == len(_model("lin")[1].state_dict()) == 616
    assert tuple(sd["bond_inference.0.weight"].shape) == (128, 148)
    assert torch.equal(sd["distance_expansion.offset"], torch.linspace(0.0, 5.0, 20))


def test_reference_pre_att_state_dict_loads_strictly():
    """The reference's own parameters and buffers (a fixture written by tools/make_preatt_golden.py from the reference model:
    its inputs / outputs do not matter here, only that the reference's weight shapes are the synthetic ones) load strictly."""
    cfg, m = _model("pre_att", seed=0)
    want = synth.synthetic_state_dict(cfg, 0)
    ref_like = {k: v.clone() for k, v in m.state_dict().items()}
    ref_like.update(want)
    m2 = DecompScorePosNet3D(cfg, 29, 10, 8)
    m2.load_state_dict(ref_like, strict=True)
    assert torch.equal(m2.state_dict()["bond_inference.0.weight"], want["bond_inference.0.weight"])
    with pytest.raises(RuntimeError):                     # a lin checkpoint does not fit a pre_att model
        m2.load_state_dict({**ref_like, "bond_inference.0.weight": torch.zeros(128, 128)}, strict=True)
    assert os.path.exists(os.path.join(GOLDEN, "forward_preatt.npz"))


def _reference_head(W1, b1, offset, coeff, pos, h, src, dst):
    """decompdiff.py:323-341 as the reference writes it (first Linear of bond_inference)."""
    d = torch.norm(pos[dst] - pos[src], p=2, dim=-1, keepdim=True)
    r = torch.exp(coeff * torch.pow(d.view(-1, 1) - offset.view(1, -1), 2))
    x = torch.cat([r, (h[dst] + h[src]) / 2], -1)
    return torch.nn.functional.linear(x, W1, b1)


def _factorised_head(form, pos, h, src, dst, dtype):
    """What the kernels compute: W_r^T r(d) + P[dst] + P[src] + b1, P = W_p h (packing.bond_head_pre_att)."""
    c = lambda t: t.to(dtype)
    P = h.to(dtype) @ c(form["W_p"]).t()
    d = (pos[dst] - pos[src]).to(dtype).norm(dim=-1)
    r = torch.exp(torch.tensor(form["coeff"], dtype=dtype) * (d.view(-1, 1) - c(form["offset"])) ** 2)
    return r @ c(form["W_r"]) + (P[dst] + P[src]) + c(form["b1"])


def _problem(seed, NL=30):
    g = torch.Generator().manual_seed(seed)
    pos = torch.randn(NL, 3, generator=g) * 2.0
    h = torch.randn(NL, 128, generator=g)
    fc = synth.fc_bond_index(NL)
    return pos, h, fc[0], fc[1]


@pytest.mark.parametrize("seed", [0, 1])
def test_factorised_head_equals_reference_head(seed):
    cfg, m = _model("pre_att", seed)
    sd = m.state_dict()
    form = packing.bond_head_pre_att(sd, cfg)
    W1, b1, off = sd["bond_inference.0.weight"], sd["bond_inference.0.bias"], sd["distance_expansion.offset"]
    assert form["coeff"] == -0.5 / (off[1] - off[0]).item() ** 2
    pos, h, src, dst = _problem(seed)
    # fp64: the factorisation is exact algebra
    want64 = _reference_head(W1.double(), b1.double(), off.double(), form["coeff"], pos.double(), h.double(), src, dst)
    got64 = _factorised_head(form, pos.double(), h.double(), src, dst, torch.float64)
    assert float((got64 - want64).abs().max()) < 1e-12
    # fp32: both orders of summation round differently; the bound is a few ulp of the |hidden| ~ 10 values
    want32 = _reference_head(W1, b1, off, form["coeff"], pos, h, src, dst)
    got32 = _factorised_head(form, pos, h, src, dst, torch.float32)
    err = float((got32 - want64).abs().max()), float((want32 - want64).abs().max())
    print(f"pre_att head fp32 maxabs vs fp64: factorised {err[0]:.3g}, reference formula {err[1]:.3g}")
    assert err[0] < 1e-5 and err[1] < 1e-5


def test_packed_slot_holds_the_halved_feature_weights():
    cfg, m = _model("pre_att")
    sd = m.state_dict()
    _, offs, named = packing.pack_model(sd, cfg, kernel_form=True)
    W1 = sd["bond_inference.0.weight"]
    assert torch.equal(named[(-1, "BH_W1")], W1[:, 20:] * 0.5)
    assert torch.equal(named[(-1, "BH_b1")], sd["bond_inference.0.bias"])
    assert len(offs) == cfg.num_layers * len(packing.LAYER_SLOTS) + len(packing.GLOBAL_SLOTS)
    # the lin model's arena is untouched by the new kind
    cfg_l, m_l = _model("lin")
    a0, _, _ = packing.pack_model(m_l.state_dict(), cfg_l, kernel_form=True)
    assert torch.equal(named[(-1, "BH_W2")], sd["bond_inference.2.weight"]) and a0.numel() > 0
    with pytest.raises(ValueError):
        packing.bond_head_pre_att(m_l.state_dict(), cfg)


def test_new_symbols_exported_and_abi_unchanged():
    import __graft_entry__
    __graft_entry__.build()
    lib = hip_lib.load()
    new = ["dd_forward_ex", "dd_sample_steps_ex", "dd_sample_steps_graph_ex", "dd_graph_create_ex", "dd_sample_steps_graph_multi_ex"]
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "decompdiff_hip.h")).read(), flags=re.S)
    for name in new:
        assert name in hip_lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r"\b" + name + r"\s*\(", hdr), name
    assert "typedef struct dd_bond_head" in hdr and "DD_NUM_GLOBAL_SLOTS" in hdr
    assert lib.dd_abi_version() == hip_lib.ABI_VERSION == 9
    assert ctypes.sizeof(hip_lib.DDBondHead) == 48
    # bad descriptors are refused before anything touches a device pointer
    bh = hip_lib.DDBondHead()
    bh.kind = 7
    s = hip_lib.DDSampler()
    assert lib.dd_forward_ex(ctypes.byref(s), ctypes.byref(bh), None) == -1
    bh.kind = hip_lib.BOND_HEAD_PRE_ATT                     # (pre_att without its weights)
    assert lib.dd_sample_steps_ex(ctypes.byref(s), ctypes.byref(bh), 1, None) == -1


def test_fixtures_within_size_limits():
    names = ["forward_preatt", "steps_preatt", "traj3_preatt_b8_plain", "traj3_preatt_b8_drift", "traj20_preatt",
             "loss_grad_preatt", "loss_grad_preatt_ragged"]
    for n in names:
        p = os.path.join(GOLDEN, n + ".npz")
        assert os.path.getsize(p) < 1 << 20, n
        with np.load(p) as z:
            assert len(z.files) > 0
