"""The narrow bond layer (h_node_in_bond_net = False, uni_transformer_edge.py:147-152) on the host: configuration, module tree,
weights, packing, and how the library learns the width from the slot table.  `zero_extend` is the identity the GPU cases of
tests/hnode_cases.py rest on: a wide model whose atom columns are zero computes what the narrow model computes."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from decompdiff_amd import DecompScorePosNet3D, hip_lib, packing, shipped_config, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["forward_hnode", "forward_hnode_preatt_outfc", "steps_hnode", "traj3_hnode_b8_plain", "traj3_hnode_b8_drift", "traj20_hnode",
            "loss_grad_hnode", "loss_grad_hnode_ragged"]
# size of each fixture's x2h_out_fc sibling, rounded up
SIZE_LIMIT = {"forward_hnode": 16 << 10, "forward_hnode_preatt_outfc": 16 << 10, "steps_hnode": 400 << 10, "traj3_hnode_b8_plain": 300 << 10,
              "traj3_hnode_b8_drift": 300 << 10, "traj20_hnode": 100 << 10, "loss_grad_hnode": 640 << 10, "loss_grad_hnode_ragged": 640 << 10}


def narrow_config(**over):
    return shipped_config(h_node_in_bond_net=False, **over)


def zero_extend(sd):
    """A narrow state dict as the wide one that computes the same: hk / hv get zero columns [181:437], hq zero columns [128:256]."""
    out = {}
    for k, v in sd.items():
        m = re.search(r"\.bond_layer\.(hk|hv|hq)_func\.net\.0\.weight$", k)
        if m:
            narrow, wide = (128, 256) if m.group(1) == "hq" else (181, 437)
            assert v.shape == (128, narrow), (k, v.shape)
            v = torch.cat([v, torch.zeros(128, wide - narrow, dtype=v.dtype, device=v.device)], 1)
        out[k] = v
    return out


def _model(cfg, sd=None):
    m = DecompScorePosNet3D(cfg, 29, 10, 8)
    full = m.state_dict()
    full.update(synth.synthetic_state_dict(cfg, 0) if sd is None else sd)
    m.load_state_dict(full, strict=True)
    return m


def test_construction_and_state_dict_equal_the_reference_key_list():
    m = _model(narrow_config())                           # (the parent commit raises NotImplementedError here)
    assert m.h_node_in_bond_net is False and _model(shipped_config()).h_node_in_bond_net is True
    want = json.load(open(os.path.join(GOLDEN, "hnode_keys.json")))
    got = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert len(want) == 616 and got == want
    learn = [p for p in m.parameters() if p.requires_grad]
    assert len(learn) == 572
    learn_keys = {k for k, p in m.named_parameters() if p.requires_grad}
    n_ref = sum(int(np.prod(s)) for k, s in want.items() if k in learn_keys)
    assert sum(p.numel() for p in learn) == n_ref == 4483749
    p = "refine_net.base_block.4.bond_layer."
    assert [got[p + f + "_func.net.0.weight"] for f in ("hk", "hv", "hq")] == [[128, 181], [128, 181], [128, 128]]
    # everything else has the wide model's shape
    wide = {k: list(v.shape) for k, v in _model(shipped_config()).state_dict().items()}
    assert set(wide) == set(got)
    assert sorted(k for k in got if got[k] != wide[k]) == sorted(
        f"refine_net.base_block.{l}.bond_layer.{f}_func.net.0.weight" for l in range(6) for f in ("hk", "hv", "hq"))


def test_a_config_without_the_key_is_the_narrow_model():
    """The encoder's constructor default (uni_transformer_edge.py:294) is False."""
    cfg = narrow_config()
    del cfg.h_node_in_bond_net
    assert DecompScorePosNet3D(cfg, 29, 10, 8).state_dict()["refine_net.base_block.0.bond_layer.hq_func.net.0.weight"].shape == (128, 128)


def test_strict_loading_fails_across_the_widths():
    narrow, wide = _model(narrow_config()), _model(shipped_config())
    DecompScorePosNet3D(narrow_config(), 29, 10, 8).load_state_dict(narrow.state_dict(), strict=True)
    with pytest.raises(RuntimeError):
        DecompScorePosNet3D(shipped_config(), 29, 10, 8).load_state_dict(narrow.state_dict(), strict=True)
    with pytest.raises(RuntimeError):
        DecompScorePosNet3D(narrow_config(), 29, 10, 8).load_state_dict(wide.state_dict(), strict=True)
    # the zero extension of a narrow checkpoint IS a wide checkpoint
    DecompScorePosNet3D(shipped_config(), 29, 10, 8).load_state_dict(zero_extend(narrow.state_dict()), strict=True)


def test_sync_twoup_constructs_and_shipped_config_is_unchanged():
    cfg = shipped_config()
    assert cfg.h_node_in_bond_net is True and cfg.sync_twoup is False
    for h_node in (False, True):
        a = DecompScorePosNet3D(shipped_config(h_node_in_bond_net=h_node, sync_twoup=True), 29, 10, 8).state_dict()
        b = DecompScorePosNet3D(shipped_config(h_node_in_bond_net=h_node), 29, 10, 8).state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("kernel_form", [False, True])
def test_packing_narrow_against_its_zero_extension(kernel_form):
    cfg_n, cfg_w = narrow_config(), shipped_config()
    sd = {k: v for k, v in _model(cfg_n).state_dict().items()}
    _, off_n, named_n = packing.pack_model(sd, cfg_n, kernel_form=kernel_form)
    _, off_w, named_w = packing.pack_model(zero_extend(sd), cfg_w, kernel_form=kernel_form)
    assert list(named_n) == list(named_w)
    for key in named_n:
        n, w = named_n[key], named_w[key]
        if key[1] == "W_l1":
            assert n.shape == (640, 128) and w.shape == (1280, 128)
            assert torch.equal(n, w[:640]) and not bool(w[640:].any())
        elif key[1] == "b_l1":
            assert n.shape == (640,) and w.shape == (1280,)
            assert torch.equal(n, w[:640]) and not bool(w[640:].any())
        else:
            assert n.shape == w.shape and torch.equal(n, w), key
    # what the library reads: rows of W_l1 from the slot table, exact in both models and in every layer
    ns = len(packing.LAYER_SLOTS)
    i_w, i_b = packing.LAYER_SLOTS.index("W_l1"), packing.LAYER_SLOTS.index("b_l1")
    assert i_b == i_w + 1
    for l in range(cfg_n.num_layers):
        assert int(off_n[l * ns + i_b] - off_n[l * ns + i_w]) == 640 * 128
        assert int(off_w[l * ns + i_b] - off_w[l * ns + i_w]) == 1280 * 128


def test_packing_refuses_other_widths():
    sd = dict(_model(narrow_config()).state_dict())
    k = "refine_net.base_block.2.bond_layer.hq_func.net.0.weight"
    sd[k] = torch.cat([sd[k], torch.zeros(128, 128)], 1)           # hq wide, hk / hv narrow
    with pytest.raises(ValueError):
        packing.pack_model(sd, narrow_config())


def _bare_sampler(offsets):
    """A dd_sampler that passes the argument checks up to the slot table and nothing else: the pointers are never followed."""
    keep = np.zeros(16, dtype=np.float32)
    s = hip_lib.DDSampler()
    s.B, s.NP, s.NL, s.K, s.num_layers, s.T = 1, 8, 4, 4, 6, 1000
    s.weights = s.workspace = keep.ctypes.data
    s.workspace_floats = 0                                # (too small: what a well-formed slot table is answered with)
    s.slot_off = offsets.ctypes.data
    return s, keep


def test_library_reads_the_width_from_the_slot_table_and_refuses_other_sizes():
    import __graft_entry__
    __graft_entry__.build()
    lib = hip_lib.load()
    assert lib.dd_abi_version() == hip_lib.ABI_VERSION == 9
    ns = len(packing.LAYER_SLOTS)
    i_w = packing.LAYER_SLOTS.index("W_l1")
    for cfg in (narrow_config(), shipped_config()):
        sd = dict(_model(cfg).state_dict())
        _, off, _ = packing.pack_model(sd, cfg)
        good = off.numpy().astype(np.int64).copy()
        s, keep = _bare_sampler(good)
        # a well-formed table of either width gets past the width check (and stops at the next one: the workspace size)
        assert lib.dd_forward_opts(ctypes.byref(s), None, None) == -3
        for layer, rows in ((0, 512), (0, 1920), (3, 640 if cfg.h_node_in_bond_net else 1280), (5, 0)):
            bad = good.copy()
            bad[layer * ns + i_w + 1:] += (rows * 128) - int(good[layer * ns + i_w + 1] - good[layer * ns + i_w])
            s, keep = _bare_sampler(bad)
            assert lib.dd_forward_opts(ctypes.byref(s), None, None) == -1, (layer, rows)


def test_header_documents_the_width_and_model_opts_is_untouched():
    hdr = open(os.path.join(ROOT, "include", "decompdiff_hip.h")).read()
    m = re.search(r"const int64_t\* slot_off;\s*/\*(.*?)\*/", hdr, flags=re.S)
    assert m and "1280" in m.group(1) and "640" in m.group(1) and "DD_ERR_BAD_ARG" in m.group(1)
    body = re.search(r"typedef struct dd_model_opts \{(.*?)\} dd_model_opts;", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S), flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*;", body) == ["size", "bond_head", "node_out", "num_blocks"]
    assert [f[0] for f in hip_lib.DDModelOpts._fields_] == ["size", "bond_head", "node_out", "num_blocks"]
    assert ctypes.sizeof(hip_lib.DDModelOpts) == 32 and ctypes.sizeof(hip_lib.DDBondHead) == 48


def test_fixtures_within_the_size_of_their_siblings():
    for n in FIXTURES:
        p = os.path.join(GOLDEN, n + ".npz")
        assert os.path.getsize(p) < SIZE_LIMIT[n], (n, os.path.getsize(p))
        with np.load(p) as z:
            assert len(z.files) > 0
