"""Host tests (no GPU) of refine nets with num_blocks > 1: the model constructs and shares the one-block state dict, the new
C entry points are exported, and every fixture of the GPU cases (tests/blocks_fixtures.py) meets its kNN-gap condition."""
import os
import re

import numpy as np
import pytest
import torch

import blocks_fixtures as BF
import golden_utils as GU
from decompdiff_amd import DecompScorePosNet3D, hip_lib, shipped_config, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS_SYMBOLS = ("dd_forward_opts", "dd_sample_steps_opts", "dd_sample_steps_graph_opts", "dd_graph_create_opts",
                "dd_sample_steps_graph_multi_opts")


def test_two_block_model_constructs_and_shares_the_one_block_state_dict():
    one = DecompScorePosNet3D(shipped_config(), 29, 10, 8)
    two = DecompScorePosNet3D(shipped_config(num_blocks=2), 29, 10, 8)
    assert two.config.num_blocks == 2
    assert len(two.state_dict()) == 616 and set(two.state_dict()) == set(one.state_dict())
    sd = one.state_dict()
    sd.update(synth.synthetic_state_dict(shipped_config(), 0))
    two.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, two.state_dict()[k]) for k, v in sd.items())
    DecompScorePosNet3D(shipped_config(num_blocks=10, num_layers=6), 29, 10, 8)           # 60 steps: within the bound
    DecompScorePosNet3D(shipped_config(num_blocks=64, num_layers=1), 29, 10, 8)
    for nb, L in ((11, 6), (0, 6), (65, 1)):
        with pytest.raises(NotImplementedError, match=r"num_blocks \* num_layers <= 64"):
            DecompScorePosNet3D(shipped_config(num_blocks=nb, num_layers=L), 29, 10, 8)


def test_opts_entry_points_exported_and_abi_unchanged():
    import __graft_entry__
    __graft_entry__.build()
    lib = hip_lib.load()
    hdr = open(os.path.join(ROOT, "include", "decompdiff_hip.h")).read()
    for name in OPTS_SYMBOLS:
        assert name in hip_lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r"\b" + name + r"\s*\(", hdr), name
    assert "dd_workspace_view_opts" in hip_lib.DEBUG_SYMBOLS and hasattr(lib, "dd_workspace_view_opts")
    assert lib.dd_abi_version() == 9
    # the struct of the binding is the header's: four fields, the size first
    m = re.search(r"typedef struct dd_model_opts \{(.*?)\} dd_model_opts;", hdr, flags=re.S)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [f[0] for f in hip_lib.DDModelOpts._fields_] == ["size", "bond_head", "node_out", "num_blocks"]
    o = hip_lib.model_opts(num_blocks=3)
    assert o.size == 32 and o.num_blocks == 3 and not o.bond_head and not o.node_out


# ---------------------------------------------------------------------------------------------- the fixtures' condition
def _assert_gaps(tag, gaps, n_expected=None):
    assert gaps and (n_expected is None or len(gaps) == n_expected), (tag, gaps)
    print(f"{tag}: smallest K-th / (K+1)-th neighbour gap at {len(gaps)} block boundaries {min(gaps):.3g} A")
    assert min(gaps) >= BF.MIN_GAP, (tag, gaps)


@pytest.mark.parametrize("name", [n for n in BF.FORWARD if not n.endswith(("preatt", "outfc"))])
def test_forward_fixtures_keep_their_distance_from_a_neighbour_tie(name):
    f = BF.FORWARD[name]
    cfg, sd = GU.weights(0, BF.config(f["nb"], f["L"], **f["over"]))
    with BF.boundary_gaps(cfg.knn) as gaps:
        BF.oracle_forward(sd, cfg, BF.forward_batch(name))
    _assert_gaps(name, gaps, f["nb"] - 1)


@pytest.mark.parametrize("name", ["2x3_preatt", "2x3_outfc", "noise_step"])
def test_reference_fixtures_keep_their_distance_from_a_neighbour_tie(name):
    """Fixtures the oracle does not restate (pre_att head, node output MLPs, noise parameterisation) come from the reference
    itself (tools/make_blocks_golden.py), which stored the coordinates its kNN calls saw at every block boundary."""
    g = GU.load("blocks_ref")
    xs, bv = g[name + "_boundary_x"], torch.from_numpy(g[name + "_boundary_batch"])
    gaps = [BF.knn_gap(torch.from_numpy(x), bv, 32) for x in xs]
    _assert_gaps(name, gaps, 1)


@pytest.mark.parametrize("specs,seed", [(BF.RAGGED, BF.RAGGED_SEED), (BF.TINY, BF.TINY_SEED)], ids=["ragged", "tiny"])
def test_ragged_fixtures_keep_their_distance_from_a_neighbour_tie(specs, seed):
    cfg, sd = GU.weights(0, BF.config(2, 3))
    gaps = []
    for b in BF.ragged_parts(specs, seed):
        with BF.boundary_gaps(cfg.knn) as g:
            BF.oracle_forward(sd, cfg, b)
        gaps += [x for x in g if np.isfinite(x)]           # (a sample with N - 1 <= K has a complete graph: exempt)
    _assert_gaps("ragged batch", gaps)


def test_sampling_fixtures_keep_their_distance_from_a_neighbour_tie():
    s = BF.SAMPLING
    cfg, sd = GU.weights(0, BF.config(s["nb"], s["L"]))
    b, noise = BF.sampling_inputs()
    with BF.boundary_gaps(cfg.knn) as gaps:
        for t in (999, 500, 0):
            BF.oracle_chain(sd, cfg, b, noise, 1, None, t_start=t)
        BF.oracle_chain(sd, cfg, b, noise, 10, GU.DRIFT)
        for part, n in zip(*BF.ragged_chain_inputs(3)):    # the padded-against-groups chain
            BF.oracle_chain(sd, cfg, part, n, 3)
    _assert_gaps("sampling", gaps, 3 + 10 + 9)


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
def test_training_fixtures_keep_their_distance_from_a_neighbour_tie(ragged):
    b, t = BF.training_batch(ragged)
    cfg = BF.config(t["nb"], t["L"])
    m = DecompScorePosNet3D(cfg, 29, 10, 8)
    sd = synth.synthetic_state_dict(cfg, 0)
    x = BF.perturbed_network_inputs(m, BF.loss_kwargs(b, t["time_step"], "cpu"), t["seed"])
    with BF.boundary_gaps(cfg.knn) as gaps:
        BF.oracle_forward(sd, cfg, x)
    _assert_gaps("training " + ("ragged" if ragged else "dense"), gaps, 1)
