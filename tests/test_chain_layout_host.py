"""Host-side checks of the sampling path's call record, row placement and drift-field parsing (CPU tensors, no GPU): where
the caller's flat rows go in a chain's dense layout (dense, padded, one group), what `_chain_rows` makes of ``fixed`` /
``init`` / ``noise`` there, and the dd_sampler drift fields of every ``energy_drift_opt`` form."""
import pytest
import torch

from decompdiff_amd import batch_layout as BL
from decompdiff_amd.model import _Call, _Placement, _chain_rows, _drift_fields

N_L, N_P = (2, 4, 3), (5, 3, 4)
LAYOUT = BL.BatchLayout(N_P, N_L)
CPU = torch.device("cpu")
BATCH_L = BL.batch_vector(3, list(N_L))
N, NB = sum(N_L), sum(LAYOUT.n_b)
NLM, EBM = 3 * 4, 3 * 4 * 3                                    # dense rows of the batch padded to its largest ligand
OFFSET = torch.tensor([[1.5, -2.25, 0.1], [-7.0, 3.3, 0.7], [0.3, 0.2, -11.0]])


def _identity(batch_l=BATCH_L, n_bonds=NB):
    return _Placement(batch_l, n_bonds)


def _padded(layout=LAYOUT, batch_l=BATCH_L):
    NL = max(layout.n_l)
    _, rows_l, rows_b = layout.padded_rows()
    return _Placement(batch_l, sum(layout.n_b), put_l=rows_l, put_b=rows_b, n_l=layout.B * NL, n_b=layout.B * NL * (NL - 1))


def _groups(layout=LAYOUT):
    return [(g, _Placement(BL.batch_vector(len(g.ids), g.n_l), len(g.rows_b), rows_l=g.rows_l, rows_b=g.rows_b, ids=g.ids, dev=CPU))
            for g in layout.size_groups()]


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def test_padded_placement_puts_flat_rows_at_padded_rows():
    pl = _padded()
    _, rows_l, rows_b = LAYOUT.padded_rows()
    for t, put, rows, n, fill in ((_rand(N, 3), pl.atoms, rows_l, NLM, 0), (torch.arange(1, N + 1, dtype=torch.int32), pl.atoms, rows_l, NLM, -2),
                                  (torch.arange(1, NB + 1, dtype=torch.int32), pl.bonds, rows_b, EBM, 0), (_rand(N, 3), pl.atoms, rows_l, NLM, 0.5)):
        out = put(t, fill)
        assert out.shape[0] == n and out.dtype == t.dtype and torch.equal(out[rows], t)
        rest = torch.ones(n, dtype=torch.bool)
        rest[rows] = False
        assert bool((out[rest] == fill).all()) and int(rest.sum()) == n - t.shape[0]
    noise = _rand(2, N, 8)                                     # (injected noise: rows along dim 1)
    out = pl.atoms(noise, 0.5, dim=1)
    assert out.shape == (2, NLM, 8) and torch.equal(out[:, rows_l], noise)


def test_identity_placement_is_the_tensor_itself():
    lay = BL.BatchLayout((4, 4), (3, 3))
    ident = _identity(BL.batch_vector(2, 3), sum(lay.n_b))
    pad = _padded(lay, BL.batch_vector(2, 3))
    for t, a, b in ((_rand(6, 3), ident.atoms, pad.atoms), (torch.arange(6, dtype=torch.int32), ident.atoms, pad.atoms),
                    (torch.arange(12, dtype=torch.int32), ident.bonds, pad.bonds)):
        assert a(t).data_ptr() == t.data_ptr() and a(t).reshape(2, -1).data_ptr() == t.data_ptr()
        assert torch.equal(a(t), b(t))                         # equal sizes: nothing is padding


def test_group_placement_selects_the_groups_rows():
    atoms, bonds = _rand(N, 3), torch.arange(NB, dtype=torch.int32)
    for g, pl in _groups():
        assert torch.equal(pl.atoms(atoms), atoms[g.rows_l]) and torch.equal(pl.bonds(bonds), bonds[g.rows_b])
        assert torch.equal(pl.take(_rand(2, N, 3, seed=1), dim=1), _rand(2, N, 3, seed=1)[:, g.rows_l])


def _fixed(mode, with_cc):
    mask = torch.tensor([True, False, False, True, True, False, True, False, True])
    return dict(mode=mode, init="draw" if mode == "replace" else None, mask=mask, pos=_rand(N, 3, seed=2),
                v=torch.arange(N, dtype=torch.int32) % 7, bond=torch.arange(NB, dtype=torch.int32) % 5, cc=_rand(N, 3, seed=3) if with_cc else None)


def _init(mode):
    ini = dict(mode=mode, cen=_rand(N, 3, seed=4), std=_rand(N, 3, seed=5).abs(), atom_lp=None, bond_lp=torch.zeros(5), pos=None, v=None, bond=None)
    if mode == "noised":
        ini.update(pos=_rand(N, 3, seed=6), v=torch.arange(N, dtype=torch.int32) % 8, bond=torch.arange(NB, dtype=torch.int32) % 5)
    return ini


def _lay(call, pl, offset):
    stds, decomp_batch = _rand(4, 3, seed=7).abs(), torch.tensor([0, 0, 1, 1, 2, 2, 3, 3, 3])
    return _chain_rows(call, pl, offset, stds, decomp_batch, torch.arange(N) % 3 - 1, 8), stds[decomp_batch]


@pytest.mark.parametrize("fixed_mode,with_cc,init_mode", [("hold", False, "prior"), ("replace", True, "noised"), ("hold", True, "noised")])
def test_chain_rows_centre_and_place_fixed_and_init(fixed_mode, with_cc, init_mode):
    fx, ini = _fixed(fixed_mode, with_cc), _init(init_mode)
    call = _Call(1000, 4, fixed=fx, chain_init=ini, sample_keys=torch.tensor([11, 12, 13]))
    off_l = OFFSET[BATCH_L]
    _, rows_l, rows_b = LAYOUT.padded_rows()
    cases = [(_identity(), OFFSET, torch.arange(N), torch.arange(NB), torch.arange(N), torch.arange(NB), [0, 1, 2]),
             (_padded(), OFFSET, torch.arange(N), torch.arange(NB), rows_l, rows_b, [0, 1, 2])]
    cases += [(pl, OFFSET[g.ids], g.rows_l, g.rows_b, torch.arange(len(g.rows_l)), torch.arange(len(g.rows_b)), g.ids) for g, pl in _groups()]
    for pl, offset, flat_l, flat_b, at_l, at_b, ids in cases:      # flat rows flat_* of the call lie at rows at_* of the chain
        rows, atom_std = _lay(call, pl, offset)
        assert torch.equal(rows["keys"], call.sample_keys[ids])
        if pl.rows_l is None:                                      # (a group's chain gets batch tensors of its own: not laid here)
            assert torch.equal(rows["atom_std"][at_l], atom_std)
        f, c = rows["fx"], rows["ci"]
        assert f["mode"] == fixed_mode and f["init"] == fx["init"] and c["mode"] == init_mode and c["bond_lp"] is ini["bond_lp"]
        assert f["mask"].dtype == torch.uint8 and torch.equal(f["mask"][at_l].bool(), fx["mask"][flat_l])
        assert torch.equal(f["v0"][at_l], fx["v"][flat_l]) and torch.equal(f["b0"][at_b], fx["bond"][flat_b])
        assert torch.equal(f["x0c"][at_l], (fx["pos"] - off_l)[flat_l])
        assert (f["cc"] is None) == (not with_cc) and (f["cc"] is None or torch.equal(f["cc"][at_l], (fx["cc"] - off_l)[flat_l]))
        assert torch.equal(c["cc"][at_l], (ini["cen"] - off_l)[flat_l]) and torch.equal(c["std"][at_l], ini["std"][flat_l])
        if init_mode == "noised":
            assert torch.equal(c["x0c"][at_l], (ini["pos"] - off_l)[flat_l])
            assert torch.equal(c["v0"][at_l], ini["v"][flat_l]) and torch.equal(c["b0"][at_b], ini["bond"][flat_b])
        else:
            assert c["x0c"] is None and c["v0"] is None and c["b0"] is None
        if pl.put_l is not None:                                   # padding rows: the documented fills
            pad_l, pad_b = torch.ones(NLM, dtype=torch.bool), torch.ones(EBM, dtype=torch.bool)
            pad_l[rows_l], pad_b[rows_b] = False, False
            for t in (f["mask"], f["v0"], f["x0c"], f["cc"], c["cc"], c["std"], c["x0c"], c["v0"], rows["atom_std"]):
                assert t is None or (t.shape[0] == NLM and not bool(t[pad_l].any()))
            for t in (f["b0"], c["b0"]):
                assert t is None or (t.shape[0] == EBM and not bool(t[pad_b].any()))
            assert bool((rows["decomp"][pad_l] == -2).all()) and torch.equal(rows["decomp"][rows_l], (torch.arange(N) % 3 - 1).int())


def test_chain_rows_without_per_row_inputs_and_noise():
    rows, atom_std = _lay(_Call(1000, 4), _identity(), OFFSET)
    assert all(rows[k] is None for k in ("fx", "ci", "noise", "keys", "fpp")) and torch.equal(rows["atom_std"], atom_std)
    noise = dict(u_v=_rand(2, N, 8), u_b=_rand(2, NB, 5, seed=1), eps=_rand(2, N, 3, seed=2))
    _, rows_l, rows_b = LAYOUT.padded_rows()
    pad = _lay(_Call(1000, 2, noise=noise), _padded(), OFFSET)[0]["noise"]
    assert pad["u_v"].shape == (2, NLM, 8) and pad["u_b"].shape == (2, EBM, 5) and pad["eps"].shape == (2, NLM, 3)
    assert all(torch.equal(pad[k][:, r], noise[k]) for k, r in (("u_v", rows_l), ("u_b", rows_b), ("eps", rows_l)))
    rest_l, rest_b = torch.ones(NLM, dtype=torch.bool), torch.ones(EBM, dtype=torch.bool)
    rest_l[rows_l], rest_b[rows_b] = False, False
    assert bool((pad["u_v"][:, rest_l] == 0.5).all()) and bool((pad["u_b"][:, rest_b] == 0.5).all()) and not bool(pad["eps"][:, rest_l].any())
    for g, pl in _groups():
        sub = _lay(_Call(1000, 2, noise=noise), pl, OFFSET[g.ids])[0]["noise"]
        assert torch.equal(sub["u_v"], noise["u_v"][:, g.rows_l]) and torch.equal(sub["u_b"], noise["u_b"][:, g.rows_b])
    for pl in (_identity(), _padded()):
        with pytest.raises(ValueError) as e:
            _lay(_Call(1000, 3, noise=noise), pl, OFFSET)
        assert str(e.value) == f"noise['u_v'] must have shape {(3, N, 8)}, got {(2, N, 8)}"


def test_clash_drift_needs_the_full_protein():
    with pytest.raises(ValueError, match="clash drift needs full_protein_pos / full_batch_protein"):
        _lay(_Call(1000, 2, drift=[dict(type="clash", sigma=25.0, gamma=1.0)]), _identity(), OFFSET)


def test_call_record_checks_the_step_range_once():
    c = _Call(1000, 20, start_step=5, resample=dict(n_total=36))
    assert (c.t_start, c.n_pos, _Call(1000, 20).n_pos, c.seed, c.keep_traj, c.use_graph) == (994, 36, 20, 0, True, True)
    for steps, start in ((1001, 0), (10, 991), (1, -1)):
        with pytest.raises(ValueError, match=r"num_steps \(\+ start_step\) exceeds num_timesteps"):
            _Call(1000, steps, start_step=start)


ZERO = dict(drift_armsca=0, armsca_min_d=0, armsca_max_d=0, armsca_scale=0, drift_clash=0, clash_sigma=0, clash_gamma=0, clash_scale=0,
            drift_repul=0, repul_max_d=0, repul_scale=0)


@pytest.mark.parametrize("drift,want", [
    (None, {}), ([], {}),
    ([dict(type="armsca_prox", min_d=1.2, max_d=1.9)], dict(drift_armsca=1, armsca_min_d=1.2, armsca_max_d=1.9)),
    ([dict(type="armsca_prox", min_d=1.0, max_d=2.0, scale=True)], dict(drift_armsca=1, armsca_min_d=1.0, armsca_max_d=2.0, armsca_scale=1)),
    ([dict(type="clash", sigma=25.0, gamma=1.0)], dict(drift_clash=1, clash_sigma=25.0, clash_gamma=1.0)),
    ([dict(type="clash", sigma=20, gamma=2, scale=1)], dict(drift_clash=1, clash_sigma=20.0, clash_gamma=2.0, clash_scale=1)),
    ([dict(type="arms_repul")], dict(drift_repul=1, repul_max_d=1.9)),
    ([dict(type="arms_repul", mode="min", max_d=2.5, scale=True)], dict(drift_repul=1, repul_max_d=2.5, repul_scale=1)),
    ([dict(type="arms_repul", mode="all")], dict(drift_repul=2, repul_max_d=1.9)),
    ([dict(type="arms_repul", mode="all", scale=True), dict(type="clash", sigma=25.0, gamma=1.0)],
     dict(drift_repul=2, repul_max_d=1.9, repul_scale=1, drift_clash=1, clash_sigma=25.0, clash_gamma=1.0)),
])
def test_drift_fields(drift, want):
    got = _drift_fields(drift, True)
    assert got == dict(ZERO, **want) and all(type(got[k]) is type(v) for k, v in want.items())


@pytest.mark.parametrize("drift,has_decomp,exc,msg", [
    ([dict(type="clash", sigma=1, gamma=1), dict(type="clash", sigma=2, gamma=1)], True, NotImplementedError, "energy_drift_opt lists 'clash' twice"),
    ([dict(type="pull")], True, ValueError, "pull"),
    ([dict(type="center_prox")], True, NotImplementedError,
     "drift 'center_prox' is outside the shipped sampling path (center_prox raises in the reference; mmff_min is RDKit/CPU)"),
    ([dict(type="mmff_min")], True, NotImplementedError,
     "drift 'mmff_min' is outside the shipped sampling path (center_prox raises in the reference; mmff_min is RDKit/CPU)"),
    ([dict(type="arms_repul", mode="max")], True, ValueError, "max"),
    ([dict(type="arms_repul")], False, ValueError, "arms_repul drift needs ligand_decomp_index"),
])
def test_drift_field_errors(drift, has_decomp, exc, msg):
    with pytest.raises(exc) as e:
        _drift_fields(drift, has_decomp)
    assert type(e.value) is exc and str(e.value) == msg
