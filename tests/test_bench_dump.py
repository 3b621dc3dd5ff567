"""CPU: bench.py's --dump-outputs writer (dump_outputs) on synthetic results shaped like a sampling call's: the arrays as
returned while they fit the budget, and the fixed, seeded row sample once they do not."""
import os

import numpy as np
import torch

import bench


def _result(B=8, NL=30, T=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    n, eb = B * NL, B * NL * (NL - 1)
    out = {"pos": torch.randn(n, 3, generator=g), "v": torch.randint(0, 13, (n,), generator=g),
           "bond": torch.randint(0, 5, (eb,), generator=g)}
    shapes = {"pos_traj": (n, 3), "v_traj": (n,), "bond_traj": (eb,), "v0_traj": (n, 13), "vt_traj": (n, 13), "bt_traj": (eb, 5)}
    for k, shp in shapes.items():
        out[k] = list(torch.randn((T,) + shp, generator=g).unbind(0))
    out["pos_traj"][-1] = out["pos"].clone()             # (as in a real call: the last frame is the returned state)
    out["v_traj"][-1] = out["v"].float()
    out["bond_traj"][-1] = out["bond"].float()
    return out


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_the_returned_arrays_and_the_last_frames(tmp_path):
    out = _result()
    bench.dump_outputs(out, str(tmp_path))
    got = _load(tmp_path)
    assert set(got) == {"pos", "v", "bond"} | {k + "_last" for k in bench.TRAJ_KEYS}
    assert all(a.dtype == np.float32 for a in got.values())
    for k in ("pos", "v", "bond"):
        assert np.array_equal(got[k], out[k].float().numpy()), k
    for k in bench.TRAJ_KEYS:
        assert np.array_equal(got[k + "_last"], out[k][-1].numpy()), k
    # a call without trajectories: the three returned arrays only
    no_traj = {k: v for k, v in out.items() if k in ("pos", "v", "bond")}
    no_traj.update({k: [] for k in bench.TRAJ_KEYS})
    bench.dump_outputs(no_traj, str(tmp_path / "plain"))
    assert set(_load(tmp_path / "plain")) == {"pos", "v", "bond"}


def test_dump_beyond_the_budget_keeps_a_fixed_seeded_row_sample(tmp_path, monkeypatch):
    out = _result()
    full = sum(a.numel() * 4 for a in [out["pos"], out["v"], out["bond"]] + [out[k][-1] for k in bench.TRAJ_KEYS])
    limit = full // 5
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", limit)
    bench.dump_outputs(out, str(tmp_path / "a"))
    bench.dump_outputs(out, str(tmp_path / "b"))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert 0 < sum(x.nbytes for x in a.values()) <= limit
    for k in a:
        assert np.array_equal(a[k], b[k]), k                       # the same rows in every run
    n, eb = out["pos"].shape[0], out["bond"].shape[0]
    assert a["pos"].shape == (int(n * limit / full), 3) and a["bt_traj_last"].shape == (int(eb * limit / full), 5)
    # one row set per row count: the atom arrays keep the same atoms, the bond arrays the same bonds ...
    assert np.array_equal(a["pos"], a["pos_traj_last"]) and np.array_equal(a["v"], a["v_traj_last"])
    assert np.array_equal(a["bond"], a["bond_traj_last"])
    # ... and those rows are real rows of the result, in their original order
    pos = out["pos"].numpy()
    idx = [int(np.flatnonzero((pos == r).all(1))[0]) for r in a["pos"]]
    assert idx == sorted(set(idx)) and np.array_equal(a["vt_traj_last"], out["vt_traj"][-1].numpy()[idx])


def test_dump_of_a_rank_without_units_writes_nothing(tmp_path):
    bench.dump_outputs(None, str(tmp_path / "none"))
    assert not os.path.exists(tmp_path / "none")
