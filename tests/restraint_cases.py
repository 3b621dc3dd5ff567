"""Deterministic cases for the distance-restraint drift kernel (k_drift_restraint in csrc/dd_step.hip, dd_drift_restraint), with the
project's own energy restated in torch and its gradient under autograd in float64 (the yardstick) and in fp32.  Both precisions see
the same fp32-representable inputs, cast up.  A plain helper module (no tests): tests/test_restraint_cases_host.py checks that every
case is what it says it is, tests/test_gpu_restraint.py runs the kernel.

    d_r = | x_w - p_r |,  w = the explicit atom, or the FIRST nearest member of the group in row order
    E   = sum_r  w_r * ( clamp(min_d_r - d_r, min=0) + clamp(d_r - max_d_r, min=0) )

Bounds follow drift_cases.bound with the flat tolerance FLAT["armsca"] times the case's largest weight (the same arithmetic: a unit
vector times a coefficient): flat where the fp32 oracle is within a quarter of it of the float64 one, else twice the fp32 oracle's own
distance; always from the two oracle runs, never from the kernel's output.

Random geometries are kept only at seeds where the float64 oracle alone has every hinge argument (min_d - d, d - max_d; finite
bounds of restraints with a winner) at least HINGE_MARGIN from zero and every winner at least WINNER_MARGIN (relative) ahead of its
runner-up (find_seed below chose the seeds written into the table; the host test asserts the margins, and that the fp32 oracle takes
the same winners and branches).  Nothing is filtered when the kernel runs.

A sample of at most 2 atoms collects all of its restraints' unit vectors on one or two rows; so that the sum stays a handful of terms
(every term is rounded at the magnitude of the running sum) nine in ten of such a sample's restraints are free (min_d = 0,
max_d = inf): they still run through the reduction and report dist / winner."""
import functools
import math

import torch

import drift_cases as DC
from decompdiff_amd import RESTRAINT_ANY

FLAT = DC.FLAT["armsca"]
HINGE_MARGIN, WINNER_MARGIN = DC.HINGE_MARGIN, DC.WINNER_MARGIN
ANY, SCA = RESTRAINT_ANY, -1
ABSENT_ARM = 9                       # an arm id no case's decomp holds
INF = math.inf


def bound(d32, wmax):
    flat = FLAT * max(wmax, 1.0e-30)
    assert d32 <= DC.D32_MAX_FACTOR * flat, f"fp32 oracle is {d32:.3g} from fp64: tame the case"
    return flat if d32 <= 0.25 * flat else max(flat, 2.0 * d32)


def _case(B, NL, pos, decomp, rs, nl_real=None, **kw):
    """rs: list of (sample, point, min_d, max_d, weight, atom (row within the sample or -1), group), any order; stored sorted by
    sample (stable) as the kernel takes them, with the CSR ptr."""
    rs = sorted(rs, key=lambda r: r[0])
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    sample = torch.tensor([r[0] for r in rs], dtype=torch.long)
    c = dict(B=B, NL=NL, pos=pos.float().contiguous(), decomp=None if decomp is None else decomp.long(), nl_real=nl_real, R=len(rs),
             sample=sample, point=f32([list(map(float, r[1])) for r in rs]).reshape(-1, 3), min_d=f32([r[2] for r in rs]),
             max_d=f32([r[3] for r in rs]), weight=f32([r[4] for r in rs]), atom=torch.tensor([r[5] for r in rs], dtype=torch.long),
             group=torch.tensor([r[6] for r in rs], dtype=torch.long), random=False)
    c["ptr"] = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(torch.bincount(sample, minlength=B), 0)])
    c.update(kw)
    return c


def members(case, r):
    """Rows (within the sample) that restraint r may pick, in row order."""
    b, NL = int(case["sample"][r]), case["NL"]
    n = NL if case["nl_real"] is None else int(case["nl_real"][b])
    at, gp = int(case["atom"][r]), int(case["group"][r])
    if at >= 0:
        return [at] if at < n else []
    if gp == ANY:
        return list(range(n))
    if case["decomp"] is None:
        return []
    dec = case["decomp"][b * NL:b * NL + n]
    return (dec == gp).nonzero()[:, 0].tolist()


def energy(case, x):
    """E of the module docstring at positions x [B*NL,3] (any dtype) -> (E, dist [R], winner [R], runner-up distance [R])."""
    dt = x.dtype
    E = torch.zeros((), dtype=dt)
    dist, win, second = [], [], []
    for r in range(case["R"]):
        rows = members(case, r)
        if not rows:
            dist.append(INF), win.append(-1), second.append(INF)
            continue
        b = int(case["sample"][r])
        idx = torch.tensor(rows) + b * case["NL"]
        d = torch.norm(x[idx] - case["point"][r].to(dt), p=2, dim=-1)
        k = int(torch.argmin(d.detach()))                                   # the first minimum
        dw = d[k]
        E = E + case["weight"][r].to(dt) * (torch.clamp(case["min_d"][r].to(dt) - dw, min=0) + torch.clamp(dw - case["max_d"][r].to(dt), min=0))
        srt = d.detach().sort().values
        dist.append(float(dw.detach())), win.append(rows[k]), second.append(float(srt[1]) if len(rows) > 1 else INF)
    return E, dist, win, second


def grad(case, dtype):
    x = case["pos"].to(dtype).clone().requires_grad_(True)
    E, dist, win, second = energy(case, x)
    g = torch.autograd.grad(E, x)[0] if E.requires_grad else torch.zeros_like(x.detach())
    return g, dist, win, second


def margins(case, dtype=torch.float64):
    """(smallest |hinge argument| over the finite bounds of restraints with a winner, smallest relative lead of a winner)."""
    _, dist, win, second = grad(case, dtype)
    h, w = INF, INF
    for r in range(case["R"]):
        if win[r] < 0:
            continue
        for bnd in (float(case["min_d"][r]), float(case["max_d"][r])):
            if math.isfinite(bnd):
                h = min(h, abs(dist[r] - bnd))
        if dist[r] > 0:
            w = min(w, (second[r] - dist[r]) / dist[r])
    return h, w


def sides(case, dist):
    return [(d < float(mn), d > float(mx)) for d, mn, mx in zip(dist, case["min_d"], case["max_d"])]


def same_branches(case):
    """Does the fp32 oracle take the winners and hinge branches of the float64 one?"""
    _, d64, w64, _ = grad(case, torch.float64)
    _, d32, w32, _ = grad(case, torch.float32)
    return w64 == w32 and sides(case, d64) == sides(case, d32)


def seed_ok(case):
    h, w = margins(case)
    return h >= HINGE_MARGIN and w >= WINNER_MARGIN and same_branches(case)


def find_seed(build, limit=200):
    """The first seed with the margins of the module docstring (how RANDOM_SEEDS was filled; not used when the tests run)."""
    for seed in range(limit):
        if seed_ok(build(seed)):
            return seed
    raise RuntimeError("no seed with the required margins")


# ============================================================================================== random cases
COUNTS = {1: (70,), 3: (70, 0, 1)}           # restraints per sample: more than a wave, none, one
KINDS = ("atom", "any", "sca", "arm", "absent")


def _decomp(NL, g):
    if NL == 1:
        return torch.tensor([-1])
    return DC._decomp_pattern(NL, g)


def random_case(NL, B, seed, padded=False):
    """B samples of NL atoms (random clouds, drift_cases' arm patterns); sample b carries COUNTS[B][b] restraints that cycle through
    the five target kinds, each with a point 0.8 .. 4 A from a random atom of the sample, min_d in [0.5, 3], max_d - min_d in
    [0.3, 1.5] (every seventh max_d = inf, every ninth min_d = 0), weights in [0.25, 2].  padded: every sample has fewer real atoms
    than NL (the rows behind them hold coordinates of their own, as close to the points as the real ones)."""
    g = DC._gen("restraint", NL, B, seed, padded)
    pos = torch.cat([DC._random_cloud(NL, g, DC.PITCHES[b % 3]) for b in range(B)])
    dec = torch.cat([_decomp(NL, g) for _ in range(B)])
    nl_real = [int(torch.randint(max(1, NL // 2), NL, (1,), generator=g)) for _ in range(B)] if padded else None
    rs, i = [], 0
    for b in range(B):
        n = NL if nl_real is None else nl_real[b]
        arms = sorted(set(dec[b * NL:b * NL + n][dec[b * NL:b * NL + n] >= 0].tolist()))
        for _ in range(COUNTS[B][b]):
            kind = KINDS[i % 5]
            near = int(torch.randint(0, NL if padded else n, (1,), generator=g))      # (padded: padding rows attract points too)
            u = torch.randn(3, generator=g)
            p = pos[b * NL + near] + u / u.norm() * (0.8 + 3.2 * float(torch.rand(1, generator=g)))
            mn = 0.0 if i % 9 == 8 else 0.5 + 2.5 * float(torch.rand(1, generator=g))
            mx = INF if i % 7 == 6 else mn + 0.3 + 1.2 * float(torch.rand(1, generator=g))
            if NL <= 2 and i % 10 != 0:
                mn, mx = 0.0, INF
            w = 0.25 + 1.75 * float(torch.rand(1, generator=g))
            at, gp = -1, ANY
            if kind == "atom":
                at = int(torch.randint(0, n, (1,), generator=g))
            elif kind == "sca":
                gp = SCA
            elif kind == "arm":
                gp = arms[i % len(arms)] if arms else ABSENT_ARM
            elif kind == "absent":
                gp = ABSENT_ARM
            rs.append((b, p.float().tolist(), mn, mx, w, at, gp))
            i += 1
    return _case(B, NL, pos, dec, rs, nl_real=nl_real, random=True)


SIZES = (1, 2, 63, 64, 65, 128)
# (NL, B, padded) -> seed chosen by find_seed(lambda s: random_case(NL, B, s, padded))
RANDOM_SEEDS = {(1, 1, False): 0, (1, 3, False): 0, (2, 1, False): 0, (2, 3, False): 0, (63, 1, False): 0, (63, 3, False): 0,
                (64, 1, False): 0, (64, 3, False): 0, (65, 1, False): 0, (65, 3, False): 0, (128, 1, False): 0, (128, 3, False): 0,
                (64, 3, True): 0, (128, 3, True): 0}


# ========================================================================================= constructed cases
def _lattice(NL, special):
    """NL points of drift_cases' far lattice (pitch 10 A, x >= 10), the rows of `special` replaced."""
    pos = DC._far_filler(NL)
    for row, p in special.items():
        pos[row] = torch.tensor(p, dtype=torch.float32)
    return pos


def constructed():
    c = {}
    # exact ties on the integer lattice (squared distances are integers: exact in fp32 and float64).  One wave: rows 10 and 20 are both
    # 3 from the point, row 10 wins; d = 3 > max_d = 2: the gradient is +w (x - p) / d on row 10 alone.
    c["tie_in_wave_nl64"] = _case(1, 64, _lattice(64, {10: [0, 0, 3], 20: [0, 0, -3]}), None, [(0, [0, 0, 0], 1.0, 2.0, 1.5, -1, ANY)],
                                  winners=[10], expect_rows={10: [0, 0, 1.5]})
    # two waves: rows 40 (first wave) and 100 (second) tie at 3 -> row 40; a second restraint whose nearest atom, row 90, sits in the
    # second wave alone (d = 1 < min_d = 2: -w (x - p) / d); a third whose tie is rows 63 | 64, the two waves' edge lanes
    c["tie_across_waves_nl128"] = _case(
        1, 128, _lattice(128, {40: [0, 3, 0], 100: [0, -3, 0], 90: [-50, 1, 0], 63: [-90, 0, 2], 64: [-90, 0, -2]}), None,
        [(0, [0, 0, 0], 1.0, 2.0, 1.0, -1, ANY), (0, [-50, 0, 0], 2.0, 4.0, 2.0, -1, ANY), (0, [-90, 0, 0], 0.0, 1.0, 0.5, -1, ANY)],
        winners=[40, 90, 63], expect_rows={40: [0, 1, 0], 90: [0, -2, 0], 63: [0, 0, .5]})
    # hinge values, one explicit atom each (rows 0 .. 6 at distance 2 along x from their own points, row 7 ON its point):
    #   d == min_d: the clamp passes its gradient (-w);  d == max_d: (+w);  min_d == max_d == d: the two cancel;  d == 0 below min_d: zero
    #   subgradient, finite;  max_d = inf, d > min_d: nothing;  max_d = inf, d < min_d: -w;  weight 0 on an active hinge: nothing
    pts = {i: [100.0 * i, 0, 0] for i in range(8)}
    pos = _lattice(8, {i: [100.0 * i + 2.0, 0, 0] for i in range(7)})
    pos[7] = torch.tensor(pts[7])
    hinge = [(0, pts[0], 2.0, 5.0, 1.0, 0, ANY), (0, pts[1], 1.0, 2.0, 1.0, 1, ANY), (0, pts[2], 2.0, 2.0, 1.0, 2, ANY),
             (0, pts[7], 1.0, 3.0, 1.0, 7, ANY), (0, pts[3], 1.0, INF, 1.0, 3, ANY), (0, pts[4], 3.0, INF, 0.75, 4, ANY),
             (0, pts[5], 3.0, 4.0, 0.0, 5, ANY), (0, pts[6], 0.0, 1.0, 1.25, 6, ANY)]
    c["hinge_values"] = _case(1, 8, pos, None, hinge, eq={0: "min", 1: "max", 2: "both"}, zero_d=(3,),
                              expect=[[-1, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, 0], [-.75, 0, 0], [0, 0, 0], [1.25, 0, 0], [0, 0, 0]])
    # all four target kinds, an absent arm and arm ids with gaps {0, 2, 5}, B = 3 with nothing on sample 1; NL = 6 rows per sample:
    #   decomp = [0, 2, -1, 5, -1, 2].  Points sit 1 below (in z) their intended winners; min_d = 2 everywhere: -w (x - p) / d = -w z
    dec = torch.tensor([0, 2, -1, 5, -1, 2] * 3)
    rows = [[0, 0, 0], [10, 0, 0], [20, 0, 0], [30, 0, 0], [40, 0, 0], [50, 0, 0]]
    pos = torch.tensor(rows * 3, dtype=torch.float32)
    below = lambda row: [rows[row][0], 0, -1]
    groups = [(0, below(3), 2.0, 9.0, 1.0, 3, ANY),             # explicit atom 3
              (0, below(1), 2.0, 9.0, 1.0, -1, ANY),            # ANY: nearest of all -> row 1
              (0, below(1), 2.0, INF, 1.0, -1, SCA),            # scaffold: rows 2, 4 -> row 2 (d = sqrt(101) > min_d: nothing)
              (0, below(3), 2.0, INF, 1.0, -1, 2),              # arm 2: rows 1, 5 -> tie at sqrt(401) -> row 1, inside: nothing
              (0, below(5), 2.0, 9.0, 0.5, -1, 2),              # arm 2 -> row 5
              (0, below(3), 2.0, 9.0, 2.0, -1, 5),              # arm 5 (ids with gaps) -> row 3
              (0, below(0), 2.0, 9.0, 1.0, -1, 1),              # arm 1: the gap, nobody
              (0, below(0), 2.0, 9.0, 1.0, -1, ABSENT_ARM),     # absent arm
              (2, below(4), 2.0, 9.0, 1.0, -1, SCA)]            # sample 2: scaffold -> row 4
    c["groups_b3"] = _case(3, 6, pos, dec, groups, winners=[3, 1, 2, 1, 5, 3, -1, -1, 4], empty_sample=1,
                           expect_rows={1: [0, 0, -1], 3: [0, 0, -3], 5: [0, 0, -.5], 12 + 4: [0, 0, -1]})
    # the same groups without decomp: arm / scaffold groups are empty, ANY and explicit atoms work
    c["groups_no_decomp"] = _case(1, 6, pos[:6], None, [g for g in groups if g[0] == 0 and g[6] == ANY], winners=[3, 1])
    # padded batch: sample 0 has 5 real atoms of 8, and rows 5 .. 7 hold coordinates; the point is ON padding row 6 and 2 from row 4
    pos = _lattice(16, {4: [0, 0, 2], 6: [0, 0, 0], 8 + 1: [500, 0, 1], 8 + 2: [500, 0, 0]})
    dec = torch.tensor([0, 0, -1, -1, 0, 0, 0, -1] + [-1, 0, 0, -2, -2, -2, -2, -2])
    c["padded_nearest_is_padding"] = _case(
        2, 8, pos, dec, [(0, [0, 0, 0], 3.0, 9.0, 1.0, -1, ANY), (0, [0, 0, 0], 3.0, 9.0, 1.0, -1, 0), (0, [0, 0, 0], 3.0, 9.0, 1.0, 6, ANY),
                         (1, [500, 0, 0], 0.0, 0.5, 1.0, -1, ANY), (1, [500, 0, 0], 0.0, 0.5, 1.0, -1, 0)],
        nl_real=[5, 2], winners=[4, 4, -1, 1, 1], expect_rows={4: [0, 0, -2], 8 + 1: [0, 0, 2]})
    return c


def _build_all():
    c = {}
    for (NL, B, padded), seed in RANDOM_SEEDS.items():
        c[f"random_nl{NL}_b{B}" + ("_padded" if padded else "")] = random_case(NL, B, seed, padded)
    c.update(constructed())
    return c


@functools.lru_cache(maxsize=None)
def all_cases():
    return _build_all()


NAMES = tuple(_build_all())


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(g64, g32, d32, bound, dist [R] float64, dist32 [R], winner [R]) of a case: computed once, shared, never modified."""
    case = all_cases()[name]
    g64, dist, win, _ = grad(case, torch.float64)
    g32, dist32, _, _ = grad(case, torch.float32)
    assert g64.dtype == torch.float64 and g32.dtype == torch.float32
    d32 = float((g64 - g32.double()).abs().max())
    wmax = float(case["weight"].max()) if case["R"] else 1.0
    return dict(g64=g64, g32=g32, d32=d32, bound=bound(d32, wmax), dist=torch.tensor(dist, dtype=torch.float64),
                dist32=torch.tensor(dist32, dtype=torch.float64), winner=torch.tensor(win, dtype=torch.long))


def dist_bound(ref):
    """Distances: sqrt of a three-term fp32 sum of squares of fp32 differences -- four roundings of half an ulp each at the size of the
    result at most (the differences' own half ulp enters twice as a relative error of the square) -> 4 ulp of the largest finite
    distance; or twice the fp32 oracle's own distance where that is more."""
    fin = torch.isfinite(ref["dist"])
    if not bool(fin.any()):
        return 0.0
    big = float(ref["dist"][fin].max())
    ulp = 2.0 ** (math.floor(math.log2(big)) - 23) if big > 0 else 2.0 ** -149
    return max(4.0 * ulp, 2.0 * float((ref["dist"][fin] - ref["dist32"][fin]).abs().max()))


# ============================================================================================ sampler-level cases
SAMPLER_SEED = 0                     # chosen like the seed table above (host test: margins of sampler_case)


def batch_entry(b, seed, per_sample=(4, 4), weight=(0.5, 1.5), **opts):
    """A ``restraint`` entry of energy_drift_opt for the sampling batch `b` (dense or ragged): sample k carries per_sample[k]
    restraints that cycle through explicit atom / ANY / scaffold / arm 0, each with a point 1.5 .. 3 A from a random atom of the
    sample (the frame of protein_pos), min_d = 0.8, max_d in {1.2, inf} -- the first two of a sample pull (d > max_d), every fourth has
    min_d = 4 and pushes --, weights in `weight`.  Restraints are listed sample-interleaved: the caller's order is not sorted."""
    g = DC._gen("restraint_entry", seed)
    bl = b["batch_ligand"]
    pos = b["init_ligand_pos"]
    if pos is None:                                                                  # (init on the device: around the prior centres)
        pos = b["prior_centers"][b["ligand_decomp_batch"]]
    rows = []
    for k, n_r in enumerate(per_sample):
        mine = (bl == k).nonzero()[:, 0]
        for i in range(n_r):
            near = int(mine[int(torch.randint(0, len(mine), (1,), generator=g))])
            u = torch.randn(3, generator=g)
            p = pos[near].float() + u / u.norm() * (1.5 + 1.5 * float(torch.rand(1, generator=g)))
            w = weight[0] + (weight[1] - weight[0]) * float(torch.rand(1, generator=g))
            mn, mx = (4.0, INF) if i % 4 == 3 else (0.8, 1.2)
            at, gp = (near, ANY) if i % 4 == 0 else (-1, (ANY, SCA, 0)[i % 4 - 1])
            rows.append((i, k, p, mn, mx, w, at, gp))
    rows.sort(key=lambda r: (r[0], -r[1]))                                           # interleaved, samples descending
    return dict(type="restraint", sample=torch.tensor([r[1] for r in rows]), point=torch.stack([r[2] for r in rows]).float(),
                min_d=torch.tensor([r[3] for r in rows]), max_d=torch.tensor([r[4] for r in rows]),
                weight=torch.tensor([r[5] for r in rows]), atom=torch.tensor([r[6] for r in rows]),
                group=torch.tensor([r[7] for r in rows]), **opts)


def model_offsets(b):
    """The per-sample centring offset as the model forms it (fp32 sum in row order / count, on the host)."""
    B = int(b["batch_protein"].max()) + 1
    n_p = torch.bincount(b["batch_protein"], minlength=B)
    tot = torch.zeros(B, 3).index_add_(0, b["batch_protein"], b["protein_pos"].float())
    return tot / n_p.float().clamp(min=1).view(B, 1)


def centred_case(b, entry, pos=None):
    """The dense batch `b` (equal ligand sizes) and a restraint entry as a case of this module in the kernel's frame: positions and
    points centred with the fp32 subtraction the model uses, explicit atoms as rows within their sample, restraints sorted by
    sample (stable) -- `order` maps the case's rows back to the entry's."""
    B = int(b["batch_ligand"].max()) + 1
    NL = b["batch_ligand"].numel() // B
    off = model_offsets(b)
    x = (b["init_ligand_pos"] if pos is None else pos).float() - off[b["batch_ligand"]]
    order = torch.sort(entry["sample"], stable=True).indices
    rs = [(int(entry["sample"][r]), (entry["point"][r].float() - off[int(entry["sample"][r])]).tolist(), float(entry["min_d"][r]),
           float(entry["max_d"][r]), float(entry["weight"][r]), int(entry["atom"][r]) - int(entry["sample"][r]) * NL if int(entry["atom"][r]) >= 0 else -1,
           int(entry["group"][r])) for r in order.tolist()]
    return _case(B, NL, x, b["ligand_decomp_index"], rs, order=order, offset=off)


def sampler_case(seed=SAMPLER_SEED, **opts):
    """drift_cases.sampler_batch (40 + 12 atoms, B = 2) with four restraints per sample -> (batch, entry, case in the kernel's frame)."""
    b = DC.sampler_batch()
    e = batch_entry(b, ("sampler", seed), **opts)
    return b, e, centred_case(b, e)


def known_buffer(name, shape):
    return torch.randn(shape, generator=DC._gen("restraint_buffer", name)).float()


def report(name, err, d32, bnd, extra=""):
    print(f"\nRESTRAINT {name} err={err:.3g} d32={d32:.3g} bound={bnd:.3g}{extra}")
