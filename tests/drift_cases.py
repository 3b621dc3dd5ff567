"""Deterministic edge-of-domain cases for the three drift guidance kernels (k_drift_armsca, k_drift_clash, k_drift_arms_repul in
csrc/dd_step.hip), with the gradient of the oracle's energy under autograd in float64 (the yardstick) and in fp32 (the suite's
reference as it is).  Both precisions see the same fp32-representable inputs, cast up.  A plain helper module (no tests):
tests/test_drift_cases_host.py checks that every case is what it says it is, tests/test_gpu_drift_edges.py runs the kernels.

Bounds follow stress_weights.bound with the flat tolerances of test_drift_gradients_match_autograd (1e-6 armsca and arms_repul,
1e-5 clash): flat where the fp32 oracle is within a quarter of it of the fp64 one, else twice the fp32 oracle's own distance
(never below the flat tolerance, as in stress_weights.bound); always from the two oracle runs, never from a kernel's output.

Random geometries are kept only at seeds where the float64 oracle alone has every hinge argument (d - min_d, d - max_d,
max_d - d, gamma - G) at least HINGE_MARGIN from zero and every winner at least WINNER_MARGIN (relative) ahead of its runner-up
(find_seed below chose the seeds written into the tables; the host test asserts the margins, and that the fp32 oracle takes the
same winners and branches).  Nothing is filtered when the kernels run."""
import functools
import math

import torch

from oracle import diffusion as OD

FLAT = {"armsca": 1e-6, "repul": 1e-6, "clash": 1e-5}
D32_MAX_FACTOR = 10.0               # an fp32 oracle further than ten flat tolerances from fp64: too ill-conditioned to judge
HINGE_MARGIN, WINNER_MARGIN = 1e-3, 1e-4
MIN_D, MAX_D = 1.2, 1.9             # the project's armsca setting (BASELINE configs[2])
FAR = 10.0                          # lattice pitch of the "everything else is far away" filler atoms


def bound(kind, d32):
    flat = FLAT[kind]
    assert d32 <= D32_MAX_FACTOR * flat, f"fp32 oracle is {d32:.3g} from fp64 ({kind}): tame the case"
    return flat if d32 <= 0.25 * flat else max(flat, 2.0 * d32)


def _gen(*key):
    return torch.Generator().manual_seed(hash_key(*key))


def hash_key(*key):
    h = 1469598103934665603
    for k in key:
        for ch in str(k) + "|":
            h = ((h ^ ord(ch)) * 1099511628211) % (1 << 62)
    return h


def _batch_index(B, NL):
    return torch.arange(B).repeat_interleave(NL)


# ==================================================================================================== armsca
def _decomp_pattern(NL, g):
    """Arm ids for NL atoms: about 40 % scaffold (-1), the rest in up to 4 arms of unequal size, shuffled; every arm and the
    scaffold have at least one atom."""
    if NL == 2:
        return torch.tensor([0, -1])
    n_arms = min(4, max(1, NL // 3)) if NL > 3 else 2
    n_sca = max(1, int(round(0.4 * NL)))
    ids = [-1] * n_sca + list(range(n_arms))
    while len(ids) < NL:
        a = int(torch.randint(0, n_arms, (1,), generator=g))
        ids.append(min(a, int(torch.randint(0, n_arms, (1,), generator=g))))       # (low ids get more atoms)
    ids = torch.tensor(ids[:NL])
    return ids[torch.randperm(NL, generator=g)]


PITCHES = (2.4, 1.7, 3.0)          # per sample of a batch


def _random_cloud(NL, g, pitch=1.7):
    """NL points at a nearest-neighbour scale of 0.8 to 3 Angstrom: uniform in a cube of pitch^3 A^3 per atom."""
    side = pitch * NL ** (1.0 / 3.0) + 1.0
    return (torch.rand(NL, 3, generator=g) * side).float()


def armsca_random(NL, B, seed):
    g = _gen("armsca", NL, B, seed)
    pos = torch.cat([_random_cloud(NL, g, PITCHES[b]) for b in range(B)])     # (dense and loose samples: both hinges get winners)
    dec = torch.cat([_decomp_pattern(NL, g) for _ in range(B)])
    return dict(kind="armsca", B=B, NL=NL, pos=pos, decomp=dec, min_d=MIN_D, max_d=MAX_D, random=True)


def _far_filler(n, start=1):
    """n distinct points of the pitch-FAR lattice, away from the origin block that the constructed atoms use (x >= FAR * start)."""
    pts = []
    i = 0
    while len(pts) < n:
        pts.append([FAR * (start + i // 36), FAR * ((i // 6) % 6), FAR * (i % 6)])
        i += 1
    return torch.tensor(pts, dtype=torch.float32)


def armsca_two_wave_winners():
    """NL = 128 (two waves, winners meet in LDS), integer lattice, three arms whose winners are built by hand:
    arm 0: nearest scaffold atom is atom 55 (first wave), d = 1 < min_d;  arm 1: nearest scaffold atom is atom 100 (second
    wave), d = 3 > max_d;  arm 2: atom 45 is exactly 3 away from scaffold atoms 60 (first wave) and 70 (second wave): an exact
    tie across the waves -- squared distances are integers, exact in fp32 and float64.  Every other arm-scaffold pair is at
    least FAR - 3 apart."""
    NL = 128
    dec = torch.tensor([0] * 20 + [1] * 20 + [2] * 10 + [-1] * 78)
    pos = _far_filler(NL)
    pos[5] = pos[55] + torch.tensor([1.0, 0.0, 0.0])
    pos[25] = pos[100] + torch.tensor([0.0, 3.0, 0.0])
    pos[60] = pos[45] + torch.tensor([0.0, 0.0, 3.0])
    pos[70] = pos[45] + torch.tensor([0.0, 0.0, -3.0])
    return dict(kind="armsca", B=1, NL=NL, pos=pos, decomp=dec, min_d=MIN_D, max_d=MAX_D, random=False,
                winners={0: (5, 55), 1: (25, 100), 2: (45, 60)}, tie=(45, 60, 70))


def _small(decomp, pts, min_d, max_d, B=1, **kw):
    pos = torch.tensor(pts, dtype=torch.float32)
    dec = torch.tensor(decomp)
    return dict(kind="armsca", B=B, NL=pos.shape[0] // B, pos=pos, decomp=dec, min_d=min_d, max_d=max_d, random=False, **kw)


def armsca_constructed():
    c = {}
    c["two_wave_winners_nl128"] = armsca_two_wave_winners()
    # finding 2 of the issue, as quoted there: d = 2.0 = max_d exactly -> clamp passes its gradient: [[-1,0,0],[1,0,0]]
    c["hinge_eq_max_quoted"] = _small([0, -1], [[0, 0, 0], [2, 0, 0]], 1.2, 2.0, expect=[[-1, 0, 0], [1, 0, 0]])
    # both hinges at exact equality in one sample: arm 0 at d = 1.0 = min_d (coefficient -1), arm 1 at d = 2.0 = max_d (+1); two arms:
    # each term weighs 1/2.  Scaffold atom 2 at the origin, a far arm-0 / arm-1 atom each so that the winners are not the only atoms.
    c["hinge_eq_both"] = _small([0, 1, -1, 0, 1], [[1, 0, 0], [0, 2, 0], [0, 0, 0], [30, 0, 0], [0, 30, 0]], 1.0, 2.0,
                                expect=[[-.5, 0, 0], [0, .5, 0], [.5, -.5, 0], [0, 0, 0], [0, 0, 0]], eq={0: 1.0, 1: 2.0})
    # min_d == max_d == d = 2: both clamps pass their gradient and the unit coefficients cancel (arm 0); arm 1 at d = 3 stays active
    c["hinge_eq_cancel"] = _small([0, 1, -1], [[2, 0, 0], [0, 0, 3], [0, 0, 0]], 2.0, 2.0,
                                  expect=[[0, 0, 0], [0, 0, .5], [0, 0, -.5]], eq={0: 2.0})
    # finding 1 of the issue as quoted (a scaffold atom on an arm atom: norm has a zero subgradient at 0 -> all zero, finite) ...
    c["coincident_quoted"] = _small([0, -1, -1], [[0, 0, 0], [0, 0, 0], [1, 0, 0]], 1.2, 1.9, expect=[[0, 0, 0]] * 3, zero_d=(0,))
    # ... and next to an active arm, not on the origin: arm 0's winner is the coincident pair (0, 2): nothing; arm 1 (atom 1) is
    # 1.0 from scaffold atom 3: -1/2 along x
    c["coincident_active_arm"] = _small([0, 1, -1, -1, 0], [[1.5, -2.25, 0.75], [4.5, -2.25, 0.75], [1.5, -2.25, 0.75], [5.5, -2.25, 0.75], [1.5, 7, 0]], 1.2, 1.9,
                                        expect=[[0, 0, 0], [.5, 0, 0], [0, 0, 0], [-.5, 0, 0], [0, 0, 0]], zero_d=(0,))
    # one batch: only scaffold atoms | only arm atoms | arm ids {0, 2} (id 1 has no atoms: the mean still runs over 3 arms and the
    # empty one passes no gradient).  Last sample: arm 0 (atom 0) is 1 < min_d from scaffold atom 2, arm 2 (atom 1) 2 > max_d from it;
    # each term weighs 1 / (3 arms * 3 samples).  (Finding 3 of the issue with the last atom at x = 6, not 5: no tie for atom 1.)
    c["invalid_and_gap_b3"] = _small([-1, -1, -1, -1,   0, 1, 0, 1,   0, 2, -1, -1],
                                     [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1],   [0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1],
                                      [0, 0, 0], [3, 0, 0], [1, 0, 0], [6, 0, 0]], 1.2, 1.9, B=3,
                                     expect=[[0, 0, 0]] * 8 + [[1 / 9, 0, 0], [1 / 9, 0, 0], [-2 / 9, 0, 0], [0, 0, 0]], invalid=(0, 1))
    return c


# (NL, B) -> seed chosen by find_seed("armsca", ...): NL 2, 3, 63, 64 one wave; 65, 127, 128 two waves
ARMSCA_SEEDS = {(2, 1): 0, (2, 3): 0, (3, 1): 0, (3, 3): 0, (63, 1): 0, (63, 3): 0, (64, 1): 0, (64, 3): 0,
                (65, 1): 0, (65, 3): 0, (127, 1): 0, (127, 3): 0, (128, 1): 0, (128, 3): 0}


def armsca_winners(case, dtype):
    """Per (sample, arm id with atoms): (arm atom, scaffold atom, d, runner-up d) by the oracle's order -- for every scaffold atom
    the first nearest atom of the arm (scatter_min), then the first scaffold atom at the smallest distance (min over columns).
    The runner-up is the second smallest distance over all (arm atom, scaffold atom) pairs."""
    out = {}
    NL = case["NL"]
    for b in range(case["B"]):
        pos = case["pos"][b * NL:(b + 1) * NL].to(dtype)
        dec = case["decomp"][b * NL:(b + 1) * NL]
        sca = (dec == -1).nonzero()[:, 0]
        if len(sca) == 0:
            continue
        for a in sorted(set(dec[dec >= 0].tolist())):
            arm = (dec == a).nonzero()[:, 0]
            pd = torch.norm(pos[arm].unsqueeze(1) - pos[sca].unsqueeze(0), p=2, dim=-1)
            col_min, col_arg = pd.min(0)
            d = float(col_min.min())
            s = int((col_min == d).nonzero()[0, 0])
            flat = pd.flatten().sort().values
            out[(b, a)] = (int(arm[int(col_arg[s])]), int(sca[s]), d, float(flat[1]) if flat.numel() > 1 else math.inf)
    return out


def armsca_margins(case, dtype=torch.float64):
    """(smallest |hinge argument|, smallest relative lead of a winner) over all arms of the case."""
    h, w = math.inf, math.inf
    for (_, _), (_, _, d, d2) in armsca_winners(case, dtype).items():
        h = min(h, abs(d - case["min_d"]), abs(d - case["max_d"]))
        w = min(w, (d2 - d) / d if d > 0 else math.inf)
    return h, w


def armsca_grad(case, dtype):
    x = case["pos"].to(dtype).clone().requires_grad_(True)
    e, n_valid = OD.armsca_prox_loss(x, _batch_index(case["B"], case["NL"]), case["decomp"], case["min_d"], case["max_d"])
    if n_valid == 0 or not e.requires_grad:
        return torch.zeros_like(x.detach())
    return torch.autograd.grad(e, x)[0]


# ===================================================================================================== clash
def clash_random(NF, NL, B, seed, sigma=2.0, gamma=4.0):
    """Per sample its own protein (NF atoms, about one per 3^3 A^3, around the sample's offset) and its own offset -- the second
    sample's about 100 A out --; every ligand atom 0.5 to 4 A from a random protein atom, so both sides of G < gamma occur."""
    g = _gen("clash", NF, NL, B, seed, sigma, gamma)
    offs = torch.tensor([[3.25, -2.5, 5.125], [97.3, -61.7, 40.9], [-20.1, 11.3, 7.7]])[:B].float()
    prot, pos = [], []
    for b in range(B):
        side = 3.0 * NF ** (1.0 / 3.0)
        p = ((torch.rand(NF, 3, generator=g) - 0.5) * side + offs[b]).float()
        pick = torch.randint(0, NF, (NL,), generator=g)
        u = torch.randn(NL, 3, generator=g)
        r = 0.5 + 3.5 * torch.rand(NL, 1, generator=g)
        y = p[pick] + u / u.norm(dim=1, keepdim=True) * r
        prot.append(p)
        pos.append((y - offs[b]).float())
    return dict(kind="clash", B=B, NL=NL, NF=NF, pos=torch.cat(pos), offset=offs, prot=torch.cat(prot), sigma=sigma, gamma=gamma,
                random=True)


def clash_constructed():
    """One sample (of two: the other is plain) that holds, at NF = 63: atom 0 exactly on protein atom 7 (y == p bit for bit: dyadic
    coordinates), atom 1 at 1 A from protein atom 3 (G < gamma: active), atom 2 at 3.5 A from the nearest protein atom (G > gamma:
    inactive), atom 3 60 A from every protein atom: every exponential underflows, S = 0 exactly, G = -sigma log(1e-3), no gradient."""
    base = clash_random(63, 4, 2, 0)
    NF, NL = 63, 4
    off = torch.tensor([8.0, -16.0, 4.0])
    g = _gen("clash_constructed")
    p = (torch.randint(-40, 41, (NF, 3), generator=g).float() * 0.25 + off)          # quarter-Angstrom lattice in a 20 A cube
    p = torch.unique(p, dim=0)
    while p.shape[0] < NF:                                                          # (duplicates dropped: fill up outside the cube)
        p = torch.cat([p, p[-1:] + torch.tensor([[0.0, 0.0, 12.0]])])
    p = p[:NF]
    y = torch.stack([p[7], p[3] + torch.tensor([0.0, 1.0, 0.0]), p[3], off + torch.tensor([70.0, 0.0, 0.0])])
    # atom 2: the lattice point of the cube's bounding box face + 3.5 A, away from every protein atom
    y[2] = torch.tensor([float(p[:, 0].max()) + 3.5, float(p[p[:, 0].argmax(), 1]), float(p[p[:, 0].argmax(), 2])])
    base["pos"][:NL] = y - off
    base["offset"][0] = off
    base["prot"][:NF] = p
    base.update(random=False, on_atom=(0, 7), underflow=3, constructed_sample=0)
    return base


CLASH_NF, CLASH_NL = (1, 63, 255, 256, 257, 600), (1, 3, 30)
OTHER_SIGMA_GAMMA = (1.5, 3.0)
# (NF, NL, sigma) -> seed chosen by find_seed("clash", ...); B = 2 throughout
CLASH_SEEDS = {(nf, nl, 2.0): 0 for nf in CLASH_NF for nl in CLASH_NL}
CLASH_SEEDS.update({(nf, nl, 1.5): 0 for nf, nl in ((1, 3), (257, 30), (600, 1))})


def clash_G(case, dtype):
    """G per ligand atom [B * NL] and the exponential sums S, as the oracle's clash_loss computes them, in `dtype`."""
    B, NL, NF = case["B"], case["NL"], case["NF"]
    G, S = [], []
    for b in range(B):
        p = case["prot"][b * NF:(b + 1) * NF].to(dtype)
        l = case["pos"][b * NL:(b + 1) * NL].to(dtype) + case["offset"][b].to(dtype)
        e = torch.exp(-torch.sum((p.view(1, -1, 3) - l.view(-1, 1, 3)) ** 2, dim=2) / float(case["sigma"]))
        S.append(e.sum(dim=1))
        G.append(-case["sigma"] * torch.log(1e-3 + e.sum(dim=1)))
    return torch.cat(G), torch.cat(S)


def clash_margin(case, dtype=torch.float64):
    G, _ = clash_G(case, dtype)
    return float((case["gamma"] - G).abs().min())


def clash_grad(case, dtype):
    B, NL, NF = case["B"], case["NL"], case["NF"]
    x = case["pos"].to(dtype).clone().requires_grad_(True)
    bl = _batch_index(B, NL)
    e = OD.clash_loss(case["prot"].to(dtype), x + case["offset"].to(dtype)[bl], _batch_index(B, NF), bl, case["sigma"], case["gamma"])
    if not e.requires_grad:
        return torch.zeros_like(x.detach())
    return torch.autograd.grad(e, x)[0]


# ================================================================================================ arms_repul
REPUL_MAX_D = 2.2


def repul_random(NL, B, seed, mode):
    g = _gen("repul", NL, B, seed)
    pos = torch.cat([_random_cloud(NL, g) for _ in range(B)])
    dec = torch.cat([_decomp_pattern(NL, g) if NL > 2 else torch.tensor([0, 1]) for _ in range(B)])
    return dict(kind="repul", B=B, NL=NL, pos=pos, decomp=dec, max_d=REPUL_MAX_D, mode=mode, random=True)


def repul_constructed(mode):
    """B = 3, NL = 10, max_d = 2 (dyadic coordinates: the quoted distances are exact in fp32 and float64).
    sample 0: arm ids {0, 2, 3} (gap at 1); arms 2 and 3 have one atom each; atoms 0 and 1 of arm 0 coincide (within one arm); atom 2
              (arm 0) and atom 6 (arm 2) coincide (across two arms: that arm pair's minimum is a single zero); atom 7 (arm 3) is exactly
              2.0 = max_d from atom 3 (arm 0) -- in mode 'all' the inclusive hinge gives that pair a gradient of +-1 / (n1 n2 B);
    sample 1: no arms at all (only scaffold atoms): zero gradient;
    sample 2: generic two-arm geometry with one-atom arm 1."""
    s0 = [[0.5, 0.25, 0.0], [0.5, 0.25, 0.0], [3.5, 0.75, 1.25], [0.5, 6.25, 0.5], [-4.0, 1.5, 2.25],
          [9.0, 9.0, 9.0], [3.5, 0.75, 1.25], [2.5, 6.25, 0.5], [12.0, -3.0, 1.0], [7.5, -6.0, 2.0]]
    d0 = [0, 0, 0, 0, 0, -1, 2, 3, -1, -1]
    s1 = [[float(i), 0.5 * i, 0.25 * i * i] for i in range(10)]
    d1 = [-1] * 10
    g = _gen("repul_constructed")
    s2 = (torch.rand(10, 3, generator=g) * 3.0).tolist()
    d2 = [0, 0, 0, 0, 1, -1, -1, 0, 0, -1]
    return dict(kind="repul", B=3, NL=10, pos=torch.tensor(s0 + s1 + s2, dtype=torch.float32), decomp=torch.tensor(d0 + d1 + d2),
                max_d=2.0, mode=mode, random=False, eq_pair=(3, 7), coincident=((0, 1), (2, 6)), no_arm_sample=1)


REPUL_NL = (2, 64, 65, 128)
# (NL, mode) -> seed chosen by find_seed("repul", ...); B = 2
REPUL_SEEDS = {(nl, m): 0 for nl in REPUL_NL for m in ("min", "all")}


def repul_pairs(case, dtype):
    """mode 'all': every distance between two arm atoms p != q of one sample.  mode 'min': per (sample, a1 < a2) the smallest and the
    second smallest cross distance and the winning pair -> (all distances [n], {(b, a1, a2): (p, q, d, runner-up)})."""
    NL = case["NL"]
    alld, mins = [], {}
    for b in range(case["B"]):
        pos = case["pos"][b * NL:(b + 1) * NL].to(dtype)
        dec = case["decomp"][b * NL:(b + 1) * NL]
        arms = sorted(set(dec[dec >= 0].tolist()))
        idx = (dec >= 0).nonzero()[:, 0]
        if len(idx) > 1:
            pd = torch.norm(pos[idx].unsqueeze(1) - pos[idx].unsqueeze(0), p=2, dim=-1)
            alld.append(pd[~torch.eye(len(idx), dtype=torch.bool)])
        for i, a1 in enumerate(arms):
            for a2 in arms[i + 1:]:
                p1, p2 = (dec == a1).nonzero()[:, 0], (dec == a2).nonzero()[:, 0]
                pd = torch.norm(pos[p1].unsqueeze(1) - pos[p2].unsqueeze(0), p=2, dim=-1)
                flat = pd.flatten()
                k = int(flat.argmin())
                srt = flat.sort().values
                mins[(b, a1, a2)] = (int(p1[k // len(p2)]), int(p2[k % len(p2)]), float(srt[0]), float(srt[1]) if len(srt) > 1 else math.inf)
    return (torch.cat(alld) if alld else torch.zeros(0, dtype=dtype)), mins


def repul_margins(case, dtype=torch.float64):
    alld, mins = repul_pairs(case, dtype)
    if case["mode"] == "all":
        return (float((alld - case["max_d"]).abs().min()) if alld.numel() else math.inf), math.inf
    h = min((abs(d - case["max_d"]) for _, _, d, _ in mins.values()), default=math.inf)
    w = min(((d2 - d) / d if d > 0 else math.inf for _, _, d, d2 in mins.values()), default=math.inf)
    return h, w


def repul_grad(case, dtype):
    x = case["pos"].to(dtype).clone().requires_grad_(True)
    e, n_valid = OD.arms_repul_loss(x, _batch_index(case["B"], case["NL"]), case["decomp"], case["max_d"], case["mode"])
    if n_valid == 0 or not e.requires_grad:
        return torch.zeros_like(x.detach())
    return torch.autograd.grad(e, x)[0]


# ================================================================================================ all cases
GRAD = {"armsca": armsca_grad, "clash": clash_grad, "repul": repul_grad}
MARGINS = {"armsca": armsca_margins, "clash": lambda c, dtype=torch.float64: (clash_margin(c, dtype), math.inf), "repul": repul_margins}


def same_branches(case):
    """Does the fp32 oracle take the winners and hinge branches of the float64 one?"""
    if case["kind"] == "armsca":
        w64, w32 = armsca_winners(case, torch.float64), armsca_winners(case, torch.float32)
        side = lambda d: (d < case["min_d"], d > case["max_d"])
        return all(w64[k][:2] == w32[k][:2] and side(w64[k][2]) == side(w32[k][2]) for k in w64)
    if case["kind"] == "clash":
        return bool(torch.equal(clash_G(case, torch.float64)[0] < case["gamma"], clash_G(case, torch.float32)[0] < case["gamma"]))
    a64, m64 = repul_pairs(case, torch.float64)
    a32, m32 = repul_pairs(case, torch.float32)
    if case["mode"] == "all":
        return bool(torch.equal(a64 <= case["max_d"], a32 <= case["max_d"]))
    return all(m64[k][:2] == m32[k][:2] and (m64[k][2] <= case["max_d"]) == (m32[k][2] <= case["max_d"]) for k in m64)


def seed_ok(case):
    h, w = MARGINS[case["kind"]](case)
    return h >= HINGE_MARGIN and w >= WINNER_MARGIN and same_branches(case)


def find_seed(build, limit=200):
    """The first seed at which the float64 oracle has the margins of the module docstring and the fp32 oracle agrees on winners and
    branches (how the seed tables above were filled; not used when the tests run)."""
    for seed in range(limit):
        if seed_ok(build(seed)):
            return seed
    raise RuntimeError("no seed with the required margins")


def _build_all():
    c = {}
    for (NL, B), seed in ARMSCA_SEEDS.items():
        c[f"armsca/random_nl{NL}_b{B}"] = armsca_random(NL, B, seed)
    for name, case in armsca_constructed().items():
        c[f"armsca/{name}"] = case
    for (NF, NL, sigma), seed in CLASH_SEEDS.items():
        gamma = 4.0 if sigma == 2.0 else OTHER_SIGMA_GAMMA[1]
        c[f"clash/random_nf{NF}_nl{NL}_s{sigma:g}"] = clash_random(NF, NL, 2, seed, sigma, gamma)
    c["clash/constructed_nf63"] = clash_constructed()
    for (NL, mode), seed in REPUL_SEEDS.items():
        c[f"repul_{mode}/random_nl{NL}"] = repul_random(NL, 2, seed, mode)
    for mode in ("min", "all"):
        c[f"repul_{mode}/constructed"] = repul_constructed(mode)
    return c


@functools.lru_cache(maxsize=None)
def all_cases():
    return _build_all()


NAMES = tuple(_build_all())


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float64 gradient, fp32 gradient, d32, bound) of a case: computed once, shared, never modified."""
    case = all_cases()[name]
    g64 = GRAD[case["kind"]](case, torch.float64)
    g32 = GRAD[case["kind"]](case, torch.float32)
    assert g64.dtype == torch.float64 and g32.dtype == torch.float32
    d32 = float((g64 - g32.double()).abs().max())
    return g64, g32, d32, bound(case["kind"], d32)


def known_buffer(name, shape):
    """The known random buffer that the accumulate = 1 run adds onto."""
    return torch.randn(shape, generator=_gen("buffer", name)).float()


def report(name, err, d32, bnd, extra=""):
    """One machine-readable line per case, printed before any assert (as stress_cases.report)."""
    print(f"\nDRIFT {name} err={err:.3g} d32={d32:.3g} bound={bnd:.3g}{extra}")


# ============================================================================================ sampler-level case
SAMPLER_SEED = 1                    # chosen like the seed tables above (sampler_margins)


def sampler_batch(seed=SAMPLER_SEED):
    """The 40 + 12 atom, B = 2 batch of stress_weights.lattice_batch with the lattice points jittered by up to 0.3 A (generic
    distances: no ties, no hinge at equality) and, in sample 0, scaffold atom 8 exactly on arm atom 0: arm 0's nearest scaffold
    atom is at distance 0, where the armsca energy has a zero subgradient."""
    import stress_weights as SW
    b = dict(SW.lattice_batch())
    g = _gen("sampler", seed)
    pos = b["init_ligand_pos"].clone()
    pos[1] = pos[0] + torch.tensor([0.0, 0.0, 1.0])             # (lattice_batch puts atom 1 on atom 0: undone, one coincidence is the subject)
    pos[13] = pos[12] + torch.tensor([0.0, 0.0, 1.0])
    pos = pos + (torch.rand(pos.shape, generator=g) - 0.5) * 0.6
    pos[8] = pos[0]
    b["init_ligand_pos"] = pos.float().contiguous()
    return b


def sampler_margins(b):
    """(armsca hinge margin, armsca winner margin, clash hinge margin) of the centred start positions in float64, and whether the fp32
    oracle takes the same branches."""
    from oracle import ops as OO
    B = int(b["batch_ligand"].max()) + 1
    NL, NF = b["init_ligand_pos"].shape[0] // B, b["full_protein_pos"].shape[0] // B
    off = OO.scatter_mean(b["protein_pos"], b["batch_protein"], dim=0)
    xt = b["init_ligand_pos"] - off[b["batch_ligand"]]
    a = dict(kind="armsca", B=B, NL=NL, pos=xt, decomp=b["ligand_decomp_index"], min_d=MIN_D, max_d=MAX_D)
    c = dict(kind="clash", B=B, NL=NL, NF=NF, pos=xt, offset=off, prot=b["full_protein_pos"], sigma=2.0, gamma=4.0)
    h, w = armsca_margins(a)
    return h, w, clash_margin(c), same_branches(a) and same_branches(c), a
