"""Deterministic cases for the general distance-restraint kernel (k_drift_restraint<true> in csrc/dd_step.hip, dd_drift_restraint2): typed
endpoints, ligand-ligand pairs, the harmonic hinge.  The energy of include/decompdiff_hip.h ("the general form") restated in torch,
its gradient under autograd in float64 (the yardstick) and in fp32; the method, the flat tolerance, the margins and the seed search
are those of tests/restraint_cases.py.  A plain helper module (no tests): tests/test_restraint2_cases_host.py checks that every case
is what it says it is, tests/test_gpu_restraint2.py runs the kernel.

    set(endpoint) = the explicit atom, or the real atoms of the group, kept where the atom's CURRENT class v is in the class mask
                    (a NULL mask array: untyped; a class outside [0, 32) is in no mask)
    point:  d_r = | x_w - p_r |,  w the FIRST nearest member of set 1 in row order
    pair:   d_r = | x_i - x_j |,  (i, j) the FIRST nearest pair in (i, then j) order, i in set 1, j in set 2, i != j
    E = sum_r w_r (relu(min_d_r - d_r)^k + relu(d_r - max_d_r)^k),  k = 1 (linear) or 2 (harmonic)

Bounds: restraint_cases.bound with FLAT times the case's largest gradient coefficient -- w of a linear restraint, 2 w |excess| (float64
oracle) of a harmonic one --, or twice the fp32 oracle's own distance where that is further than a quarter of it from float64.
Random geometries are kept only at seeds where the float64 oracle alone has every winner (or winning pair) WINNER_MARGIN ahead of the
runner-up and every LINEAR hinge argument HINGE_MARGIN from zero (a harmonic hinge has a continuous gradient: no margin).  The
mirror (j, i) of a winning pair that lies in both sets ties with it EXACTLY (the differences negate, the squares are the same bits):
(i, j) with i < j comes first, and the runner-up is the nearest pair other than these two.  Nothing is filtered when the kernel runs.

A sample of at most 3 atoms collects all of its restraints' gradients on its few rows; as in restraint_cases nine in ten of such a
sample's restraints are free (min_d = 0, max_d = inf): they still run through the search and report dist / winners."""
import functools
import math

import torch

import drift_cases as DC
import restraint_cases as RC
from restraint_cases import ABSENT_ARM, ANY, FLAT, HINGE_MARGIN, INF, SCA, WINNER_MARGIN, bound, dist_bound  # noqa: F401

NONE = -4                            # DD_RESTRAINT_NONE: group2 of a row without a second endpoint
ALL = 0xFFFFFFFF
NUM_CLASSES = 8                      # the classes the random cases draw from (the smallest vocabulary)


def mask_of(ids):
    return ALL if ids is None else sum(1 << i for i in ids)


def _case(B, NL, pos, decomp, v, rs, nl_real=None, typed=True, **kw):
    """rs: list of dicts(sample, min_d, max_d, weight, and any of point, atom, group, cls, atom2, group2, cls2, form), any order;
    stored sorted by sample (stable) with the CSR ptr.  cls / cls2: class ids or None (every class); atom / atom2: rows within the
    sample; a restraint is a pair iff it gives atom2 or group2.  typed=False: the case hands no class masks over at all."""
    rs = sorted(rs, key=lambda r: r["sample"])
    f32 = lambda v_: torch.tensor(v_, dtype=torch.float32)
    i64 = lambda key, default: torch.tensor([r.get(key, default) for r in rs], dtype=torch.long)
    sample = i64("sample", 0)
    pair = torch.tensor([("atom2" in r) or ("group2" in r) for r in rs], dtype=torch.bool)
    c = dict(B=B, NL=NL, pos=pos.float().contiguous(), decomp=None if decomp is None else decomp.long(), v=None if v is None else v.long(),
             nl_real=nl_real, R=len(rs), sample=sample,
             point=f32([list(map(float, r.get("point", (0.0, 0.0, 0.0)))) for r in rs]).reshape(-1, 3),
             min_d=f32([r["min_d"] for r in rs]), max_d=f32([r["max_d"] for r in rs]), weight=f32([r["weight"] for r in rs]),
             atom=i64("atom", -1), group=i64("group", ANY), atom2=i64("atom2", -1), pair=pair,
             group2=torch.tensor([r.get("group2", ANY if "atom2" in r else NONE) for r in rs], dtype=torch.long),
             form=torch.tensor([1 if r.get("form", "linear") == "harmonic" else 0 for r in rs], dtype=torch.long),
             cls=torch.tensor([mask_of(r.get("cls")) for r in rs], dtype=torch.long) if typed else None,
             cls2=torch.tensor([mask_of(r.get("cls2")) for r in rs], dtype=torch.long) if typed else None, random=False)
    c["ptr"] = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(torch.bincount(sample, minlength=B), 0)])
    c.update(kw)
    return c


def members(case, r, end=1):
    """Rows (within the sample) of endpoint `end` of restraint r, in row order."""
    b, NL = int(case["sample"][r]), case["NL"]
    n = NL if case["nl_real"] is None else int(case["nl_real"][b])
    sfx = "2" if end == 2 else ""
    at, gp = int(case["atom" + sfx][r]), int(case["group" + sfx][r])
    cl = None if case["cls" + sfx] is None else int(case["cls" + sfx][r])
    if at >= 0:
        rows = [at] if at < n else []
    elif gp == ANY:
        rows = list(range(n))
    elif case["decomp"] is None or gp < -1:
        rows = []
    else:
        rows = (case["decomp"][b * NL:b * NL + n] == gp).nonzero()[:, 0].tolist()
    if cl is not None:
        v = case["v"][b * NL:(b + 1) * NL]
        rows = [i for i in rows if 0 <= int(v[i]) < 32 and (cl >> int(v[i])) & 1]
    return rows


def _first_min(d):
    """Index of the first minimum of the 1-d tensor d."""
    return int((d == d.min()).nonzero()[0, 0])


def energy(case, x):
    """E of the module docstring at positions x [B*NL,3] (any dtype) -> (E, dist [R], winner [R], winner2 [R], runner-up distance [R])."""
    dt = x.dtype
    E = torch.zeros((), dtype=dt)
    dist, win, win2, second = [], [], [], []
    for r in range(case["R"]):
        b = int(case["sample"][r])
        base = b * case["NL"]
        s1 = members(case, r, 1)
        if not bool(case["pair"][r]):
            if not s1:
                dist.append(INF), win.append(-1), win2.append(-1), second.append(INF)
                continue
            d = torch.norm(x[torch.tensor(s1) + base] - case["point"][r].to(dt), p=2, dim=-1)
            k = _first_min(d.detach())
            dw = d[k]
            srt = d.detach().sort().values
            win.append(s1[k]), win2.append(-1), second.append(float(srt[1]) if len(s1) > 1 else INF)
        else:
            s2 = members(case, r, 2)
            pairs = [(i, j) for i in s1 for j in s2 if i != j]                      # (i, then j) order
            if not pairs:
                dist.append(INF), win.append(-1), win2.append(-1), second.append(INF)
                continue
            ii, jj = torch.tensor([p[0] for p in pairs]) + base, torch.tensor([p[1] for p in pairs]) + base
            d = torch.norm(x[ii] - x[jj], p=2, dim=-1)
            k = _first_min(d.detach())
            dw = d[k]
            others = [dq for dq, p in zip(d.detach().tolist(), pairs) if p != pairs[k] and p != (pairs[k][1], pairs[k][0])]
            win.append(pairs[k][0]), win2.append(pairs[k][1]), second.append(min(others) if others else INF)
        lo = torch.clamp(case["min_d"][r].to(dt) - dw, min=0)
        hi = torch.clamp(dw - case["max_d"][r].to(dt), min=0)
        E = E + case["weight"][r].to(dt) * ((lo * lo + hi * hi) if int(case["form"][r]) else (lo + hi))
        dist.append(float(dw.detach()))
    return E, dist, win, win2, second


def grad(case, dtype):
    x = case["pos"].to(dtype).clone().requires_grad_(True)
    E, dist, win, win2, second = energy(case, x)
    g = torch.autograd.grad(E, x)[0] if E.requires_grad else torch.zeros_like(x.detach())
    return g, dist, win, win2, second


def coefficients(case, dist):
    """|c| of every restraint at the distances `dist`: w (linear, where a hinge is active or not: the size a rounding error scales
    with) or 2 w |excess| (harmonic); 0 without a winner."""
    out = []
    for r, d in enumerate(dist):
        w, mn, mx = float(case["weight"][r]), float(case["min_d"][r]), float(case["max_d"][r])
        if not math.isfinite(d):
            out.append(0.0)
        elif int(case["form"][r]):
            out.append(2.0 * w * max(mn - d, d - mx, 0.0))
        else:
            out.append(w)
    return out


def margins(case, dtype=torch.float64):
    """(smallest |hinge argument| over the finite bounds of LINEAR restraints with a winner, smallest relative lead of a winner)."""
    _, dist, win, _, second = grad(case, dtype)
    h, w = INF, INF
    for r in range(case["R"]):
        if win[r] < 0:
            continue
        if not int(case["form"][r]):
            for bnd in (float(case["min_d"][r]), float(case["max_d"][r])):
                if math.isfinite(bnd):
                    h = min(h, abs(dist[r] - bnd))
        if dist[r] > 0:
            w = min(w, (second[r] - dist[r]) / dist[r])
    return h, w


def same_branches(case):
    """Does the fp32 oracle take the winners and hinge branches of the float64 one?"""
    _, d64, w64, v64, _ = grad(case, torch.float64)
    _, d32, w32, v32, _ = grad(case, torch.float32)
    return w64 == w32 and v64 == v32 and RC.sides(case, d64) == RC.sides(case, d32)


def seed_ok(case):
    h, w = margins(case)
    if not (h >= HINGE_MARGIN and w >= WINNER_MARGIN and same_branches(case)):
        return False
    try:                                                                            # (the fp32 oracle must be able to judge the case)
        _reference(case)
    except AssertionError:
        return False
    return True


def find_seed(build, limit=200):
    """restraint_cases.find_seed with this module's seed_ok (how RANDOM_SEEDS was filled; not used when the tests run)."""
    for seed in range(limit):
        if seed_ok(build(seed)):
            return seed
    raise RuntimeError("no seed with the required margins")


# ============================================================================================== random cases
COUNTS = RC.COUNTS                   # restraints per sample: more than a wave, none, one
KINDS = ("typed_any", "pair_atoms", "pair_typed_any", "pair_arm_sca", "typed_atom", "pair_atom_any", "pair_absent")


def random_case(NL, B, seed, padded=False):
    """B samples of NL atoms (restraint_cases' clouds and arm patterns, classes uniform in [0, NUM_CLASSES)); sample b carries
    COUNTS[B][b] restraints that cycle through KINDS: typed point restraints on a group or an explicit atom (which may have the
    wrong class: empty), pairs of explicit atoms, of typed groups, of an arm and the scaffold, of an atom and a typed group, of an
    absent arm; forms alternate.  Windows as restraint_cases.random_case.  padded: real sizes below NL, the second sample's is 2."""
    g = DC._gen("restraint2", NL, B, seed, padded)
    pos = torch.cat([DC._random_cloud(NL, g, DC.PITCHES[b % 3]) for b in range(B)])
    dec = torch.cat([RC._decomp(NL, g) for _ in range(B)])
    v = torch.randint(0, NUM_CLASSES, (B * NL,), generator=g)
    nl_real = None
    if padded:
        nl_real = [int(torch.randint(max(2, NL // 2), NL, (1,), generator=g)) for _ in range(B)]
        nl_real[1 % B] = 2
    rnd = lambda: float(torch.rand(1, generator=g))
    pick = lambda n: int(torch.randint(0, n, (1,), generator=g))
    rs, i = [], 0
    for b in range(B):
        n = NL if nl_real is None else nl_real[b]
        real = dec[b * NL:b * NL + n]
        arms = sorted(set(real[real >= 0].tolist()))
        for _ in range(COUNTS[B][b]):
            kind = KINDS[i % len(KINDS)]
            near = pick(NL if padded else n)
            u = torch.randn(3, generator=g)
            p = pos[b * NL + near] + u / u.norm() * (0.8 + 3.2 * rnd())
            mn = 0.0 if i % 9 == 8 else 0.5 + 2.5 * rnd()
            mx = INF if i % 11 == 6 else mn + 0.3 + 1.2 * rnd()
            if min(n, NL) <= 3 and i % 10 != 0:
                mn, mx = 0.0, INF
            r = dict(sample=b, point=p.float().tolist(), min_d=mn, max_d=mx, weight=0.25 + 1.75 * rnd(), form=("linear", "harmonic")[(i // 2) % 2])
            three = lambda: sorted(set(pick(NUM_CLASSES) for _ in range(3)))
            if kind == "typed_any":
                r.update(cls=three())
            elif kind == "pair_atoms":
                a = pick(n)
                r.update(atom=a, atom2=(a + 1 + pick(n - 1)) % n)
            elif kind == "pair_typed_any":
                r.update(cls=three(), group2=ANY, cls2=three())
            elif kind == "pair_arm_sca":
                r.update(group=arms[i % len(arms)] if arms else ABSENT_ARM, group2=SCA)
            elif kind == "typed_atom":
                a = pick(n)
                r.update(atom=a, cls=sorted({int(v[b * NL + a]), pick(NUM_CLASSES)}) if i % 2 else three())
            elif kind == "pair_atom_any":
                r.update(atom=pick(n), group2=ANY, cls2=three())
            else:
                r.update(group=ABSENT_ARM, group2=ANY)
            rs.append(r)
            i += 1
    return _case(B, NL, pos, dec, v, rs, nl_real=nl_real, random=True)


SIZES = (2, 3, 63, 64, 65, 128)
# (NL, B, padded) -> seed chosen by find_seed(lambda s: random_case(NL, B, s, padded))
RANDOM_SEEDS = {(2, 1, False): 0, (2, 3, False): 0, (3, 1, False): 0, (3, 3, False): 0, (63, 1, False): 0, (63, 3, False): 0,
                (64, 1, False): 0, (64, 3, False): 0, (65, 1, False): 0, (65, 3, False): 0, (128, 1, False): 0, (128, 3, False): 0,
                (64, 3, True): 0, (128, 3, True): 0}


# ========================================================================================= constructed cases
def constructed():
    c = {}
    L = RC._lattice
    # exact ties between two pairs on the integer lattice: rows (5, 9) and (7, 20) are both 3 apart, everything else is far: ANY-ANY
    # has the candidates (5,9), (7,20), (9,5), (20,7) at the same distance -> (5, 9).  d = 3 > max_d = 2, linear: +w u on 5, -w u on 9
    c["pair_tie_in_wave_nl64"] = _case(
        1, 64, L(64, {5: [0, 0, 3], 9: [0, 0, 0], 7: [0, 50, 0], 20: [0, 53, 0]}), None, None,
        [dict(sample=0, min_d=1.0, max_d=2.0, weight=1.5, group2=ANY)], typed=False, winners=[(5, 9)],
        expect_rows={5: [0, 0, 1.5], 9: [0, 0, -1.5]})
    # two waves: (40, 100) and (10, 110) tie at 3 -> (10, 110), whose ends lie in different waves; a second restraint between explicit
    # atoms of the two waves' edge lanes (63, 64), harmonic, d = 4, max_d = 2.5: c = 2 * 0.5 * 1.5 = 1.5; a third, (100 -> ANY) from
    # the second wave back into the first: nearest of 100 is 40
    c["pair_tie_across_waves_nl128"] = _case(
        1, 128, L(128, {40: [0, 3, 0], 100: [0, 0, 0], 10: [0, -50, 3], 110: [0, -50, 0], 63: [-90, 0, 4], 64: [-90, 0, 0]}), None, None,
        [dict(sample=0, min_d=1.0, max_d=2.0, weight=1.0, group2=ANY),
         dict(sample=0, min_d=1.0, max_d=2.5, weight=0.5, atom=63, atom2=64, form="harmonic"),
         dict(sample=0, min_d=4.0, max_d=9.0, weight=2.0, atom=100, group2=ANY)], typed=False,
        winners=[(10, 110), (63, 64), (100, 40)],
        expect_rows={10: [0, 0, 1], 110: [0, 0, -1], 63: [0, 0, 1.5], 64: [0, 0, -1.5], 100: [0, 2, 0], 40: [0, -2, 0]})
    # values of the two forms between explicit atoms 2 apart along x (rows 2k, 2k + 1), and a coincident pair (rows 12, 13: d == 0):
    #   linear d == min_d: -w; linear min_d == max_d == d: the two cancel; harmonic min_d == max_d == d: 0; harmonic d = 2 < min_d = 3.5:
    #   c = -2 * 1 * 1.5 = -3; harmonic inside: 0; d == 0 below min_d, both forms: nothing, finite, winners reported
    pos = L(14, {})
    for k in range(6):
        pos[2 * k] = torch.tensor([100.0 * k + 2.0, 0, 0])
        pos[2 * k + 1] = torch.tensor([100.0 * k, 0, 0])
    pos[12] = pos[13] = torch.tensor([700.0, 0, 0])
    pr = lambda k, mn, mx, w, form: dict(sample=0, min_d=mn, max_d=mx, weight=w, atom=2 * k, atom2=2 * k + 1, form=form)
    c["pair_hinge_values"] = _case(
        1, 14, pos, None, None,
        [pr(0, 2.0, 5.0, 1.0, "linear"), pr(1, 2.0, 2.0, 1.0, "linear"), pr(2, 2.0, 2.0, 1.0, "harmonic"), pr(3, 3.5, INF, 1.0, "harmonic"),
         pr(4, 1.0, 3.0, 1.0, "harmonic"), pr(6, 1.0, 3.0, 1.0, "linear"), pr(6, 1.0, 3.0, 1.0, "harmonic"), pr(5, 0.0, 0.5, 0.25, "harmonic")],
        typed=False, zero_d=(5, 6), winners=[(0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (12, 13), (12, 13), (10, 11)],
        expect_rows={0: [-1, 0, 0], 1: [1, 0, 0], 6: [-3, 0, 0], 7: [3, 0, 0], 10: [.75, 0, 0], 11: [-.75, 0, 0]})
    # sets and classes, B = 3 with nothing on sample 1, NL = 6: decomp = [0, 2, -1, 5, -1, 2], classes = [1, 1, 3, 40, 3, -5] (rows 3 and
    # 5 carry class ids no mask can hold); rows sit 10 apart along x, points 1 below their intended winners, min_d = 2: -w z
    dec = torch.tensor([0, 2, -1, 5, -1, 2] * 3)
    v = torch.tensor([1, 1, 3, 40, 3, -5] * 3)
    rows = [[0, 0, 0], [10, 0, 0], [20, 0, 0], [30, 0, 0], [40, 0, 0], [50, 0, 0]]
    pos = torch.tensor(rows * 3, dtype=torch.float32)
    below = lambda row: [rows[row][0], 0, -1]
    pt = lambda s, row, **kw: dict(sample=s, point=below(row), min_d=2.0, max_d=9.0, weight=1.0, **kw)
    pp = lambda s, **kw: dict(sample=s, min_d=12.0, max_d=99.0, weight=1.0, **kw)
    sets = [pt(0, 3, cls=None),                                  # every class: row 3 (class 40) is in no mask -> nearest other: rows 2, 4 tie -> 2
            pt(0, 3, atom=3, cls=[1, 3]),                        # the explicit atom's class is out of range: empty
            pt(0, 1, cls=[3]),                                   # class 3: rows 2, 4 -> row 2 (d = sqrt(101) > 9: +w u)
            pt(0, 1, atom=1, cls=[3]),                           # an explicit atom of the wrong class: empty
            pt(0, 1, atom=1, cls=[1]),                           # ... of the right class -> row 1
            pt(0, 0, cls=[7]),                                   # a class no atom has: empty
            pt(0, 5, group=2, cls=[1]),                          # arm 2 = rows 1, 5; row 5's class is -5 -> row 1
            pp(0, atom=2, atom2=2),                              # set 1 == set 2 == one atom: empty
            pp(0, group=0, group2=0),                            # ... as groups (arm 0 = row 0 alone): empty
            pp(0, group=SCA, group2=SCA, cls=[3], cls2=[3]),     # scaffold x scaffold, class 3: (2, 4), d = 20 inside: nothing
            pp(0, group=ANY, group2=2, cls=[3], cls2=None),      # class 3 x arm 2 (row 5 out): (2, 1), d = 10 < 12: -w u on 2, +w u on 1
            pp(0, group=5, group2=ANY),                          # arm 5 = row 3 (out of range class) x ANY: empty
            pp(0, group=1, group2=ANY),                          # arm 1: the gap, nobody
            pp(2, group=ANY, group2=SCA, cls=[1], cls2=[3], form="harmonic")]   # sample 2: (1, 2), d = 10 < 12: c = -4
    c["sets_and_classes_b3"] = _case(3, 6, pos, dec, v, sets, empty_sample=1,
                                     winners=[(2, -1), (-1, -1), (2, -1), (-1, -1), (1, -1), (-1, -1), (1, -1), (-1, -1), (-1, -1), (2, 4),
                                              (2, 1), (-1, -1), (-1, -1), (1, 2)])
    # without decomp_index (arm / scaffold groups are then refused at the boundary): the ANY and explicit-atom restraints of the same list
    free = lambda s: s["sample"] == 0 and s.get("group", ANY) == ANY and s.get("group2", ANY) == ANY
    c["sets_no_decomp"] = _case(1, 6, pos[:6], None, v[:6], [s for s in sets if free(s)] + [pp(0, group=ANY, group2=ANY, cls=[3], cls2=[1])],
                                winners=[(2, -1), (-1, -1), (2, -1), (-1, -1), (1, -1), (-1, -1), (-1, -1), (2, 1)])
    # one atom that wins several restraints as i and as j: row 0 against rows 1 .. 4 in alternating roles, oblique directions, both forms
    g = DC._gen("restraint2", "order")
    pos = (torch.rand(5, 3, generator=g) * 4.0).float()
    many = [dict(sample=0, min_d=0.5, max_d=1.0 + 0.1 * k, weight=0.5 + 0.25 * k, form=("linear", "harmonic")[k % 2],
                 **(dict(atom=0, atom2=1 + k % 4) if k % 2 == 0 else dict(atom=1 + k % 4, atom2=0))) for k in range(8)]
    c["one_atom_many_roles"] = _case(1, 5, pos, None, None, many, typed=False)
    # padded batch: sample 0 has 5 real atoms of 8 and its padding rows 5 .. 7 sit between the real ones; sample 1 has 2 real atoms
    pos = L(16, {0: [0, 0, 0], 4: [0, 0, 3], 6: [0, 0, 1], 7: [0, 0, 2], 8: [500, 0, 0], 8 + 1: [500, 0, 2], 8 + 2: [500, 0, 1]})
    dec = torch.tensor([0, 0, -1, -1, 0, 0, 0, -1] + [-1, 0, 0, -2, -2, -2, -2, -2])
    v = torch.tensor([2] * 16)
    c["padded_pair_skips_padding"] = _case(
        2, 8, pos, dec, v,
        [dict(sample=0, min_d=4.0, max_d=9.0, weight=1.0, atom=0, group2=ANY), dict(sample=0, min_d=4.0, max_d=9.0, weight=1.0, atom=0, atom2=6),
         dict(sample=0, min_d=4.0, max_d=9.0, weight=1.0, group=0, group2=0, cls=[2], cls2=[2]),
         dict(sample=1, min_d=0.0, max_d=0.5, weight=1.0, group2=ANY, form="harmonic"), dict(sample=1, min_d=0.0, max_d=0.5, weight=1.0, group=0, group2=0)],
        nl_real=[5, 2], winners=[(0, 4), (-1, -1), (0, 4), (0, 1), (-1, -1)],
        expect_rows={0: [0, 0, 2], 4: [0, 0, -2], 8: [0, 0, -3], 8 + 1: [0, 0, 3]})
    return c


def old_form_case(NL):
    """A point / linear / untyped case (restraint_cases' random case of that size), for the bit comparison of the two kernels."""
    return RC.all_cases()[f"random_nl{NL}_b3"]


def _build_all():
    c = {}
    for (NL, B, padded), seed in RANDOM_SEEDS.items():
        c[f"random_nl{NL}_b{B}" + ("_padded" if padded else "")] = random_case(NL, B, seed, padded)
    c.update(constructed())
    return c


def _reference(case):
    g64, dist, win, win2, _ = grad(case, torch.float64)
    g32, dist32, _, _, _ = grad(case, torch.float32)
    assert g64.dtype == torch.float64 and g32.dtype == torch.float32
    d32 = float((g64 - g32.double()).abs().max())
    cmax = max(coefficients(case, dist), default=1.0) if case["R"] else 1.0
    return dict(g64=g64, g32=g32, d32=d32, cmax=cmax, bound=bound(d32, cmax), dist=torch.tensor(dist, dtype=torch.float64),
                dist32=torch.tensor(dist32, dtype=torch.float64), winner=torch.tensor(win, dtype=torch.long),
                winner2=torch.tensor(win2, dtype=torch.long))


@functools.lru_cache(maxsize=None)
def all_cases():
    return _build_all()


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(g64, g32, d32, cmax, bound, dist [R] float64, dist32 [R], winner [R], winner2 [R]) of a case: computed once, shared, never
    modified."""
    return _reference(all_cases()[name])


# ============================================================================================ sampler-level cases
SAMPLER_SEED = 0                     # chosen like the seed table (host test: margins of sampler_case)


def batch_entry(b, seed, per_sample=(4, 4), weight=(0.5, 1.5), **opts):
    """A general ``restraint`` entry of energy_drift_opt for the sampling batch `b` (dense or ragged): sample k carries per_sample[k]
    restraints that cycle through: a harmonic pair of two explicit atoms asked to close to 0.8 .. 1.2 A; a linear point restraint on
    the nearest atom of three classes; a harmonic pair arm 0 x scaffold with the scaffold end typed, asked apart (min_d = 6); a linear
    pair ANY x ANY asked apart (min_d = 3).  Listed sample-interleaved: the caller's order is not sorted."""
    g = DC._gen("restraint2_entry", seed)
    bl = b["batch_ligand"]
    pos = b["init_ligand_pos"]
    if pos is None:                                                                  # (init on the device: around the prior centres)
        pos = b["prior_centers"][b["ligand_decomp_batch"]]
    rows = []
    for k, n_r in enumerate(per_sample):
        mine = (bl == k).nonzero()[:, 0]
        n = len(mine)
        for i in range(n_r):
            a = int(torch.randint(0, n, (1,), generator=g))
            a2 = (a + 1 + int(torch.randint(0, n - 1, (1,), generator=g))) % n
            u = torch.randn(3, generator=g)
            p = pos[int(mine[a])].float() + u / u.norm() * (1.5 + 1.5 * float(torch.rand(1, generator=g)))
            w = weight[0] + (weight[1] - weight[0]) * float(torch.rand(1, generator=g))
            cl = sorted(set(int(c) for c in torch.randint(0, NUM_CLASSES, (3,), generator=g)))
            kind = i % 4
            r = dict(i=i, k=k, point=p, w=w, atom=-1, group=ANY, atom2=-1, group2=NONE, cls=None, cls2=None, form="linear", mn=0.8, mx=1.2)
            if kind == 0:
                r.update(atom=int(mine[a]), atom2=int(mine[a2]), form="harmonic")
            elif kind == 1:
                r.update(cls=cl)
            elif kind == 2:
                r.update(group=0, group2=SCA, cls2=list(range(NUM_CLASSES)), form="harmonic", mn=6.0, mx=INF)
            else:
                r.update(group2=ANY, mn=3.0, mx=INF)
            rows.append(r)
    rows.sort(key=lambda r: (r["i"], -r["k"]))                                       # interleaved, samples descending
    col = lambda key: torch.tensor([r[key] for r in rows])
    return dict(type="restraint", sample=col("k"), point=torch.stack([r["point"] for r in rows]).float() if rows else torch.zeros(0, 3),
                min_d=col("mn"), max_d=col("mx"), weight=col("w"), atom=col("atom"), group=col("group"), atom2=col("atom2"),
                group2=col("group2"), classes=[r["cls"] for r in rows], classes2=[r["cls2"] for r in rows],
                form=[r["form"] for r in rows], **opts)


def centred_case(b, entry, pos=None, v=None, centre=True):
    """The dense batch `b` (equal ligand sizes) and a general restraint entry as a case of this module in the kernel's frame:
    positions and points centred with the fp32 subtraction the model uses, explicit atoms as rows within their sample, restraints
    sorted by sample (stable) -- `order` maps the case's rows back to the entry's.  pos / v: another state of the same batch;
    centre=False: the frame of a center_pos_mode="none" call (no offset)."""
    B = int(b["batch_ligand"].max()) + 1
    NL = b["batch_ligand"].numel() // B
    off = RC.model_offsets(b) if centre else torch.zeros(B, 3)                      # (centre=False: center_pos_mode="none")
    x = (b["init_ligand_pos"] if pos is None else pos).float() - off[b["batch_ligand"]]
    order = torch.sort(entry["sample"], stable=True).indices
    R = int(entry["sample"].numel())
    get = lambda key, r, default: default if entry.get(key) is None else entry[key][r]
    rs = []
    for r in order.tolist():
        s = int(entry["sample"][r])
        d = dict(sample=s, point=(entry["point"][r].float() - off[s]).tolist(), min_d=float(entry["min_d"][r]), max_d=float(entry["max_d"][r]),
                 weight=float(entry["weight"][r]), atom=int(entry["atom"][r]) - s * NL if int(entry["atom"][r]) >= 0 else -1,
                 group=int(entry["group"][r]), cls=get("classes", r, None), cls2=get("classes2", r, None),
                 form=get("form", r, "linear") if not isinstance(entry.get("form"), str) else entry["form"])
        a2, g2 = int(get("atom2", r, -1)), get("group2", r, NONE)
        g2 = NONE if g2 is None else int(g2)
        if a2 >= 0:
            d.update(atom2=a2 - s * NL)
        elif g2 != NONE:
            d.update(group2=g2)
        rs.append(d)
    assert len(rs) == R
    return _case(B, NL, x, b["ligand_decomp_index"], (b["init_ligand_v"] if v is None else v), rs, order=order, offset=off)


def sampler_case(seed=SAMPLER_SEED, **opts):
    """drift_cases.sampler_batch (40 + 12 atoms, B = 2) with four general restraints per sample -> (batch, entry, case in the kernel's frame)."""
    b = DC.sampler_batch()
    e = batch_entry(b, ("sampler", seed), **opts)
    return b, e, centred_case(b, e)


known_buffer, report, model_offsets = RC.known_buffer, RC.report, RC.model_offsets
NAMES = tuple(_build_all())
