"""Seeded grounds, vehicles and poses of the ground-prior tests (tests/test_prior_twin.py on the CPU, tests/test_gpu_groundprior.py on the device), and the
statement's results on them, computed once per process and shared: `solve_reference()` runs tests/prior_twin.py by both of its routes on every terrain and
records the spread between them, from which the device's bars derive (10 x the spread; never from the device)."""
import functools

import numpy as np

import prior_twin as tw

f32 = np.float32
HALF = 6.0          # the grounds cover [-6, 6]^2
N_GROUND = 6000     # about 47 neighbours in a fit's 0.6 m disc
FLAT_H = 0.37


def ground(kind, seed=1, n=N_GROUND, noise=0.0, stride=4):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-HALF, HALF, (n, 2))
    x, y = xy[:, 0], xy[:, 1]
    if kind == "flat":
        z = np.full(n, FLAT_H)
    elif kind == "tilt":
        z = 0.08 * x - 0.05 * y + 0.2
    elif kind == "gentle":
        z = 1e-3 * x - 5e-4 * y + 0.2
    elif kind == "curve":
        z = 0.01 * x * x - 0.008 * y * y + 0.03 * x
    else:
        raise KeyError(kind)
    z = z + noise * rng.standard_normal(n)
    out = np.zeros((n, stride), f32)
    out[:, 0], out[:, 1], out[:, 2] = x, y, z
    if stride > 3:
        out[:, 3] = rng.uniform(0, 255, n)
    return out


# name -> (kind, noise): the issue's four kinds of ground
TERRAINS = {"flat": ("flat", 0.0), "tilt": ("tilt", 0.0), "tilt_noise": ("tilt", 0.02), "curve": ("curve", 0.0)}
# the grounds on which the statement's end reason and iteration count are decisive for every pose (prior_twin.decisive): the Jacobian takes the ground point as
# fixed, so on a slope the step shrinks by a near-constant factor per iteration, about 10^2 at 8 % — the width of the band the rule keeps clear around tol_step —
# and some iteration lands inside the band for nearly every pose (measured: 0 to 1 of 6 poses decisive on `tilt`, `tilt_noise` and `curve`, all on these)
DISCRETE_TERRAINS = {"flat": ("flat", 0.0), "gentle": ("gentle", 0.0)}
VEHICLES = {"square": lambda **kw: tw.Params.square(2.0, **kw), "shipped": lambda **kw: tw.Params(**kw)}
N_POSES = 6


def poses(seed, n=N_POSES):
    """spread over the middle of a ground, every wheel well inside it; yaw over more than the full turn (wraps included)"""
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.5, 1.5, n), rng.uniform(-3.3, 3.3, n)])


@functools.lru_cache(maxsize=None)
def terrain_cloud(name):
    kind, noise = {**TERRAINS, **DISCRETE_TERRAINS}[name]
    return ground(kind, seed=1, noise=noise)


QUANTITIES = ("z", "roll", "pitch", "cost", "wheel_distance")


@functools.lru_cache(maxsize=None)
def solve_reference():
    """{(terrain, vehicle): (poses, [result by route A], [result by route B])} over all terrains, and the recorded spread {quantity: max |A - B|}"""
    out, spread = {}, {q: 0.0 for q in QUANTITIES}
    for ti, name in enumerate(list(TERRAINS) + [t for t in DISCRETE_TERRAINS if t not in TERRAINS]):
        cloud = terrain_cloud(name)
        for vi, (vname, make) in enumerate(VEHICLES.items()):
            P = make()
            ps = poses(100 + 10 * ti + vi)
            a = [tw.solve(cloud, P, *p) for p in ps]
            b = [tw.solve(cloud, P, *p, eig="eigh", lin="solve") for p in ps]
            for ra, rb in zip(a, b):
                for q in QUANTITIES:
                    spread[q] = max(spread[q], float(np.max(np.abs(np.asarray(ra[q]) - np.asarray(rb[q])))))
            out[(name, vname)] = (ps, a, b)
    return out, spread


# ---- constructed neighbourhoods for the fit ------------------------------------------------------------------------------------------------------------------
def ring_points(n, radius, z, centre=(0.0, 0.0), phase=0.0):
    a = phase + 2 * np.pi * np.arange(n) / max(n, 1)
    out = np.zeros((n, 4), f32)
    out[:, 0], out[:, 1], out[:, 2] = centre[0] + radius * np.cos(a), centre[1] + radius * np.sin(a), z
    return out


def fit_cases():
    """name -> (cloud, query xy, Params kwargs, expected fallback, expected hits, expected inliers). Far points (30 m off) make sure a nearest point exists that is
    not part of the neighbourhood's story"""
    far = np.array([[30.0, 30.0, 5.0, 0.0]], f32)
    cases = {}
    tilt = lambda p: (0.1 * p[:, 0] - 0.2 * p[:, 1] + 1.0).astype(f32)
    for n in (14, 15):   # exactly 14 and 15 hits
        c = ring_points(n, 0.3, 0.0)
        c[:, 2] = tilt(c)
        cases[f"hits_{n}"] = (np.vstack([c, far]), (0.01, -0.02), {}, tw.FIT_FEW_HITS if n < 15 else tw.FIT_OK, n, n if n >= 15 else 0)
    # exactly 15 and 14 inliers: the ring and one point far beyond the cut
    for keep in (15, 14):
        c = ring_points(keep, 0.3, 0.0)
        c[:, 2] = tilt(c)
        out3 = ring_points(1, 0.1, 1000.0, phase=0.3)   # one point 1000 m up: beyond mean + 3 sigma of keep + 1 points (sigma ~ 1000 sqrt(keep) / (keep + 1) ~ 242)
        cases[f"inliers_{keep}"] = (np.vstack([c, out3, far]), (0.0, 0.0), {}, tw.FIT_OK if keep >= 15 else tw.FIT_FEW_INLIERS, keep + 1, keep)
    # a vertical wall: 20 points in the plane x = 0.1, spread in y and z -> the normal is (1, 0, 0), |c| < 1e-6
    rng = np.random.default_rng(4)
    wall = np.zeros((20, 4), f32)
    wall[:, 0], wall[:, 1], wall[:, 2] = 0.1, rng.uniform(-0.3, 0.3, 20), rng.uniform(0.0, 2.0, 20)
    cases["vertical_wall"] = (np.vstack([wall, far]), (0.0, 0.0), {}, tw.FIT_VERTICAL, 20, 20)
    # points exactly ON the outlier bounds: 16 at z = 0, one at +3, one at -3 -> mean 0, sum of squares 18, sigma 1, bounds -3 and +3 exactly: inclusive keeps all 18
    c = ring_points(18, 0.3, 0.0)
    c[0, 2], c[9, 2] = 3.0, -3.0
    cases["on_the_bound"] = (np.vstack([c, far]), (0.0, 0.0), {}, tw.FIT_OK, 18, 18)
    # fewer than 3 inliers with fit_min_points = 1: FitPlane's own refusal
    cases["no_plane"] = (np.vstack([ring_points(2, 0.2, 0.5), far]), (0.0, 0.0), dict(fit_min_points=1), tw.FIT_NO_PLANE, 2, 2)
    return cases
