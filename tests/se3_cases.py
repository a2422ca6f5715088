"""The angles, axes and tiny graphs on which the pose graph's SE(3) maps are held to tests/se3_mp.py: on the CPU the numpy statement (tests/test_pgo_twin.py), on
the GPU the device code (tests/test_gpu_posegraph_se3.py). Built with se3_mp's Exp rounded to fp64, so that nothing here comes from the code under test."""
import numpy as np

import se3_mp as sm

PI = float(np.pi)
# 0; far below every switch; both sides of Log's switch to its small-angle form (|w| < 1e-6); inside the coefficient series; both sides of the series' switch
# (1e-2); ordinary angles; and towards pi, where atan2 takes over from asin and |w| falls again (the statement excludes only the last 1e-6 before pi)
ANGLES = (0.0, 1e-12, 1e-7, 0.999e-6, 1.001e-6, 5e-3, 1e-2 * (1 - 1e-9), 1e-2 * (1 + 1e-9), 0.3, 0.5 * PI, 2.0, PI - 0.1, PI - 1e-3, PI - 1e-5)
RETRACT_ANGLES = ANGLES[:-1]      # one Gauss-Newton step is checked up to pi - 1e-3: beyond, the statement's own step loses digits (8e-10 m at pi - 2e-6)

ODOM_VAR = np.array([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4])
PLANTED_V = np.array([12.0, -15.0, 5.0])      # 19.8 m: with ODOM_VAR, r^2 reaches 1e7 and more
KINDS = ("prior", "between", "cauchy1", "cauchy0.1")
LOSS = {"prior": None, "between": None, "cauchy1": 1.0, "cauchy0.1": 0.1}


def axes(n_random=2, seed=17):
    """unit axes: +-x, +-y, +-z (components of w exactly zero), yaw with roll and pitch at 1e-9 (the common case), and random ones"""
    out = [s * np.eye(3)[k] for k in range(3) for s in (1.0, -1.0)]
    out.append(np.array([1e-9, 1e-9, 1.0]))
    rng = np.random.default_rng(seed)
    out += list(rng.normal(size=(n_random, 3)))
    return [a / np.linalg.norm(a) for a in out]


def X_of_mp(X):
    return sm.floats(X[0]), sm.floats(X[1])


def T_of(X):
    T = np.eye(4); T[:3, :3] = X[0]; T[:3, 3] = X[1]
    return T


X0 = (np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), np.array([0.5, -0.25, 1.0]))      # its inverse and its products with itself are exact
Z = X_of_mp(sm.exp_se3(np.array([0.3, -0.2, 0.9, 4.0, -2.0, 1.0])))


def planted(kind, theta, axis, v=PLANTED_V):
    """-> spec (the form of pgo_twin.circuit, plus `loss`), the index of the factor with the planted error Exp([theta axis, v]), and the zero-error poses.
    prior: one pose Z Exp(xi) with the prior Z. Otherwise: X0 under a prior at X0 (its error is exactly zero), X1 = X0 Z Exp(xi), and the between factor Z from
    0 to 1, plain or under Cauchy(k)"""
    xi = np.concatenate([theta * np.asarray(axis, np.float64), v])
    E = sm.exp_se3(xi)
    if kind == "prior":
        X = X_of_mp(sm.mul(Z, E))
        return dict(initial=[X], priors=[(0, T_of(Z), ODOM_VAR)], betweens=[], loss=[]), 0, [Z]
    X1 = X_of_mp(sm.mul(sm.mul(X0, Z), E))
    rest = X_of_mp(sm.mul(X0, Z))
    return dict(initial=[X0, X1], priors=[(0, T_of(X0), np.full(6, 1e-4))], betweens=[(0, 1, T_of(Z), ODOM_VAR)], loss=[LOSS[kind]]), 1, [X0, rest]


def planted_error(kind, spec):
    """the planted factor's error vector, r^2, weight and cost term in mpmath, from the spec's own doubles"""
    if kind == "prior":
        e = sm.log_se3(*sm.mul(sm.inv(Z), spec["initial"][0]))
    else:
        e = sm.log_se3(*sm.mul(sm.inv(Z), sm.mul(sm.inv(spec["initial"][0]), spec["initial"][1])))
    r2 = sm.whitened_r2(e, ODOM_VAR)
    k = LOSS[kind]
    rho, w = (r2 / 2, 1) if k is None else sm.cauchy(r2, k)
    return e, r2, w, rho
