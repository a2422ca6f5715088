"""GPU: the pose graph's SE(3) maps on the device (log_se3, exp_se3, so3_coeffs and the Cauchy loss of rolo_amd/csrc/posegraph.hip, in the copies inside
pgo_linearize_kernel, linearize_robust, pgo_factor_error_kernel and pgo_retract_cost_kernel) against tests/se3_mp.py, mpmath at 60 digits written from the
mathematics, at every angle where the device code changes form and up to pi - 1e-5; tests/pgo_twin.py has the device's own branches and cannot show them wrong.

Tiny graphs (tests/se3_cases.py) whose one interesting factor has a planted error Exp([theta axis, v]), |v| = 19.8 m: one pose under a prior; two poses, a
zero-error prior and a between factor; the same under Cauchy(1) and Cauchy(0.1). With the odometry variances r^2 is 4e6 .. 1.4e7, so log1p(r^2 / k^2) and
w = k^2 / (k^2 + r^2) are checked at 1e-7 .. 1e-9, far from the scales of tests/test_gpu_posegraph_robust.py.

Bars. r^2, w and the cost against mpmath on the same doubles: BAR_LIN = 1e-9 relative, the project's bar for costs (the statement is within 1e-15 of mpmath:
tests/test_pgo_twin.py). Gradient and blocks against the statement at BAR_LIN, as everywhere: the Jacobian's series is the statement. The poses after one
Gauss-Newton step: 10 x what the statement's own step leaves (TWIN_RETRACT in tests/test_gpu_posegraph.py, measured by tests/test_pgo_twin.py), never tighter
than 1e-9 m / 1e-10 rad."""
import numpy as np
import pytest

import pgo_robust_twin as rt
import pgo_twin as tw
import se3_cases as sc
import se3_mp as sm
from rolo_amd.backend import pgo_params
from test_gpu_posegraph import BAR_LIN, TWIN_RETRACT, bars, rel
from test_gpu_posegraph_robust import device_graph

pytestmark = pytest.mark.gpu

ONE_STEP = dict(max_iterations=1, lambda_initial=0.0, absolute_error_tol=0.0, relative_error_tol=0.0)


def mp_rel(got, want):
    """|got - want| / want of a double against an mpmath number"""
    with sm.mp.workdps(sm.DIGITS):
        return float(abs(sm.mp.mpf(float(got)) - want) / want)


@pytest.mark.parametrize("kind", sc.KINDS)
def test_planted_error(kind):
    worst = dict(r2=0.0, w=0.0, cost=0.0, gradient=0.0, blocks=0.0)
    for theta in sc.ANGLES:
        for axis in sc.axes():
            spec, f, _ = sc.planted(kind, theta, axis)
            _, want_r2, want_w, want_rho = sc.planted_error(kind, spec)
            t = rt.build(spec)
            lin = t.linearize()
            g = device_graph(spec)
            try:
                r2, w = g.factorErrors()
                got = g.linearize()
            finally:
                g.close()
            where = (kind, theta, tuple(axis))
            if f == 1:      # the prior on X0 has no error at all
                assert r2[0] == 0.0 and w[0] == 1.0
            fig = dict(r2=mp_rel(r2[f], want_r2), w=mp_rel(w[f], want_w), cost=mp_rel(got[0], want_rho), gradient=rel(got[1], lin[1]),
                       blocks=max(rel(x, y) for a, b in zip(got[2:4], lin[2:4]) for x, y in zip(a, b)))
            if sc.LOSS[kind] is None:
                assert w[f] == 1.0
            for name, v in fig.items():
                worst[name] = max(worst[name], v)
                assert v <= BAR_LIN, (where, name, v)
            assert got[4].shape == (0, 6, 6)
    print(f"{kind}: worst relative differences, r^2, w and cost against mpmath, gradient and blocks against the statement: {worst}")


@pytest.mark.parametrize("kind", sc.KINDS)
def test_one_step_lands_on_the_zero_error_poses(kind):
    """lambda = 0: the Gauss-Newton step of a factor with Jr^-1 e = e (ad(e) e = 0) is delta = -e on the moved pose, and X Exp(-e) is the zero-error pose, at
    every angle. The poses after the step are also X Exp(delta) in mpmath for the delta that solveLinear(0) returns on an identical graph, which holds exp_se3
    and the retraction to the independent reference by themselves"""
    bm, br = bars(TWIN_RETRACT[kind])
    worst = [0.0, 0.0, 0.0, 0.0]
    for theta in sc.RETRACT_ANGLES:
        for axis in sc.axes():
            spec, f, rest = sc.planted(kind, theta, axis)
            g, h = device_graph(spec), device_graph(spec)
            try:
                r = g.optimize(pgo_params(**ONE_STEP))
                P = [tw.X_of(T) for T in g.poses()]
                h.linearize()
                delta = h.solveLinear(0.0)[0].reshape(-1, 6)
            finally:
                g.close(); h.close()
            where = (kind, theta, tuple(axis))
            assert (r["state"], r["iterations"], r["trials"]) == (tw.ITERATIONS, 1, 1), (where, r)
            dt, dr = sm.pose_distance(P, rest)
            et, er = sm.pose_distance(P, [sm.mul(X, sm.exp_se3(d)) for X, d in zip(spec["initial"], delta)])
            worst = [max(a, b) for a, b in zip(worst, (dt, dr, et, er))]
            assert dt <= bm and dr <= br, (where, dt, dr)
            assert et <= bm and er <= br, (where, et, er)
    print(f"{kind}: after one step, from the zero-error poses {worst[0]:.2e} m {worst[1]:.2e} rad; from mpmath's X Exp(delta) {worst[2]:.2e} m {worst[3]:.2e} rad")
