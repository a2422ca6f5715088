"""CPU: tests/pgo_twin.py, the numpy statement of the pose-graph optimisation (include/rolo_hip.h), against finite differences, known answers and itself
(its direct solve against its preconditioned conjugate gradients). The figures the GPU test's bars are derived from are measured here and asserted to stay
below the constants recorded at the top of tests/test_gpu_posegraph.py."""
import numpy as np
import pytest

import pgo_twin as tw

from test_gpu_posegraph import TWIN_REFERENCE as RECORDED_REFERENCE, TWIN_STEP as RECORDED_STEP, TWIN_WHOLE as RECORDED_WHOLE   # the recorded figures live there


def rand_xi(rng, th, tscale=1.0):
    w = rng.normal(size=3); w *= th / np.linalg.norm(w)
    return np.concatenate([w, tscale * rng.normal(size=3)])


@pytest.mark.parametrize("th", [0.0, 1e-12, 1e-7, 5e-3, 1e-2, 0.3, 2.0, np.pi - 0.1])
def test_exp_log_round_trip(th):
    rng = np.random.default_rng(3)
    for _ in range(20):
        xi = rand_xi(rng, th) if th > 0 else np.concatenate([np.zeros(3), rng.normal(size=3)])
        R, t = tw.exp_se3(xi)
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-14
        assert np.abs(tw.log_se3(R, t) - xi).max() < 1e-12 * max(1.0, np.abs(xi).max())
        R2, t2 = tw.exp_se3(tw.log_se3(R, t))
        assert np.abs(R2 - R).max() < 1e-13 and np.abs(t2 - t).max() < 1e-12


def test_coefficient_series_meet_the_closed_forms():
    lo, hi = np.array(tw.coeffs(tw.SMALL * (1 - 1e-9))), np.array(tw.coeffs(tw.SMALL * (1 + 1e-9)))
    assert np.abs(lo - hi).max() < 1e-11   # (C and D lose eps / th^2 in the closed form: 1e-12 at the switch)


def numeric_jacobians(g, f, h=1e-6):
    i, j, _, _ = g.factors[f]
    out = []
    for k in (i, j):
        if k < 0:
            out.append(None); continue
        J = np.zeros((6, 6))
        for a in range(6):
            d = np.zeros(6); d[a] = h
            P = list(g.poses); P[k] = tw.mul(g.poses[k], tw.exp_se3(d)); ep = g.factor(f, P)[0]
            P[k] = tw.mul(g.poses[k], tw.exp_se3(-d)); em = g.factor(f, P)[0]
            J[:, a] = (ep - em) / (2 * h)
        out.append(J)
    return out


def test_jacobians_against_central_differences():
    """errors up to 0.25 rad / 0.5 m: the series of Jr^-1 is cut after ad^4, its next term |e|^6 / 30240 is below 1e-7 there"""
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(30):
        g = tw.Graph()
        Xa, Xb = tw.exp_se3(rand_xi(rng, rng.uniform(0.1, 2.5), 3.0)), tw.exp_se3(rand_xi(rng, rng.uniform(0.1, 2.5), 3.0))
        g.add_pose(tw.T_of(Xa)); g.add_pose(tw.T_of(Xb))
        var = 10.0 ** rng.uniform(-4, 0, 6)
        g.add_prior(0, tw.T_of(tw.mul(Xa, tw.exp_se3(rand_xi(rng, rng.uniform(0, 0.25), 0.3)))), var)
        Z = tw.mul(tw.mul(tw.inv(*Xa), Xb), tw.exp_se3(rand_xi(rng, rng.uniform(0, 0.25), 0.3)))
        g.add_between(0, 1, tw.T_of(Z), var)
        g.add_between(1, 0, tw.T_of(tw.inv(*Z)), var)
        for f in range(3):
            _, Ji, Jj = g.factor(f)
            Ni, Nj = numeric_jacobians(g, f)
            for A, B in ((Ji, Ni), (Jj, Nj)):
                if B is not None:
                    worst = max(worst, np.abs(A - B).max() / np.abs(B).max())
    print("analytic against central differences:", worst)
    assert worst <= 1e-6


@pytest.mark.parametrize("solver", ["direct", "pcg"])
def test_zero_residual_chain_stays_and_converges(solver):
    g = tw.build(tw.exact_chain(40))
    before = [tw.T_of(X) for X in g.poses]
    r = g.optimize(solver)
    assert r["state"] == tw.CONVERGED and r["iterations"] == 0 and r["trials"] == 1 and r["initial_cost"] == 0.0 and r["final_cost"] == 0.0
    assert all(np.array_equal(a, tw.T_of(X)) for a, X in zip(before, g.poses))
    assert tw.Graph.solve_pcg(g.linearize(), 1e-5)[1:] == (0, 0.0) and not np.any(tw.Graph.solve_pcg(g.linearize(), 0.0)[0])


@pytest.mark.parametrize("a,b", [(1e-2, 1e-2), (1e-2, 4e-2), (1e-4, 0.3)])
def test_two_conflicting_betweens_meet_at_the_information_weighted_mean(a, b):
    """two poses without rotation, pose 0 pinned: the optimum's relative translation is (z1 / a + z2 / b) / (1 / a + 1 / b)"""
    g = tw.Graph()
    g.add_pose(np.eye(4)); T1 = np.eye(4); T1[:3, 3] = [1.0, 0.2, 0.0]; g.add_pose(T1)
    g.add_prior(0, np.eye(4), np.full(6, 1e-6))
    z1, z2 = np.array([1.0, 0.0, 0.1]), np.array([1.4, -0.2, 0.0])
    for z, v in ((z1, a), (z2, b)):
        Z = np.eye(4); Z[:3, 3] = z
        g.add_between(0, 1, Z, np.full(6, v))
    r = g.optimize("pcg", absolute_error_tol=0.0, relative_error_tol=0.0, max_iterations=50)
    rel = tw.mul(tw.inv(*g.poses[0]), g.poses[1])
    want = (z1 / a + z2 / b) / (1 / a + 1 / b)
    assert np.abs(rel[1] - want).max() < 1e-9 and np.abs(rel[0] - np.eye(3)).max() < 1e-9, (rel, want, r)


def test_every_exit():
    spec = tw.circuit(65, 1, seed=65)
    r = tw.build(spec).optimize("pcg", relative_error_tol=0.0)
    acc = [t for t in r["trace"] if t[2]]
    assert r["state"] == tw.CONVERGED and r["iterations"] == len(acc) >= 1
    r2 = tw.build(spec).optimize("pcg", absolute_error_tol=0.0)
    assert r2["state"] == tw.CONVERGED and r2["iterations"] >= 1
    last, prev = r2["trace"][-1][1], (r2["trace"][-2][1] if len(r2["trace"]) > 1 else r2["initial_cost"])
    assert 0 < prev - last <= 1e-5 * prev
    r3 = tw.build(spec).optimize("pcg", max_iterations=1, absolute_error_tol=0.0, relative_error_tol=0.0)
    assert r3["state"] == tw.ITERATIONS and r3["iterations"] == 1
    r4 = tw.build(spec).optimize("pcg", lambda_initial=1e-3, lambda_upper=1e-4)
    assert r4["state"] == tw.LAMBDA and r4["trials"] == 0 and r4["final_cost"] == r4["initial_cost"]
    r5 = tw.build(spec).optimize("pcg", absolute_error_tol=0.0, relative_error_tol=0.0, max_iterations=50)   # at the floor no trial lowers the cost: lambda climbs to its bound
    assert r5["state"] == tw.LAMBDA and r5["trials"] > r5["iterations"]
    lams = [t[0] for t in r5["trace"]]
    for (l0, _, acc0, _), l1 in zip(r5["trace"], lams[1:]):
        assert np.isclose(l1, l0 / 10.0 if acc0 else l0 * 10.0, rtol=1e-12)


def test_pcg_without_chords_takes_one_iteration():
    for n in (1, 2, 5, 64):
        lin = tw.build(tw.case_spec(n, "none")).linearize()
        for lam in (0.0, 1e-5):
            d, its, res = tw.Graph.solve_pcg(lin, lam)
            assert its == 1 and np.abs(d - tw.Graph.solve_direct(lin, lam)).max() <= 1e-9 * np.abs(d).max()


def test_pcg_against_the_direct_solve_on_the_test_graphs():
    worst = 0.0
    for n, kind in tw.CASES:
        g = tw.build(tw.case_spec(n, kind))
        lin = g.linearize()
        for lam in (0.0, 1e-5):
            d, its, _ = tw.Graph.solve_pcg(lin, lam)
            dd = tw.Graph.solve_direct(lin, lam)
            assert its <= tw.Graph.pcg_cap(len(g.chords()))
            worst = max(worst, np.abs(d - dd).max() / np.abs(dd).max())
    print("twin PCG against twin direct solve, largest relative difference of the step:", worst)
    assert worst <= RECORDED_STEP


# ---- the twin's two entry points against each other on the graphs of tests/test_gpu_posegraph.py: the figures its bars are 10 x of ----
@pytest.fixture(scope="module")
def whole():
    out = {}
    for n, loops in tw.WHOLE:
        spec = tw.circuit(n, loops, seed=n)
        for solver in ("direct", "pcg"):
            for name, kw in (("strict", tw.STRICT), ("default", {})):
                g = tw.build(spec)
                out[n, solver, name] = (g.optimize(solver, **kw), g.poses)
    return out


@pytest.mark.parametrize("n", [n for n, _ in tw.WHOLE])
def test_entry_points_agree_on_whole_optimisations(whole, n):
    a, b = whole[n, "direct", "strict"], whole[n, "pcg", "strict"]
    dt, dr = tw.pose_distance(a[1], b[1])
    print(f"N = {n}: twin direct against twin PCG at the optimum: {dt:.3e} m, {dr:.3e} rad; final costs {a[0]['final_cost']!r} {b[0]['final_cost']!r}")
    assert a[0]["state"] == b[0]["state"] and abs(a[0]["final_cost"] - b[0]["final_cost"]) <= 1e-9 * b[0]["final_cost"]
    assert dt <= RECORDED_WHOLE[n][0] and dr <= RECORDED_WHOLE[n][1]
    c, d = whole[n, "direct", "default"][0], whole[n, "pcg", "default"][0]
    # the condition under which the GPU test asserts the counts: the two entry points agree on them
    assert (c["state"], c["iterations"], c["trials"]) == (d["state"], d["iterations"], d["trials"]) and c["state"] == tw.CONVERGED


def test_entry_points_agree_under_the_reference_prior():
    """120 poses, 4 loops through the reference's own calls and noise models: cond(H) ~ 1e17, so only gauge-free quantities are compared, at the optimum"""
    ref = tw.reference_spec()
    res = {}
    for solver in ("direct", "pcg"):
        g = tw.build_reference(ref)
        p0 = g.poses[0]
        r = g.optimize(solver, **tw.STRICT)
        res[solver] = (r, g.poses)
        moved = tw.pose_distance([p0], [g.poses[0]])
        print(solver, "pose 0 moved", moved)
        assert moved[0] <= 1e-2 and moved[1] <= 1e-4
    a, b = res["direct"], res["pcg"]
    dt, dr = tw.pose_distance(tw.relative_to_first(a[1]), tw.relative_to_first(b[1]))
    print(f"relative poses, twin direct against twin PCG: {dt:.3e} m, {dr:.3e} rad")
    assert abs(a[0]["final_cost"] - b[0]["final_cost"]) <= 1e-6 * b[0]["final_cost"] and dt <= RECORDED_REFERENCE[0] and dr <= RECORDED_REFERENCE[1]


def test_the_twin_halves_the_drift():
    spec = tw.drift_spec()
    g = tw.build(spec)
    before = tw.max_position_error(g.poses, spec["truth"])
    r = g.optimize("direct")
    after = tw.max_position_error(g.poses, spec["truth"])
    print("largest position error against truth:", before, "->", after)
    assert r["state"] == tw.CONVERGED and after <= 0.5 * before
