"""CPU: tests/pgo_twin.py, the numpy statement of the pose-graph optimisation (include/rolo_hip.h), against finite differences, known answers, mpmath
(tests/se3_mp.py: Exp and Log written from the mathematics, at every angle where the statement changes form) and itself (its direct solve against its
preconditioned conjugate gradients). The figures the GPU test's bars are derived from are measured here and asserted to stay
below the constants recorded at the top of tests/test_gpu_posegraph.py."""
import numpy as np
import pytest

import pgo_robust_twin as rt
import pgo_twin as tw
import se3_cases as sc
import se3_mp as sm

from test_gpu_posegraph import (TWIN_LIFE as RECORDED_LIFE, TWIN_REFERENCE as RECORDED_REFERENCE, TWIN_RETRACT as RECORDED_RETRACT, TWIN_STEP as RECORDED_STEP,
                                TWIN_WHOLE as RECORDED_WHOLE)   # the recorded figures live there


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


def test_exp_and_log_against_mpmath():
    """the statement's Exp and Log against tests/se3_mp.py on the same doubles: every angle of se3_cases.ANGLES (both sides of each switch of form, and up to
    pi - 1e-5), 20 random axes and the exact and near-yaw ones, translations up to 20 m. Relative to the largest entry of mpmath's vector (for R: to 1)"""
    rng = np.random.default_rng(3)
    worst_exp = worst_log = 0.0
    for th in sc.ANGLES:
        for axis in sc.axes(20, seed=5):
            xi = np.concatenate([th * axis, rng.uniform(-20.0, 20.0, 3)])
            R, t = tw.exp_se3(xi)
            Rm, tm = sm.exp_se3(xi)
            tm = sm.floats(tm)
            worst_exp = max(worst_exp, np.abs(R - sm.floats(Rm)).max(), np.abs(t - tm).max() / np.abs(tm).max())
            want = sm.floats(sm.log_se3(R, t))      # Log of the statement's own doubles: the same input on both sides
            worst_log = max(worst_log, np.abs(tw.log_se3(R, t) - want).max() / np.abs(want).max())
    print(f"the statement against mpmath, worst relative difference: Exp {worst_exp:.2e}, Log {worst_log:.2e}")
    assert worst_exp <= 1e-14 and worst_log <= 1e-14


@pytest.mark.parametrize("kind", sc.KINDS)
def test_one_gauss_newton_step_lands_on_the_zero_error_poses(kind):
    """lambda = 0 on the planted graphs of tests/se3_cases.py: Jr^-1 e = e, so the step is -e and X Exp(-e) the zero-error pose at every angle; the distance
    left is the figure the bar of tests/test_gpu_posegraph_se3.py is 10 x of"""
    worst = {}
    for th in sc.RETRACT_ANGLES:
        wt = wr = 0.0
        for axis in sc.axes():
            spec, _, rest = sc.planted(kind, th, axis)
            g = rt.build(spec)
            r = g.optimize("direct", max_iterations=1, lambda_initial=0.0, absolute_error_tol=0.0, relative_error_tol=0.0)
            assert (r["state"], r["iterations"], r["trials"]) == (tw.ITERATIONS, 1, 1), (th, axis, r)
            dt, dr = sm.pose_distance(g.poses, rest)
            wt, wr = max(wt, dt), max(wr, dr)
        worst[th] = (wt, wr)
    print(kind, "after one step, (m, rad) from the zero-error poses by angle:", {f"{th:.6g}": (f"{a:.1e}", f"{b:.1e}") for th, (a, b) in worst.items()})
    assert max(v[0] for v in worst.values()) <= RECORDED_RETRACT[kind][0] and max(v[1] for v in worst.values()) <= RECORDED_RETRACT[kind][1]


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
    worst, by_size = 0.0, {}
    for n, kind in tw.CASES + tw.CASES_LARGE:
        g = tw.build(tw.case_spec(n, kind))
        lin = g.linearize()
        for lam in (0.0, 1e-5):
            d, its, _ = tw.Graph.solve_pcg(lin, lam)
            dd = tw.Graph.solve_direct(lin, lam)
            assert its <= tw.Graph.pcg_cap(len(g.chords()))
            worst = max(worst, np.abs(d - dd).max() / np.abs(dd).max())
            by_size[n] = max(by_size.get(n, 0.0), np.abs(d - dd).max() / np.abs(dd).max())
    print("twin PCG against twin direct solve, largest relative difference of the step:", worst, "by size:", {n: f"{v:.2e}" for n, v in by_size.items()})
    assert worst <= RECORDED_STEP
    assert max(by_size[n] for n in tw.SIZES_LARGE) <= max(by_size[n] for n in tw.SIZES)      # the sizes past 1 024 poses did not widen the figure


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


def test_the_grown_graph_reaches_the_optimum_of_the_whole():
    """the graph of tests/test_gpu_posegraph_life.py, grown on the statement as that test grows it on the device (one key pose and one default optimize per step,
    PCG, then STRICT), against the statement's direct solve on the whole graph from the composed odometry: the figure that test's last bar is 10 x of"""
    steps, spec = rt.life_script()
    g = rt.Graph()
    moved = []
    rt.grow_life(steps, tw.T_of(spec["initial"][0]), g.add_pose, g.add_prior, g.add_between, lambda: tw.T_of(g.poses[-1]),
                 lambda n, ops: moved.append((n, g.optimize("pcg")["iterations"])))
    ends = [(f[1], -1) if f[0] == "prior" else (f[1], f[2]) for f in spec["factors"]]
    assert ends == [(i, j) for i, j, _, _ in g.factors] and g.k == [f[5] if f[0] == "between" else None for f in spec["factors"]]      # the same graph
    assert all(its >= 1 for n, its in moved if n in spec["events"])      # every event moves the graph
    a = g.optimize("pcg", **tw.STRICT)
    whole = {}
    for solver in ("direct", "pcg"):
        t = rt.build_life(spec)
        whole[solver] = (t.optimize(solver, **tw.STRICT), t.poses)
    b = whole["direct"][0]
    dt, dr = tw.pose_distance(g.poses, whole["direct"][1])
    print(f"grown against whole: {dt:.3e} m {dr:.3e} rad, costs {a['final_cost']!r} {b['final_cost']!r}; whole, direct against PCG:", tw.pose_distance(whole["direct"][1], whole["pcg"][1]))
    assert abs(a["final_cost"] - b["final_cost"]) <= 1e-9 * b["final_cost"] and dt <= RECORDED_LIFE[0] and dr <= RECORDED_LIFE[1]
