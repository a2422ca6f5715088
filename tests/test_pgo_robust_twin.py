"""CPU: tests/pgo_robust_twin.py, the numpy statement of the Cauchy-robust between factor (include/rolo_hip.h, "loss"), against finite differences of its own
cost, its limits in k, and itself on graphs with false loops (its direct solve against its preconditioned conjugate gradients). The figures the GPU test's bars
are derived from are measured here and asserted to stay below the constants recorded at the top of tests/test_gpu_posegraph_robust.py. Run with `pytest -s` to
see them."""
import numpy as np
import pytest

import pgo_robust_twin as rt
import pgo_twin as tw

from test_gpu_posegraph_robust import KS, LIN_CASES, PERTURBS, TWIN_ROBUST_STEP as RECORDED_STEP, TWIN_ROBUST_WHOLE as RECORDED_WHOLE   # the recorded figures live there

# the central difference of the cost against linearize()'s gradient, h = 1e-6, relative to the gradient's largest entry: measured 1.2e-7 at the worst of the three
# perturbations (the smallest: the third derivative of rho along a rotation with a 20 m lever is about 1e7, times h^2 / 6; the same graph without loss, whose cost
# is nearly quadratic, gives 4.5e-11). The bar is 10 x the measured figure, for the step's own truncation; a mis-stated w or rho misses it by more than 1e3
GRADIENT_BAR = 1.2e-6


def gradient_graph(perturb, k=1.0, seed=4):
    """4 poses, six between factors (the chain, two chords, one reversed), every variance drawn from 1e-2 .. 0.3, every factor under Cauchy(k)"""
    spec = tw.circuit(4, 0, seed=seed, laps=1)
    rng = np.random.default_rng(40 + seed)
    noise = lambda s: np.concatenate([rng.normal(0, s[0], 3), rng.normal(0, s[1], 3)])
    tr = spec["truth"]
    g = rt.Graph()
    for X in tr:
        g.add_pose(tw.T_of(tw.mul(X, tw.exp_se3(noise(perturb)))))
    for i, j in ((0, 1), (1, 2), (2, 3), (0, 3), (3, 1), (0, 2)):
        Z = tw.mul(tw.mul(tw.inv(*tr[i]), tr[j]), tw.exp_se3(noise((1e-3, 1e-2))))
        g.add_between(i, j, tw.T_of(Z), 10.0 ** rng.uniform(-2.0, np.log10(0.3), 6), k)
    return g


def central_difference(g, h=1e-6):
    n = 6 * len(g.poses)
    fd = np.zeros(n)
    for q in range(n):
        d = np.zeros(n); d[q] = h
        fd[q] = (g.cost(g.retract(d)) - g.cost(g.retract(-d))) / (2.0 * h)
    return fd


def test_gradient_is_that_of_the_cost():
    """w J^T e_w is the gradient of rho = k^2 / 2 log1p(r^2 / k^2): a mis-stated w or rho fails here. r^2 from well below k^2 to well above it"""
    worst, lo, hi = 0.0, np.inf, 0.0
    for perturb in ((1e-3, 5e-3), (1e-2, 5e-2), (3e-2, 3e-1)):
        g = gradient_graph(perturb)
        r2, w = g.factor_errors()
        lo, hi = min(lo, r2.min()), max(hi, r2.max())
        grad = g.linearize()[1]
        fd = central_difference(g)
        err = np.abs(fd - grad).max() / np.abs(grad).max()
        print(f"perturbation {perturb}: r^2 {r2.min():.3g} .. {r2.max():.3g}, w {w.min():.3g} .. {w.max():.3g}, central difference against the gradient {err:.2e}")
        worst = max(worst, err)
        plain = rt.Graph()
        plain.poses = g.poses; plain.factors = g.factors; plain.k = [None] * len(g.k)
        print(f"    the same graph without loss: {np.abs(central_difference(plain) - plain.linearize()[1]).max() / np.abs(plain.linearize()[1]).max():.2e}")
    print(f"r^2 spans {lo:.3g} .. {hi:.3g}; worst {worst:.2e}")
    assert lo < 0.1 and hi > 100.0      # both sides of k^2 = 1
    assert worst <= GRADIENT_BAR


def test_a_wrong_weight_or_loss_is_caught():
    """the guard itself: the gradient of the plain cost (w = 1) and the Cauchy weight paired with the plain cost both miss the bar by orders of magnitude"""
    g = gradient_graph((1e-2, 5e-2))
    grad = g.linearize()[1]
    plain = rt.Graph()
    plain.poses = g.poses; plain.factors = g.factors; plain.k = [None] * len(g.k)
    assert np.abs(central_difference(plain) - grad).max() / np.abs(grad).max() > 1e3 * GRADIENT_BAR      # rho mis-stated as r^2 / 2
    assert np.abs(central_difference(g) - plain.linearize()[1]).max() / np.abs(grad).max() > 1e3 * GRADIENT_BAR      # w mis-stated as 1


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    return float(np.abs(a - b).max() / np.abs(b).max()) if a.size else 0.0


def test_a_huge_k_is_the_plain_factor():
    spec = rt.robust_case_spec(65, "one", k=1e9)
    a, b = rt.build(spec).linearize(), tw.build(spec).linearize()
    worst = max(rel(a[0], b[0]), rel(a[1], b[1]), max(rel(x, y) for x, y in zip(a[2], b[2])), max(rel(x, y) for x, y in zip(a[3], b[3])), rel(a[4], b[4]))
    print("k = 1e9 against the plain twin: cost, gradient and blocks within", worst)
    assert worst <= 1e-12 and np.array_equal(a[5], b[5])
    r2, w = rt.build(spec).factor_errors()
    assert np.all(w[:-1] == 1.0) and abs(w[-1] - 1.0) <= 1e-15


def test_zero_error_has_weight_one_and_no_cost():
    spec = tw.exact_chain(3)
    spec["loss"] = [1.0, 0.1]
    g = rt.build(spec)
    r2, w = g.factor_errors()
    assert not np.any(r2) and np.all(w == 1.0)
    cost, grad = g.linearize()[:2]
    assert cost == 0.0 and g.cost() == 0.0 and not np.any(grad)


def test_plain_factors_are_the_plain_twin():
    """a graph without a robust factor: the same bits as pgo_twin.Graph"""
    spec = tw.case_spec(65, "pair2")
    a, b = rt.build(spec).linearize(), tw.build(spec).linearize()
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))
    assert rt.build(spec).cost() == tw.build(spec).cost()


def test_pcg_against_the_direct_solve_on_the_robust_graphs():
    """the graphs of the GPU test's linearisation cases: the figure its step bar is 10 x of"""
    worst = 0.0
    for n, kind in LIN_CASES:
        for perturb in PERTURBS:
            for k in KS:
                g = rt.build(rt.robust_case_spec(n, kind, perturb, k))
                lin = g.linearize()
                for lam in (0.0, 1e-5):
                    d, its, _ = tw.Graph.solve_pcg(lin, lam)
                    dd = tw.Graph.solve_direct(lin, lam)
                    assert its <= tw.Graph.pcg_cap(len(g.chords()))
                    worst = max(worst, np.abs(d - dd).max() / np.abs(dd).max())
    print("twin PCG against twin direct solve on the robust graphs, largest relative difference of the step:", worst)
    assert worst <= RECORDED_STEP


# ---- the outlier graphs of tests/test_gpu_posegraph_robust.py: the twin's two entry points against each other, and the conditions the twin itself must meet ----
@pytest.fixture(scope="module")
def whole():
    out = {}
    for n in rt.OUTLIER_SIZES:
        spec = rt.outlier_spec(n)
        for solver in ("direct", "pcg"):
            for name, kw in (("strict", tw.STRICT), ("default", {})):
                g = rt.build(spec)
                out[n, solver, name] = (g.optimize(solver, **kw), g.poses, g.factor_errors())
    return out


def test_false_loops_are_where_the_issue_puts_them():
    for n in rt.OUTLIER_SIZES:
        spec = rt.outlier_spec(n)
        assert [spec["betweens"][f - 1][:2] for f in spec["false_loops"]] == [(n - 1, n - 1 - n // 4), (n - 4, n - 9 - n // 4)]
        assert len(spec["true_loops"]) == 4 and all(spec["loss"][f - 1] == 1.0 for f in spec["true_loops"] + spec["false_loops"])
        assert all(k is None for k in spec["loss"][:n - 1])


@pytest.mark.parametrize("n", rt.OUTLIER_SIZES)
def test_entry_points_agree_on_the_outlier_graphs(whole, n):
    c, d = whole[n, "direct", "default"], whole[n, "pcg", "default"]
    # the condition under which the GPU test asserts the counts and the accepted flags: the two entry points agree on them
    assert (c[0]["state"], c[0]["iterations"], c[0]["trials"]) == (d[0]["state"], d[0]["iterations"], d[0]["trials"]) and c[0]["state"] == tw.CONVERGED
    assert [t[2] for t in c[0]["trace"]] == [t[2] for t in d[0]["trace"]]
    dt, dr = tw.pose_distance(c[1], d[1])
    print(f"N = {n}, defaults: (state, iterations, trials) {(d[0]['state'], d[0]['iterations'], d[0]['trials'])}, direct against PCG {dt:.3e} m {dr:.3e} rad")
    assert dt <= 1e-12
    a, b = whole[n, "direct", "strict"], whole[n, "pcg", "strict"]     # (at the floor the accepted flags differ in the last bit of a cost: no counts held)
    dt, dr = tw.pose_distance(a[1], b[1])
    print(f"N = {n}, STRICT: twin direct against twin PCG at the optimum: {dt:.3e} m, {dr:.3e} rad; final costs {a[0]['final_cost']!r} {b[0]['final_cost']!r}")
    assert abs(a[0]["final_cost"] - b[0]["final_cost"]) <= 1e-9 * b[0]["final_cost"]
    assert dt <= RECORDED_WHOLE[n][0] and dr <= RECORDED_WHOLE[n][1]


@pytest.mark.parametrize("n", rt.OUTLIER_SIZES)
@pytest.mark.parametrize("solver,name", [("direct", "strict"), ("pcg", "strict"), ("direct", "default"), ("pcg", "default")])
def test_the_optimum_outvotes_the_false_loops(whole, n, solver, name):
    spec = rt.outlier_spec(n)
    r2, w = whole[n, solver, name][2]
    loops = spec["true_loops"] + spec["false_loops"]
    print(f"N = {n} {solver} {name}: weights of the true loops {w[spec['true_loops']]}, of the false loops {w[spec['false_loops']]}")
    assert np.all(w[spec["false_loops"]] <= 1e-3)
    assert np.all(w[spec["true_loops"]] >= 0.1)
    assert np.all(np.delete(w, loops) == 1.0)


def test_robust_loops_keep_the_trajectory_and_plain_ones_bend_it(whole):
    n = 120
    truth = rt.outlier_spec(n)["truth"]
    clean = tw.build(tw.circuit(n, 4, seed=n)); clean.optimize("direct")
    plain = rt.build(rt.outlier_spec(n), plain=True); plain.optimize("direct")
    e_clean, e_plain = tw.max_position_error(clean.poses, truth), tw.max_position_error(plain.poses, truth)
    e_robust = tw.max_position_error(whole[n, "pcg", "default"][1], truth)
    print(f"largest position error against truth: clean {e_clean:.3f} m, false loops under Cauchy(1) {e_robust:.3f} m, false loops with plain factors {e_plain:.3f} m")
    assert e_robust <= e_clean + 0.5
    assert e_plain >= 3.0
