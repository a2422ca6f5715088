"""GPU: between factors under a Cauchy loss on the device (rolo_pgo_add_between_robust, rolo_pgo_get_factor_errors; PoseGraph.addBetween(cauchy=),
factorErrors, LoopFactor) against the numpy statement tests/pgo_robust_twin.py: the reweighted linearisation block by block, the linear step, every factor's
r^2 and weight, whole optimisations of graphs with false loops, the limit of a huge k, every error, and the way from LoopCloser's result into the graph.

Bars, by the rules of tests/test_gpu_posegraph.py. Cost, gradient, blocks, r^2 and w: 1e-9 relative (blocks and vectors to their largest magnitude; r^2 and w
entry by entry on the graphs whose every residual is moved off zero, and to the vector's largest entry on the circuit, whose prior and chain start at zero
error). The step and the poses: 10 x what the twin's two entry points differ by on the same graphs, measured on the CPU by
tests/test_pgo_robust_twin.py, which asserts that the figures below still hold; never tighter than 1e-9 (step), 1e-9 m / 1e-10 rad (poses)."""
import ctypes as C

import numpy as np
import pytest

import pgo_robust_twin as rt
import pgo_twin as tw
from rolo_amd._lib import RoloError, lib
from rolo_amd.backend import KeyFrameMap, LoopCloser, LoopFactor, PoseGraph, pgo_params

pytestmark = pytest.mark.gpu

# measured by tests/test_pgo_robust_twin.py (numpy 2 / scipy, fp64), printed there with `pytest -s`:
TWIN_ROBUST_STEP = 2.8e-8                                               # test_pcg_against_the_direct_solve_on_the_robust_graphs: largest relative difference of the step
TWIN_ROBUST_WHOLE = {65: (1.9e-10, 5.1e-12), 120: (6.0e-9, 1.4e-10)}    # test_entry_points_agree_on_the_outlier_graphs: (m, rad) at the optimum under tw.STRICT

BAR_LIN = 1e-9
BAR_STEP = max(10.0 * TWIN_ROBUST_STEP, 1e-9)
EINVAL, ESTATE, EUNSUPPORTED = -1, -5, -7
CAUCHY = 1     # ROLO_PGO_LOSS_CAUCHY

PERTURBS = ((1e-2, 5e-2), (3e-2, 3e-1))
KS = (1.0, 0.1)
# (poses, kind): every kind at sizes around the solve's power-of-two padding; `one` with F = 127, 128, 129, where the robust factor is the last thread of the
# first workgroup of the factor kernels (128 threads), then the first thread of the second
LIN_CASES = [(n, kind) for n in (3, 5, 64, 65) for kind in rt.ROBUST_KINDS] + [(n, "one") for n in (126, 127, 128)]


def bars(rec):
    return max(10.0 * rec[0], 1e-9), max(10.0 * rec[1], 1e-10)


def device_graph(spec, plain=False):
    g = PoseGraph()
    loss = spec.get("loss", [None] * len(spec["betweens"]))
    for X in spec["initial"]:
        g.addPose(tw.T_of(X))
    for i, T, v in spec["priors"]:
        g.addPrior(i, T, v)
    for (i, j, T, v), k in zip(spec["betweens"], loss):
        if plain or k is None:
            g.addBetween(i, j, T, v)
        else:
            g.addBetween(i, j, T, v, cauchy=k)
    return g


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / np.abs(b).max()) if a.size and np.abs(b).max() > 0 else float(np.abs(a).max()) if a.size else 0.0


def each_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and np.all(b > 0), (a.shape, b.shape)
    return float((np.abs(a - b) / b).max())


def same_bits(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


# ---- 1. linearisation, the linear step and the factor errors ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin_lin():
    cache = {}

    def get(n, kind, perturb, k):
        key = (n, kind, perturb, k)
        if key not in cache:
            spec = rt.robust_case_spec(n, kind, perturb, k)
            t = rt.build(spec)
            cache[key] = (spec, t, t.linearize(), t.factor_errors())
        return cache[key]
    return get


@pytest.mark.parametrize("n,kind", LIN_CASES)
def test_linearisation_and_step(twin_lin, n, kind):
    for perturb in PERTURBS:
        for k in KS:
            spec, t, lin, _ = twin_lin(n, kind, perturb, k)
            g = device_graph(spec)
            try:
                assert g.size() == (n, len(t.factors), len(t.chords()))
                if kind == "chain2":
                    assert g.size()[2] == 0 and t.k[-1] == k      # a robust factor in the chain block
                if kind == "one":
                    assert g.size()[1] == n + 1
                got = g.linearize()
                names = ("cost", "gradient", "diagonal", "chain", "chord")
                assert rel(got[0], lin[0]) <= BAR_LIN and rel(got[1], lin[1]) <= BAR_LIN, (perturb, k, rel(got[0], lin[0]), rel(got[1], lin[1]))
                for name, a, b in zip(names[2:], got[2:5], lin[2:5]):
                    assert a.shape == b.shape, name
                    worst = max([rel(x, y) for x, y in zip(a, b)], default=0.0)     # block by block
                    assert worst <= BAR_LIN, (perturb, k, name, worst)
                assert np.array_equal(got[5], lin[5])
                assert same_bits(got, g.linearize())     # the same bits on every run
                for lam in (0.0, 1e-5):
                    d, its, res = g.solveLinear(lam)
                    want = tw.Graph.solve_direct(lin, lam)
                    assert np.all(np.isfinite(d)) and np.isfinite(res)
                    assert (its == 1) if len(t.chords()) == 0 else (1 <= its <= 12 * len(t.chords()) + 2)
                    print(f"N = {n} {kind} perturbation {perturb} k = {k} lambda = {lam}: {its} iterations, residual {res:.2e}, step against the twin's direct solve "
                          f"{rel(d, want):.2e}")
                    assert rel(d, want) <= BAR_STEP
            finally:
                g.close()


@pytest.mark.parametrize("n,kind", LIN_CASES)
def test_factor_errors(twin_lin, n, kind):
    for perturb in PERTURBS:
        for k in KS:
            spec, t, _, (want_r2, want_w) = twin_lin(n, kind, perturb, k)
            g = device_graph(spec)
            try:
                r2, w = g.factorErrors()
                assert r2.dtype == np.float64 and w.dtype == np.float64 and r2.shape == w.shape == (len(t.factors),)
                assert each_rel(r2, want_r2) <= BAR_LIN and each_rel(w, want_w) <= BAR_LIN, (perturb, k, each_rel(r2, want_r2), each_rel(w, want_w))
                plain = np.array([x is None for x in t.k])
                assert np.all(w[plain] == 1.0) and np.all(w[~plain] < 1.0) and (~plain).sum() == 1
                again = g.factorErrors()
                assert same_bits((r2, w), again)
            finally:
                g.close()


def test_factor_errors_follow_the_poses_and_respect_cap():
    spec = rt.outlier_spec(65)
    g = device_graph(spec)
    try:
        F = g.size()[1]
        before = g.factorErrors()
        t = rt.build(spec)
        assert rel(before[0], t.factor_errors()[0]) <= BAR_LIN and rel(before[1], t.factor_errors()[1]) <= BAR_LIN
        assert g.optimize()["iterations"] >= 1
        r2, w = g.factorErrors()
        t.poses = [tw.X_of(T) for T in g.poses()]      # the twin's figures at the device's new poses
        want_r2, want_w = t.factor_errors()
        assert rel(r2, want_r2) <= BAR_LIN and rel(w, want_w) <= BAR_LIN
        chain = slice(1, 65)      # and not those of the poses before: the chain started at its own measurements and has given way to the loops
        assert before[0][chain].max() < 1e-20 and r2[chain].max() > 1e-5 and not np.array_equal(w, before[1])
        # cap below F: only cap entries are written, F is still returned; each output is optional
        L, dp = lib(), C.POINTER(C.c_double)
        for cap in (0, 1, F - 1):
            a, b = np.full(F, -7.0), np.full(F, -7.0)
            assert L.rolo_pgo_get_factor_errors(g._h, a.ctypes.data_as(dp), b.ctypes.data_as(dp), cap) == F
            assert np.array_equal(a[:cap], r2[:cap]) and np.array_equal(b[:cap], w[:cap]) and np.all(a[cap:] == -7.0) and np.all(b[cap:] == -7.0)
        a, b = np.full(F, -7.0), np.full(F, -7.0)
        assert L.rolo_pgo_get_factor_errors(g._h, a.ctypes.data_as(dp), None, F) == F and np.array_equal(a, r2)
        assert L.rolo_pgo_get_factor_errors(g._h, None, b.ctypes.data_as(dp), F) == F and np.array_equal(b, w)
        assert L.rolo_pgo_get_factor_errors(g._h, None, None, F) == F
        assert L.rolo_pgo_get_factor_errors(g._h, a.ctypes.data_as(dp), b.ctypes.data_as(dp), -1) == EINVAL
    finally:
        g.close()


# ---- 2. whole optimisations of the outlier graphs --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin_whole():
    cache = {}

    def get(n, name):
        if (n, name) not in cache:
            t = rt.build(rt.outlier_spec(n))
            cache[n, name] = (t.optimize("direct", **tw.STRICT) if name == "strict" else t.optimize("pcg"), t.poses)
        return cache[n, name]
    return get


def check_weights(spec, w):
    loops = spec["true_loops"] + spec["false_loops"]
    assert np.all(w[spec["false_loops"]] <= 1e-3), w[spec["false_loops"]]
    assert np.all(w[spec["true_loops"]] >= 0.1), w[spec["true_loops"]]
    assert np.all(np.delete(w, loops) == 1.0)


@pytest.mark.parametrize("n", rt.OUTLIER_SIZES)
def test_whole_optimisation_against_the_twin(twin_whole, n):
    spec = rt.outlier_spec(n)
    want, _ = twin_whole(n, "default")
    g = device_graph(spec)
    try:
        r = g.optimize()
        tr = g.trace()
        print(f"N = {n}, defaults: {(r['state'], r['iterations'], r['trials'])} / {(want['state'], want['iterations'], want['trials'])}, cost {r['final_cost']!r} / "
              f"{want['final_cost']!r}, weights of the loops {g.factorErrors()[1][spec['true_loops'] + spec['false_loops']]}")
        assert (r["state"], r["iterations"], r["trials"]) == (want["state"], want["iterations"], want["trials"])
        assert [x["accepted"] for x in tr] == [bool(x[2]) for x in want["trace"]] and np.allclose([x["lambda_"] for x in tr], [x[0] for x in want["trace"]], rtol=1e-12)
        assert abs(r["final_cost"] - want["final_cost"]) <= 1e-9 * want["final_cost"]
        check_weights(spec, g.factorErrors()[1])
        g.close()
        want, want_poses = twin_whole(n, "strict")
        g = device_graph(spec)
        r = g.optimize(pgo_params(**tw.STRICT))
        dt, dr = tw.pose_distance(list(g.poses()), want_poses)
        print(f"N = {n}, STRICT: state {r['state']} / {want['state']}, cost {r['final_cost']!r} / {want['final_cost']!r}, poses {dt:.3e} m {dr:.3e} rad")
        bm, br = bars(TWIN_ROBUST_WHOLE[n])
        assert dt <= bm and dr <= br
        assert abs(r["final_cost"] - want["final_cost"]) <= 1e-9 * want["final_cost"]
        check_weights(spec, g.factorErrors()[1])
    finally:
        g.close()


def test_two_runs_give_the_same_bits():
    spec = rt.outlier_spec(120)
    out = []
    for _ in range(2):
        g = device_graph(spec)
        try:
            r = g.optimize()
            out.append((g.poses().tobytes(), r["final_cost"], r["pcg_iterations"], [x["cost"] for x in g.trace()], g.factorErrors()[0].tobytes(), g.factorErrors()[1].tobytes()))
        finally:
            g.close()
    assert out[0] == out[1]


def test_a_huge_k_is_the_plain_factor():
    """k = 1e9: w = 1 and rho = r^2 / 2 to rounding; the same device graph built from plain addBetween agrees in the linearisation and at the optimum"""
    lin_spec = rt.robust_case_spec(65, "pair2", PERTURBS[1], 1e9)
    whole_spec = rt.outlier_spec(65, k=1e9, outliers=False)
    a, b = device_graph(lin_spec), device_graph(lin_spec, plain=True)
    c, d = device_graph(whole_spec), device_graph(whole_spec, plain=True)
    try:
        la, lb = a.linearize(), b.linearize()
        assert rel(la[0], lb[0]) <= BAR_LIN and rel(la[1], lb[1]) <= BAR_LIN
        for x, y in zip(la[2:5], lb[2:5]):
            assert max([rel(p, q) for p, q in zip(x, y)], default=0.0) <= BAR_LIN
        assert np.array_equal(la[5], lb[5])
        assert each_rel(a.factorErrors()[0], b.factorErrors()[0]) <= BAR_LIN and each_rel(a.factorErrors()[1], b.factorErrors()[1]) <= BAR_LIN
        assert np.all(b.factorErrors()[1] == 1.0)
        rc, rd = c.optimize(), d.optimize()
        assert (rc["state"], rc["iterations"], rc["trials"]) == (rd["state"], rd["iterations"], rd["trials"]) and rc["iterations"] >= 1
        assert abs(rc["final_cost"] - rd["final_cost"]) <= 1e-9 * rd["final_cost"]
        dt, dr = tw.pose_distance(list(c.poses()), list(d.poses()))
        print(f"k = 1e9 against plain factors at the optimum: {dt:.3e} m {dr:.3e} rad")
        assert dt <= 1e-9 and dr <= 1e-10
    finally:
        for g in (a, b, c, d):
            g.close()


# ---- 3. errors -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_errors():
    L = lib()
    dp = C.POINTER(C.c_double)
    eye = np.eye(4).reshape(16)
    ok = np.full(6, 1e-2)
    ptr = lambda a: a.ctypes.data_as(dp)
    g = PoseGraph()
    try:
        a = np.zeros(4)
        assert L.rolo_pgo_get_factor_errors(g._h, ptr(a), ptr(a), 4) == ESTATE      # no pose
        with pytest.raises(RoloError) as e:
            g.factorErrors()
        assert e.value.code == ESTATE
        assert g.addPose(eye) == 0 and g.addPose(eye) == 1
        assert L.rolo_pgo_get_factor_errors(g._h, ptr(a), ptr(a), 4) == ESTATE      # no factor
        add = L.rolo_pgo_add_between_robust
        for k in (0.0, -1.0, np.nan, np.inf, -np.inf):
            assert add(g._h, 0, 1, ptr(eye), ptr(ok), CAUCHY, k) == EINVAL
            with pytest.raises(RoloError) as e:
                g.addBetween(0, 1, eye, ok, cauchy=k)
            assert e.value.code == EINVAL
        for loss in (0, 2):
            assert add(g._h, 0, 1, ptr(eye), ptr(ok), loss, 1.0) == EUNSUPPORTED
        assert add(g._h, 1, 1, ptr(eye), ptr(ok), CAUCHY, 1.0) == EINVAL
        for i in (-1, 2):
            assert add(g._h, i, 0, ptr(eye), ptr(ok), CAUCHY, 1.0) == EINVAL and add(g._h, 0, i, ptr(eye), ptr(ok), CAUCHY, 1.0) == EINVAL
        for v in (0.0, -1.0, np.inf, np.nan):
            var = ok.copy(); var[4] = v
            assert add(g._h, 0, 1, ptr(eye), ptr(var), CAUCHY, 1.0) == EINVAL
        bad_T = eye.copy(); bad_T[3] = np.nan
        assert add(g._h, 0, 1, ptr(bad_T), ptr(ok), CAUCHY, 1.0) == EINVAL
        assert add(g._h, 0, 1, None, ptr(ok), CAUCHY, 1.0) == EINVAL and add(g._h, 0, 1, ptr(eye), None, CAUCHY, 1.0) == EINVAL
        assert g.size() == (2, 0, 0)      # every refused call left the graph as it was
        g.addPrior(0, eye, ok)
        g.addBetween(1, 0, eye, ok, cauchy=1.0)
        assert g.size() == (2, 2, 0)
        assert add(g._h, 0, 1, ptr(eye), ptr(ok), 2, 1.0) == EUNSUPPORTED and add(g._h, 0, 1, ptr(eye), ptr(ok), CAUCHY, 0.0) == EINVAL and g.size() == (2, 2, 0)
        r2, w = g.factorErrors()
        assert not np.any(r2) and np.all(w == 1.0)      # r^2 = 0: w = 1, rho = 0
        assert g.linearize()[0] == 0.0 and g.optimize()["state"] == tw.CONVERGED
    finally:
        g.close()


# ---- 4. from LoopCloser's result into the graph ------------------------------------------------------------------------------------------------------------------------
def loop_entries():
    spec = tw.case_spec(5, "none")
    pose_from = tw.T_of(spec["truth"][4]) @ tw.T_of(tw.exp_se3(np.array([0.01, -0.02, 0.03, 0.2, -0.1, 0.05])))
    return spec, (4, 0, pose_from, tw.T_of(spec["truth"][0]), np.float32(0.25))


@pytest.mark.parametrize("robust", [1.0, 0.5, None, "tuple"])
def test_add_loop_factor_reads_the_loss(robust):
    spec, entries = loop_entries()
    a, b = device_graph(spec), device_graph(spec)
    try:
        loop = entries if robust == "tuple" else LoopFactor(entries, robust=robust)
        assert len(loop) == 5
        cur, pre, pose_from, pose_to, noise = loop      # it unpacks into the five entries
        assert (cur, pre) == (4, 0) and noise == entries[4]
        a.addLoopFactor(loop)
        k = None if robust == "tuple" else robust
        assert getattr(loop, "robust", None) == k
        b.addBetween(4, 0, np.linalg.inv(pose_from) @ pose_to, np.full(6, float(noise)), cauchy=k)
        assert a.size() == b.size() == (5, 6, 1)
        assert same_bits(a.linearize(), b.linearize()) and same_bits(a.factorErrors(), b.factorErrors())
        w = a.factorErrors()[1]
        assert (w[-1] < 1.0) if k is not None else (w[-1] == 1.0)
        if k is None:      # and the plain call as it has always been made
            c = device_graph(spec)
            try:
                check = lib().rolo_pgo_add_between
                Z = np.ascontiguousarray(np.linalg.inv(pose_from) @ pose_to).reshape(16); v = np.full(6, float(noise))
                assert check(c._h, 4, 0, Z.ctypes.data_as(C.POINTER(C.c_double)), v.ctypes.data_as(C.POINTER(C.c_double))) == 0
                assert same_bits(a.linearize(), c.linearize())
            finally:
                c.close()
    finally:
        a.close(); b.close()


class StubScanContext:
    def __init__(self, loop_id):
        self.loop_id = loop_id

    def detectLoopClosureID(self):
        return self.loop_id, np.float32(0.1)


def test_loop_closer_marks_the_sc_loop_robust_and_the_rs_loop_plain():
    """performSCLoopClosure's factor is Robust(Cauchy(1), ...) (:2468-2470), performRSLoopClosure's the plain diagonal (:2382-2385); ICP and Scan Context are
    stubbed: their own tests run them"""
    rng = np.random.default_rng(7)
    km = KeyFrameMap()
    try:
        for k, (x, tm) in enumerate(((0.0, 0.0), (5.0, 1.0), (10.0, 2.0), (1.0, 50.0))):
            pts = np.concatenate([rng.normal(size=(12, 3)), np.zeros((12, 1))], axis=1).astype(np.float32)
            assert km.addKeyFrame(pts[:4], pts, np.array([0, 0, 0, x, 0, 0], np.float32), tm) == k
        lc = LoopCloser(km)
        T = np.eye(4, dtype=np.float32); T[0, 3] = 0.5
        lc._align = lambda cur, pre, wrt_key, cap, guess=None: dict(T=T, fitness=0.125, converged=True)
        sc = lc.performSCLoopClosure(StubScanContext(1))
        assert isinstance(sc, LoopFactor) and isinstance(sc, tuple) and len(sc) == 5 and sc.robust == 1.0
        cur, pre, pose_from, pose_to, noise = sc
        assert (cur, pre) == (3, 1) and np.array_equal(pose_from, T.astype(np.float64)) and np.array_equal(pose_to, np.eye(4)) and noise == np.float32(0.125)
        assert lc.performSCLoopClosure(StubScanContext(-1)) is None
        lc = LoopCloser(km)
        lc._align = lambda cur, pre, wrt_key, cap, guess=None: dict(T=T, fitness=0.125, converged=True)
        rs = lc.performRSLoopClosure(50.0)
        assert isinstance(rs, LoopFactor) and len(rs) == 5 and rs.robust is None
        assert rs[:2] == (3, 0) and rs[4] == np.float32(0.125)
        # both into a graph: the SC loop is down-weighted where it disagrees, the RS loop is not
        g = PoseGraph()
        try:
            for p in km.poses:
                g.addOdomFactor(p)
            g.addLoopFactor(sc); g.addLoopFactor(rs)
            r2, w = g.factorErrors()
            assert g.size() == (4, 6, 2) and r2[4] > 0 and w[4] == 1.0 / (1.0 + r2[4]) and w[5] == 1.0
        finally:
            g.close()
    finally:
        km.close()
