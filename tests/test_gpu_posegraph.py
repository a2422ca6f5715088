"""GPU: the pose-graph optimisation on the device (rolo_amd/csrc/posegraph.hip, rolo_pgo_* and rolo_keymap_set_poses) against the numpy statement
tests/pgo_twin.py: the linearisation block by block, the linear step against the twin's direct solve, whole optimisations against the twin's optimum, the
reference's own prior and noise models through addOdomFactor / addLoopFactor on gauge-free quantities, truth, every exit, every error, the key map, and the
every-key-frame use without loops.

Bars. Blocks, gradient and cost: 1e-9 relative to the block's (vector's) largest magnitude, the bar the project holds H, b, err to. The step and the poses:
10 x what the twin's two entry points (sparse direct solve; PCG with an exact block-tridiagonal solve) differ by on the same graphs, measured on the CPU by
tests/test_pgo_twin.py, which asserts the figures below still hold; never tighter than 1e-9 (step), 1e-9 m / 1e-10 rad (poses). The factor 10 covers a
different summation order in the dot products and the cyclic reduction's rounding, which the twin's exact solve does not have."""
import ctypes as C

import numpy as np
import pytest

import pgo_twin as tw
from rolo_amd._lib import RoloError, lib
from rolo_amd.backend import KeyFrameMap, LoopCloser, PoseGraph, pgo_params, pose6_to_T

pytestmark = pytest.mark.gpu

# measured by tests/test_pgo_twin.py (numpy 2 / scipy, fp64), printed there with `pytest -s`:
TWIN_STEP = 5.2e-8            # test_pcg_against_the_direct_solve_on_the_test_graphs: largest relative difference of the step over tw.CASES x lambda in {0, 1e-5}
                              # (5.17e-8 at N = 1000 with the chord (k, k+2); every N <= 65 is below 6.3e-9). Over tw.CASES_LARGE it is 4.42e-8, at N = 4097
                              # with the chord (k, k+2) (7.9e-9 at 1024, 3.2e-8 at 1025, 8.5e-9 at 2049, 6.9e-9 at 2051): the sizes past 1 024 poses add nothing to the figure
# test_entry_points_agree_on_whole_optimisations: (m, rad) at the optimum, by the number of poses
TWIN_WHOLE = {65: (5.4e-14, 2.6e-16), 200: (5.3e-9, 2.7e-10), 1000: (4.6e-11, 1.5e-12), 2500: (5.7e-11, 2.8e-12)}
TWIN_REFERENCE = (4.9e-14, 3.8e-16)                                                       # test_entry_points_agree_under_the_reference_prior: relative poses (m, rad)
# test_one_gauss_newton_step_lands_on_the_zero_error_poses: (m, rad) from the zero-error poses after the statement's own step on the graphs of tests/se3_cases.py,
# the worst over its angles up to pi - 1e-3 and its axes. One pose, and two poses under Cauchy: at pi - 1e-3, and under 2.4e-14 m / 1.9e-15 rad up to pi - 0.1; the
# plain between factor, whose two poses share the step: 1e-12 .. 3.5e-12 m at every angle but 0
TWIN_RETRACT = {"prior": (2.1e-12, 1.3e-13), "between": (3.6e-12, 3.5e-13), "cauchy1": (2.1e-12, 1.3e-13), "cauchy0.1": (2.1e-12, 1.3e-13)}
# test_the_grown_graph_reaches_the_optimum_of_the_whole: (m, rad) between the statement grown step by step as tests/test_gpu_posegraph_life.py grows the device's
# graph (PCG, then STRICT) and its direct solve on the whole graph from the composed odometry (the two entry points on the whole graph: 4.7e-9 m, 1.5e-10 rad)
TWIN_LIFE = (1.7e-8, 5.6e-10)

BAR_LIN = 1e-9
BAR_STEP = max(10.0 * TWIN_STEP, 1e-9)
EINVAL, ESTATE = -1, -5


def bars(rec):
    return max(10.0 * rec[0], 1e-9), max(10.0 * rec[1], 1e-10)


def device_graph(spec):
    g = PoseGraph()
    for X in spec["initial"]:
        g.addPose(tw.T_of(X))
    for i, T, v in spec["priors"]:
        g.addPrior(i, T, v)
    for i, j, T, v in spec["betweens"]:
        g.addBetween(i, j, T, v)
    return g


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / np.abs(b).max()) if a.size and np.abs(b).max() > 0 else float(np.abs(a).max()) if a.size else 0.0


# ---- 1. linearisation and the linear step ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin_lin():
    cache = {}

    def get(n, kind):
        if (n, kind) not in cache:
            spec = tw.case_spec(n, kind)
            t = tw.build(spec)
            cache[n, kind] = (spec, t, t.linearize())
        return cache[n, kind]
    return get


@pytest.mark.parametrize("n,kind", tw.CASES + tw.CASES_LARGE)
def test_linearisation_and_step(twin_lin, n, kind):
    spec, t, lin = twin_lin(n, kind)
    g = device_graph(spec)
    try:
        assert g.size() == (n, len(t.factors), len(t.chords()))
        if kind == "chain2":
            assert g.size()[2] == 0      # the second factor of a chain pair lands in the chain block
        got = g.linearize()
        names = ("cost", "gradient", "diagonal", "chain", "chord")
        assert rel(got[0], lin[0]) <= BAR_LIN and rel(got[1], lin[1]) <= BAR_LIN, (rel(got[0], lin[0]), rel(got[1], lin[1]))
        for name, a, b in zip(names[2:], got[2:5], lin[2:5]):
            assert a.shape == b.shape, name
            worst = max([rel(x, y) for x, y in zip(a, b)], default=0.0)     # block by block
            assert worst <= BAR_LIN, (name, worst)
        assert np.array_equal(got[5], lin[5])
        again = g.linearize()
        assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(got, again))     # the same bits on every run
        for lam in (0.0, 1e-5):
            d, its, res = g.solveLinear(lam)
            want = tw.Graph.solve_direct(lin, lam)
            assert np.all(np.isfinite(d)) and np.isfinite(res)
            if len(t.chords()) == 0:
                assert its == 1
            else:
                assert 1 <= its <= 12 * len(t.chords()) + 2
            print(f"N = {n} {kind} lambda = {lam}: {its} iterations, residual {res:.2e}, step against the twin's direct solve {rel(d, want):.2e}")
            assert rel(d, want) <= BAR_STEP
            d2, its2, res2 = g.solveLinear(lam)
            assert d2.tobytes() == d.tobytes() and (its2, res2) == (its, res)
    finally:
        g.close()


@pytest.mark.parametrize("n", tw.SIZES)
def test_zero_gradient_returns_zero_at_once(n):
    """a chain composed from its own measurements, in numbers whose products are exact: r0 z0 == 0, and nothing is divided by it"""
    g = device_graph(tw.exact_chain(n))
    try:
        cost, grad = g.linearize()[:2]
        assert cost == 0.0 and not np.any(grad)
        for lam in (0.0, 1e-5):
            d, its, res = g.solveLinear(lam)
            assert its == 0 and res == 0.0 and not np.any(d) and np.all(np.isfinite(d))
        r = g.optimize()
        assert (r["state"], r["iterations"], r["trials"], r["final_cost"]) == (tw.CONVERGED, 0, 1, 0.0)
    finally:
        g.close()


# ---- 2. whole optimisations ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin_whole():
    cache = {}

    def get(n, loops, name):
        if (n, name) not in cache:
            t = tw.build(tw.circuit(n, loops, seed=n))
            cache[n, name] = (t.optimize("direct", **(tw.STRICT if name == "strict" else {})), t.poses)
        return cache[n, name]
    return get


@pytest.mark.parametrize("n,loops", tw.WHOLE)
def test_whole_optimisation_against_the_twin(twin_whole, n, loops):
    spec = tw.circuit(n, loops, seed=n)
    want, want_poses = twin_whole(n, loops, "strict")
    g = device_graph(spec)
    try:
        r = g.optimize(pgo_params(**tw.STRICT))
        P = g.poses()
        dt, dr = tw.pose_distance(list(P), want_poses)
        print(f"N = {n}: state {r['state']} / {want['state']}, {r['iterations']} iterations {r['trials']} trials ({want['iterations']}, {want['trials']}), "
              f"cost {r['final_cost']!r} / {want['final_cost']!r}, poses {dt:.3e} m {dr:.3e} rad, ms {g.lastMs()}")
        assert r["state"] == want["state"]
        assert abs(r["final_cost"] - want["final_cost"]) <= 1e-9 * want["final_cost"]
        bm, br = bars(TWIN_WHOLE[n])
        assert dt <= bm and dr <= br
        assert len(g.trace()) == r["trials"]
        g.close()
        # the defaults: the same state and counts (tests/test_pgo_twin.py checks that the twin's two entry points agree on them for these graphs)
        want_d, _ = twin_whole(n, loops, "default")
        g = device_graph(spec)
        r = g.optimize()
        assert (r["state"], r["iterations"], r["trials"]) == (want_d["state"], want_d["iterations"], want_d["trials"])
        assert abs(r["final_cost"] - want_d["final_cost"]) <= 1e-9 * want_d["final_cost"]
        tr = g.trace()
        assert [x["accepted"] for x in tr] == [bool(x[2]) for x in want_d["trace"]] and np.allclose([x["lambda_"] for x in tr], [x[0] for x in want_d["trace"]], rtol=1e-12)
        assert r["pcg_iterations"] == sum(x["pcg_iterations"] for x in tr) > 0 and g.lastMs().min() > 0
    finally:
        g.close()


def test_two_runs_give_the_same_bits():
    spec = tw.circuit(200, 8, seed=200)
    out = []
    for _ in range(2):
        g = device_graph(spec)
        try:
            r = g.optimize()
            out.append((g.poses().tobytes(), r["final_cost"], r["pcg_iterations"], [x["cost"] for x in g.trace()]))
        finally:
            g.close()
    assert out[0] == out[1]


def test_reference_prior_and_noise_models():
    """N = 120, 4 loops through addOdomFactor / addLoopFactor: the prior (1e-2, 1e-2, pi^2, 1e8, 1e8, 1e8) leaves translation and yaw a numerical near-gauge
    (cond(H) ~ 1e17), so only the cost, the poses relative to pose 0 and pose 0's distance from its prior are held. Both sides sit at the optimum (tolerances 0):
    with the default tolerances the damped steps spread the loops' correction over all poses and stop with pose 0 about 0.09 m off its prior (the twin does the
    same), which the prior's 1e-8 weight only undoes once lambda has fallen below it."""
    ref = tw.reference_spec()
    t = tw.build_reference(ref)
    want = t.optimize("direct", **tw.STRICT)
    g = PoseGraph()
    try:
        for k, p in enumerate(ref["poses6"]):
            assert g.addOdomFactor(p) == k
        for loop in ref["loops"]:
            g.addLoopFactor(loop)
        assert g.size() == (120, 120 + len(ref["loops"]), len(ref["loops"]))
        r = g.optimize(pgo_params(**tw.STRICT))
        P = list(g.poses())
        dt, dr = tw.pose_distance(tw.relative_to_first(P), tw.relative_to_first(t.poses))
        moved = tw.pose_distance([P[0]], [tw.pose6_to_T(ref["poses6"][0])])
        print(f"cost {r['final_cost']!r} / {want['final_cost']!r}; relative poses {dt:.3e} m {dr:.3e} rad; pose 0 moved {moved}; state {r['state']} {r['iterations']} {r['trials']}")
        assert abs(r["final_cost"] - want["final_cost"]) <= 1e-6 * want["final_cost"]
        bm, br = bars(TWIN_REFERENCE)
        assert dt <= bm and dr <= br
        assert moved[0] <= 1e-2 and moved[1] <= 1e-4
    finally:
        g.close()


def test_truth():
    """the twin at least halves the largest position error against truth on this graph (tests/test_pgo_twin.py): the device must too"""
    spec = tw.drift_spec()
    g = device_graph(spec)
    try:
        before = tw.max_position_error(list(g.poses()), spec["truth"])
        r = g.optimize()
        after = tw.max_position_error(list(g.poses()), spec["truth"])
        print("largest position error against truth:", before, "->", after)
        assert r["state"] == tw.CONVERGED and after <= 0.5 * before
    finally:
        g.close()


# ---- 3. exits, trace, errors ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw,state", [("absolute", dict(relative_error_tol=0.0), tw.CONVERGED), ("relative", dict(absolute_error_tol=0.0), tw.CONVERGED),
                                           ("cap", dict(max_iterations=1, absolute_error_tol=0.0, relative_error_tol=0.0), tw.ITERATIONS),
                                           ("lambda at once", dict(lambda_initial=1e-3, lambda_upper=1e-4), tw.LAMBDA),
                                           ("lambda at the floor", tw.STRICT, tw.LAMBDA)])
def test_every_exit(name, kw, state):
    spec = tw.circuit(65, 1, seed=65)
    t = tw.build(spec)
    want = t.optimize("pcg", **kw)
    assert want["state"] == state
    g = device_graph(spec)
    try:
        r = g.optimize(pgo_params(**kw))
        tr = g.trace()
        print(name, r, [(x["lambda_"], x["accepted"]) for x in tr])
        assert r["state"] == state and len(tr) == r["trials"] and sum(x["accepted"] for x in tr) == r["iterations"]
        lam = kw.get("lambda_initial", 1e-5)
        for x in tr:        # the lambda sequence follows the accepted flags
            assert np.isclose(x["lambda_"], lam, rtol=1e-12)
            lam = lam / 10.0 if x["accepted"] else lam * 10.0
        assert np.isclose(r["lambda_"], lam, rtol=1e-12)
        if name != "lambda at the floor":     # (at the floor the accepted flags are decided by the last bit of a cost: the sequence is each side's own)
            assert (r["iterations"], r["trials"]) == (want["iterations"], want["trials"])
            assert [x["accepted"] for x in tr] == [bool(x[2]) for x in want["trace"]] and np.allclose([x["lambda_"] for x in tr], [x[0] for x in want["trace"]], rtol=1e-12)
        if name == "lambda at once":
            assert r["trials"] == 0 and r["final_cost"] == r["initial_cost"]
    finally:
        g.close()


def test_errors():
    L = lib()
    dp = C.POINTER(C.c_double)
    eye = np.eye(4).reshape(16)
    ok = np.full(6, 1e-2)
    ptr = lambda a: a.ctypes.data_as(dp)
    g = PoseGraph()
    try:
        with pytest.raises(RoloError) as e:      # no pose
            g.optimize()
        assert e.value.code == ESTATE
        assert g.addPose(eye) == 0
        with pytest.raises(RoloError) as e:      # no factor
            g.optimize()
        assert e.value.code == ESTATE
        with pytest.raises(RoloError) as e:
            g.linearize()
        assert e.value.code == ESTATE
        assert g.addPose(eye) == 1
        bad_T = eye.copy(); bad_T[3] = np.nan
        assert L.rolo_pgo_add_pose(g._h, ptr(bad_T)) == EINVAL
        assert L.rolo_pgo_add_prior(g._h, 0, ptr(bad_T), ptr(ok)) == EINVAL
        assert L.rolo_pgo_add_between(g._h, 0, 1, ptr(bad_T), ptr(ok)) == EINVAL
        for i in (-1, 2):
            assert L.rolo_pgo_add_prior(g._h, i, ptr(eye), ptr(ok)) == EINVAL
            assert L.rolo_pgo_add_between(g._h, i, 0, ptr(eye), ptr(ok)) == EINVAL and L.rolo_pgo_add_between(g._h, 0, i, ptr(eye), ptr(ok)) == EINVAL
        assert L.rolo_pgo_add_between(g._h, 1, 1, ptr(eye), ptr(ok)) == EINVAL
        for v in (0.0, -1.0, np.inf, np.nan):
            var = ok.copy(); var[4] = v
            assert L.rolo_pgo_add_prior(g._h, 0, ptr(eye), ptr(var)) == EINVAL and L.rolo_pgo_add_between(g._h, 0, 1, ptr(eye), ptr(var)) == EINVAL
        assert g.size() == (2, 0, 0)
        g.addPrior(0, eye, ok)
        with pytest.raises(RoloError) as e:      # solve_linear before any linearisation
            g.solveLinear()
        assert e.value.code == ESTATE
        g.linearize()
        g.solveLinear(1e-5)
        g.addBetween(0, 1, eye, ok)
        with pytest.raises(RoloError) as e:      # the graph has changed since
            g.solveLinear()
        assert e.value.code == ESTATE
        assert g.optimize()["state"] == tw.CONVERGED
    finally:
        g.close()


def test_pose_limit():
    g = PoseGraph()
    try:
        T = np.eye(4).reshape(16)
        p = T.ctypes.data_as(C.POINTER(C.c_double))
        L = lib()
        for k in range(1 << 16):
            assert L.rolo_pgo_add_pose(g._h, p) == k
        assert L.rolo_pgo_add_pose(g._h, p) == EINVAL and len(g) == 1 << 16
    finally:
        g.close()


# ---- 4. the every-key-frame use ----------------------------------------------------------------------------------------------------------------------------------------
def test_zero_loop_incremental_use():
    """300 addOdomFactor + optimize calls in a row: the graph is its own odometry, every call ends converged within one iteration and moves nothing"""
    c = tw.circuit(300, 0, seed=3)
    poses6 = [tw.pose6_of(X).astype(np.float32) for X in c["initial"]]
    g = PoseGraph()
    try:
        for k, p in enumerate(poses6):
            g.addOdomFactor(p)
            r = g.optimize()
            assert r["state"] == tw.CONVERGED and r["iterations"] <= 1 and r["trials"] <= 1, (k, r)
        want = [pose6_to_T(p, np.float64) for p in poses6]
        dt, dr = tw.pose_distance(list(g.poses()), want)
        print("300 key frames without a loop: poses against the composed odometry", dt, dr)
        assert dt <= 1e-9 and dr <= 1e-9
    finally:
        g.close()


# ---- 5. with the key map -------------------------------------------------------------------------------------------------------------------------------------------
def test_loop_closure_into_the_key_map():
    """34 synthetic key frames, a lap of 30 and four more on the same places, stored with a planted drift (1 cm and 0.3 mrad of yaw per key frame):
    performRSLoopClosure -> addLoopFactor -> optimize -> correctPoses; the key map then holds the graph's pose6, and its next extraction is the one a fresh key map
    built with those poses gives, bit for bit"""
    from scipy.spatial.transform import Rotation
    from oracle import pyorc
    from rolo_amd import synth
    fo = pyorc.front_params(n_scan=16, horizon_scan=1800)

    def scene(k):
        phi = k * 2.0 * np.pi / 30.0
        return synth.rpy_to_R(0.0, 0.0, 0.01 * (k % 30)), np.array([20.0 * np.cos(phi), 12.0 * np.sin(phi), 0.0])
    R0, t0 = scene(0)
    frames = []
    for k in range(34):
        Rk, tk = scene(k)
        fr = synth.make_frame("vlp16", Rk, tk, synth.SEED + k, col_stride=4)
        e = pyorc.extract_features(fo, pyorc.project(fo, fr.xyz, fr.ring))
        rpy = Rotation.from_matrix(R0.T @ Rk).as_euler("xyz") + np.array([0.0, 0.0, 3e-4 * k])
        pose = np.concatenate([rpy, R0.T @ (tk - t0) + np.array([0.01 * k, 0.0, 0.0])]).astype(np.float32)
        frames.append((pyorc.voxelgrid(e["corner"], 0.2), pyorc.voxelgrid(e["surface"], 0.4), pose, float(k)))
    km, fresh, g = KeyFrameMap(), KeyFrameMap(), PoseGraph()
    try:
        for k, f in enumerate(frames):
            assert km.addKeyFrame(*f) == k
            g.addOdomFactor(f[2])
        lc = LoopCloser(km, historyKeyframeSearchTimeDiff=20.0, historyKeyframeSearchNum=3)
        loop = lc.performRSLoopClosure(33.0)
        assert loop is not None, lc.last
        print("loop", loop[:2], "fitness", loop[4], lc.last["state"], lc.last["iterations"])
        assert loop[0] == 33 and 0 <= loop[1] <= 6
        g.addLoopFactor(loop)
        assert g.size() == (34, 35, 1)
        r = g.optimize()
        assert r["state"] == tw.CONVERGED and r["iterations"] >= 1 and r["final_cost"] < r["initial_cost"]
        g.correctPoses(km)
        p6 = g.poses6()
        assert np.array_equal(np.array(km.poses, np.float32), p6)
        assert np.abs(p6 - np.array([f[2] for f in frames])).max() > 1e-3       # the loop moved something
        for f, p in zip(frames, p6):
            fresh.addKeyFrame(f[0], f[1], p, f[3])
        idx = np.arange(20, 34, dtype=np.int32)
        assert km.extractCloud(idx) == fresh.extractCloud(idx)
        a, b = km.submap(), fresh.submap()
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[0].shape[0] > 0
        too_many = np.zeros((35, 6), np.float32)
        assert lib().rolo_keymap_set_poses(km._h, too_many.ctypes.data_as(C.POINTER(C.c_float)), 35) == EINVAL
        assert lib().rolo_keymap_set_poses(km._h, too_many.ctypes.data_as(C.POINTER(C.c_float)), 0) == 0
    finally:
        g.close(); km.close(); fresh.close()
