"""GPU: the two forms of the pose graph's linear solve (rolo_amd/csrc/posegraph.hip) return the same bits. "one" is pgo_solve_kernel, the factorisation and the
whole PCG loop in one workgroup; "grid" is the pgo_grid_* kernels, the same per-element bodies cut into one launch per seam, PCG's scalars and its exit in
device memory, the host looking at a pinned word once per batch of iterations. Every comparison of form against form is of bytes, with no tolerance.

The sizes are the grid form's own seams. Its constants (posegraph.hip; restated here because a test cannot read them):
  PGO_GRID_TOP   = 256   a level of at most 256 blocks is finished, with all levels above it, by one workgroup: up to N = 256 no level has a launch of its own
  PGO_GRID_TILE  = 32    one workgroup of a level's launch makes 32 blocks of the next level from 64 of its own: its share of level 0 is 64 poses
  PGO_GRID_BATCH = 4     PCG iterations enqueued between two looks at the done word
  PGO_GRID_FROM  = 512   the pose count from which AUTO takes the grid form
At the largest sizes, where the one-workgroup form itself was never checked, both forms are also held to the statement's direct solve on the host."""
import numpy as np
import pytest

import pgo_twin as tw
from rolo_amd._lib import RoloError
from rolo_amd.backend import PoseGraph, pgo_params
from test_gpu_posegraph import device_graph, rel

pytestmark = pytest.mark.gpu

TOP, SHARE, BATCH, GRID_FROM = 256, 64, 4, 512
FORMS = ("one", "grid")

SEAMS = (
    (1, "L = 0: the top block alone, no level at all"),
    (2, "L = 1"),
    (3, "L = 2, one block of padding"),
    (5, "L = 3"),
    (SHARE - 1, "one share of level 0 less one pose (inside the fused top)"),
    (SHARE, "one share"),
    (SHARE + 1, "one share and one pose"),
    (2 * SHARE + 1, "two shares and one pose"),
    (TOP, "the largest N the fused top finishes alone: M = 256, no level launch"),
    (TOP + 1, "the smallest N with a level launch: M = 512, level 0 over 8 workgroups, all but one pose of the second half padding"),
    (TOP + SHARE - 1, "level 0 in launches: the graph ends one pose before the edge of workgroup 4's share"),
    (TOP + SHARE, "the graph ends on that edge: workgroup 5 reads its left halo from the graph and owns padding only"),
    (TOP + SHARE + 1, "one pose past the edge"),
    (TOP + 2 * SHARE + 1, "two shares past the top and one pose"),
    (1025, "M = 2048: three levels in launches, more identity padding than graph"),
    (2051, "M = 4096, an odd tail: the last pose is an even block whose right neighbour is padding"),
    (4097, "M = 8192: five levels in launches, 128 workgroups on level 0"),
)
CASES = [(n, k) for n, _ in SEAMS for k in tw.KINDS if n >= tw.MIN_N[k]]


def solve_under(g, form, *a, **kw):
    g.setSolveForm(form)
    out = g.solveLinear(*a, **kw)
    assert g.solveForm() == (form, form)
    return out


def same_solve(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and np.float64(a[2]).tobytes() == np.float64(b[2]).tobytes()


# ---- 1. bits, form against form, at the seams ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", CASES)
def test_both_forms_return_the_same_bits(n, kind):
    g = device_graph(tw.case_spec(n, kind))
    try:
        g.linearize()
        for lam in (0.0, 1e-5):
            one = solve_under(g, "one", lam)
            grid = solve_under(g, "grid", lam)
            assert np.all(np.isfinite(one[0])) and np.any(one[0])
            assert same_solve(one, grid), (lam, one[1:], grid[1:], rel(grid[0], one[0]))
    finally:
        g.close()


# ---- 2. the limit, and an independent answer there ------------------------------------------------------------------------------------------------------------------
def ring(N, seed):
    """tw.circuit's shape without its loop over poses: N poses on a circle driven twice, an exact odometry chain from the true poses, every initial pose moved off
    it (yaw and position) so that no residual is trivial, a prior on pose 0 and two chords measured from the true poses. -> initial (N x 4 x 4), odometry
    ((N - 1) x 4 x 4), [(i, j, Z)]"""
    rng = np.random.default_rng(seed)

    def Tz(yaw, x, y, z):
        T = np.zeros((len(yaw), 4, 4))
        T[:, 0, 0] = np.cos(yaw); T[:, 0, 1] = -np.sin(yaw); T[:, 1, 0] = np.sin(yaw); T[:, 1, 1] = np.cos(yaw); T[:, 2, 2] = 1.0; T[:, 3, 3] = 1.0
        T[:, 0, 3] = x; T[:, 1, 3] = y; T[:, 2, 3] = z
        return T
    a = 4.0 * np.pi * np.arange(N) / N
    truth = Tz(a + 0.5 * np.pi, 20.0 * np.cos(a), 20.0 * np.sin(a), 0.5 * np.sin(a))
    odo = np.linalg.inv(truth[:-1]) @ truth[1:]
    initial = truth @ Tz(rng.normal(0, 1e-2, N), rng.normal(0, 5e-2, N), rng.normal(0, 5e-2, N), rng.normal(0, 5e-2, N))
    chords = [(i, j, np.linalg.inv(truth[i]) @ truth[j]) for i, j in ((N - 1, 0), (N // 2 + 1, 1))]
    return initial, odo, chords


def ring_graph(N, seed=None, prior=True, chords=True):
    initial, odo, ch = ring(N, N if seed is None else seed)
    g = PoseGraph()
    try:
        for T in initial:
            g.addPose(T)
        if prior:
            g.addPrior(0, initial[0], np.full(6, 1e-4))
        ov = np.array(tw.ODOM_VARIANCES)
        for k in range(N - 1):
            g.addBetween(k, k + 1, odo[k], ov)
        for i, j, Z in (ch if chords else ()):
            g.addBetween(i, j, Z, np.full(6, 0.3))
    except Exception:
        g.close()
        raise
    return g


@pytest.mark.parametrize("n", [32769, 65536])
def test_both_forms_return_the_same_bits_at_the_pose_limit(n):
    """32 769: half of M = 65 536 is identity padding; 65 536 = ROLO_PGO_MAX_POSES: none is. Two chords: the cap is 26 iterations"""
    g = ring_graph(n)
    try:
        assert g.size() == (n, n + 2, 2)
        g.linearize()
        for lam in (0.0, 1e-5):
            one = solve_under(g, "one", lam)
            grid = solve_under(g, "grid", lam)
            print(f"N = {n} lambda = {lam}: {one[1]} iterations, residual {one[2]:.2e}")
            assert np.all(np.isfinite(one[0])) and np.any(one[0]) and 1 <= one[1] <= 26
            assert same_solve(one, grid), (lam, one[1:], grid[1:], rel(grid[0], one[0]))
    finally:
        g.close()


@pytest.mark.parametrize("n", [16385, 65536])
def test_both_forms_against_the_statements_direct_solve_at_large_sizes(n):
    """the device's own linearisation, solved by the statement's two routes on the host (sparse direct; PCG with an exact block-tridiagonal solve): what they
    differ by, times ten and never below 1e-9, is the bar for the device's step (the rule of BAR_STEP in tests/test_gpu_posegraph.py)"""
    lam = 1e-5
    g = ring_graph(n)
    try:
        lin = g.linearize()
        d_direct = tw.Graph.solve_direct(lin, lam)
        d_pcg = tw.Graph.solve_pcg(lin, lam)[0]
        bar = max(10.0 * rel(d_pcg, d_direct), 1e-9)
        for form in FORMS:
            d, its, res = solve_under(g, form, lam)
            print(f"N = {n} {form}: {its} iterations, residual {res:.2e}; the device against the direct solve {rel(d, d_direct):.3e}, "
                  f"the statement's PCG against it {rel(d_pcg, d_direct):.3e}")
            assert rel(d, d_direct) <= bar, (form, rel(d, d_direct), bar)
    finally:
        g.close()


# ---- 3. exits and the batch boundary ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def looped():
    """300 poses (one level in launches) and 6 loops: a graph whose solve needs more than BATCH + 1 iterations"""
    g = device_graph(tw.circuit(300, 6, seed=300))
    try:
        g.linearize()
        yield g
    finally:
        g.close()


def test_the_cap_on_each_side_of_a_read_back(looped):
    natural = solve_under(looped, "one", 1e-5)[1]
    assert natural > BATCH + 1, natural
    for cap in (BATCH - 1, BATCH, BATCH + 1, 2 * BATCH, 2 * BATCH + 1):
        one = solve_under(looped, "one", 1e-5, pcg_max=cap)
        grid = solve_under(looped, "grid", 1e-5, pcg_max=cap)
        assert one[1] == cap and one[2] > 1e-10, (cap, one[1:])     # ended by the cap, not by the tolerance
        assert same_solve(one, grid), (cap, one[1:], grid[1:])


def test_a_natural_exit_in_the_first_batch_and_in_a_later_one(looped):
    seen = []
    for tol in (0.5, 1e-1, 1e-2, 1e-4, 1e-7, 1e-10):
        one = solve_under(looped, "one", 1e-5, pcg_tol=tol)
        grid = solve_under(looped, "grid", 1e-5, pcg_tol=tol)
        assert one[2] <= tol, (tol, one[1:])     # ended by the tolerance
        assert same_solve(one, grid), (tol, one[1:], grid[1:])
        seen.append(one[1])
    print("iterations by tolerance:", seen)
    assert 1 <= seen[0] <= BATCH < seen[-1], seen     # the loosest leaves in the first batch, the tightest in a later one


@pytest.mark.parametrize("n", [5, 300])
def test_a_zero_gradient_returns_zero_in_both_forms(n):
    g = device_graph(tw.exact_chain(n))
    try:
        cost, grad = g.linearize()[:2]
        assert cost == 0.0 and not np.any(grad)
        for form in FORMS:
            d, its, res = solve_under(g, form, 1e-5)
            assert its == 0 and res == 0.0 and not np.any(d) and np.all(np.isfinite(d))
    finally:
        g.close()


@pytest.mark.parametrize("n", [5, 300])
def test_without_chords_one_iteration_is_the_solve(n):
    g = device_graph(tw.case_spec(n, "none"))
    try:
        g.linearize()
        one, grid = solve_under(g, "one", 1e-5), solve_under(g, "grid", 1e-5)
        assert one[1] == 1 and same_solve(one, grid), (one[1:], grid[1:])
    finally:
        g.close()


@pytest.mark.parametrize("n", [5, 300])
def test_not_positive_definite_is_the_same_error_in_both_forms(n):
    """lambda = 0 on a graph without a prior. Its last pose is one that no factor touches: that pose's block of H is exactly zero, so the factorisation meets a
    pivot that is not positive whatever the rounding. (Without such a pose H is singular by its gauge freedom alone, its last pivots are rounding noise of
    either sign, and the flag is a matter of luck: on that graph the two forms must still agree, whichever way it falls.)"""
    spec = tw.case_spec(n, "one")
    spec["priors"] = []
    gauge_only = device_graph(spec)
    spec["betweens"] = [f for f in spec["betweens"] if n - 1 not in f[:2]]
    g = device_graph(spec)

    def outcome(h, form, lam):
        h.setSolveForm(form)
        try:
            d, its, res = h.solveLinear(lam)
        except RoloError as e:
            assert e.code == -1
            out = str(e)
        else:
            out = (d.tobytes(), its, np.float64(res).tobytes())
        assert h.solveForm() == (form, form)
        return out
    try:
        assert g.size() == (n, n - 2, 0)
        g.linearize()
        said = [outcome(g, form, 0.0) for form in FORMS]
        assert said[0] == said[1] and isinstance(said[0], str) and "not positive definite" in said[0], said
        assert same_solve(solve_under(g, "one", 1e-5), solve_under(g, "grid", 1e-5))     # and the graph still solves under damping
        gauge_only.linearize()
        assert outcome(gauge_only, "one", 0.0) == outcome(gauge_only, "grid", 0.0)
    finally:
        g.close(); gauge_only.close()


# ---- 4. whole optimisations, a graph that changes form mid-life, run to run ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", ["defaults", "strict"])
@pytest.mark.parametrize("n,loops", [(200, 8), (2500, 30)])
def test_whole_optimisations_agree_in_every_trial(n, loops, params):
    spec = tw.circuit(n, loops, seed=n)
    got = []
    for form in FORMS:
        g = device_graph(spec)
        try:
            g.setSolveForm(form)
            r = g.optimize(pgo_params(**tw.STRICT) if params == "strict" else None)
            assert g.solveForm() == (form, form)
            got.append((r, g.trace(), g.poses().tobytes()))
        finally:
            g.close()
    assert got[0][0]["iterations"] >= 1 and got[0][0]["pcg_iterations"] > got[0][0]["trials"]
    assert got[0][0] == got[1][0] and got[0][1] == got[1][1] and got[0][2] == got[1][2]


def test_a_graph_that_changes_form_at_every_step():
    """120 key poses fed as the back end feeds them, an optimise after each; one graph alternates between the forms, the other stays with one workgroup"""
    ref = tw.reference_spec()
    a, b = PoseGraph(), PoseGraph()
    try:
        b.setSolveForm("one")
        moved = 0
        for k, p in enumerate(ref["poses6"]):
            a.setSolveForm(FORMS[k % 2])
            for g in (a, b):
                g.addOdomFactor(p)
                for loop in ref["loops"]:
                    if loop[0] == k:
                        g.addLoopFactor(loop)
            ra, rb = a.optimize(), b.optimize()
            assert a.solveForm() == (FORMS[k % 2], FORMS[k % 2]) and b.solveForm() == ("one", "one")
            assert ra == rb and a.trace() == b.trace() and a.poses().tobytes() == b.poses().tobytes(), k
            moved += ra["iterations"]
        assert a.size() == b.size() == (120, 120 + len(ref["loops"]), len(ref["loops"])) and moved >= 1
    finally:
        a.close(); b.close()


def test_the_grid_form_returns_the_same_bits_on_every_run(looped):
    first = solve_under(looped, "grid", 1e-5)
    assert same_solve(first, solve_under(looped, "grid", 1e-5))


# ---- 5. the interface ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_form_is_set_and_read_per_graph():
    g, h = device_graph(tw.case_spec(5, "one")), PoseGraph()
    try:
        assert g.solveForm() == ("auto", None)
        g.linearize()
        assert g.solveForm() == ("auto", None)     # a linearisation is no solve
        g.setSolveForm("grid")
        assert g.solveForm() == ("grid", None) and h.solveForm() == ("auto", None)
        for bad in ("", "GRID", "both", 2):
            with pytest.raises(RoloError):
                g.setSolveForm(bad)
            assert g.solveForm() == ("grid", None)
        g.solveLinear(1e-5)
        assert g.solveForm() == ("grid", "grid")
        g.setSolveForm("auto")
        assert g.solveForm() == ("auto", "grid")
        g.solveLinear(1e-5)
        assert g.solveForm() == ("auto", "one")
    finally:
        g.close(); h.close()


@pytest.mark.parametrize("n,form", [(GRID_FROM - 1, "one"), (GRID_FROM, "grid")])
def test_auto_takes_the_grid_form_from_its_constant_on(n, form):
    g = ring_graph(n)
    try:
        g.linearize()
        auto = g.solveLinear(1e-5)
        assert g.solveForm() == ("auto", form)
        r = g.optimize()
        assert g.solveForm() == ("auto", form) and r["trials"] >= 1
        g.linearize()
        assert same_solve(solve_under(g, "one", 1e-5), solve_under(g, "grid", 1e-5))
        assert np.all(np.isfinite(auto[0]))
    finally:
        g.close()
