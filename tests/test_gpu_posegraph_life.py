"""GPU: the pose graph grown as the back end grows it (saveKeyFramesAndFactor: one addOdomFactor, sometimes a loop factor, optimize, correctPoses, for every key
frame), which is what pgo_sync_graph's state is for: the partial uploads of the incidence rows from the first changed pose, the device buffers regrown several
times over with their contents kept or sent again, the chord tables sent again when a chord arrives, and the pose buffers swapped by every accepted trial.

One graph of 200 key poses (tests/pgo_robust_twin.py, life_script), one key pose and one optimize per step, with events on the way: loops from the newest pose,
two in one step, a loop between old poses in a step without a pose, a loop under Cauchy, a second factor in an old pose's chain block, a late prior, a loop to
pose 0 (rows sent from 0) and a factor on the pair (N - 2, N - 1) in a step without a pose (rows sent from N - 2). After every step a fresh graph is built in
one go from the grown graph's poses (doubles, exact) and the same factors in the same order: both then hold the same graph, every sum of the linearisation is
in a fixed order, and so the two must agree bit for bit, with no tolerance. The fresh graph shares the kernels: what this isolates is the host's incremental
upload and buffer state. The end is held to the statement's optimum by the rule of tests/test_gpu_posegraph.py."""
import numpy as np
import pytest

import pgo_robust_twin as rt
import pgo_twin as tw
from rolo_amd.backend import PoseGraph, pgo_params
from test_gpu_posegraph import TWIN_LIFE, bars

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return len(a) == len(b) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def fresh_graph(poses, factors):
    g = PoseGraph()
    for T in poses:
        g.addPose(T)
    for f in factors:
        if f[0] == "prior": g.addPrior(f[1], f[2], f[3])
        else: g.addBetween(f[1], f[2], f[3], f[4], cauchy=f[5])
    return g


def same_optimisation(g, h):
    ra, rb = g.optimize(), h.optimize()
    return ra == rb and g.trace() == h.trace() and g.poses().tobytes() == h.poses().tobytes()


def test_a_graph_grown_step_by_step_is_the_graph_built_at_once():
    steps, spec = rt.life_script()
    g = PoseGraph()
    factors = []
    seen = dict(iterations=0, compared=0, optimised=0)

    def add_prior(i, T, var):
        g.addPrior(i, T, var); factors.append(("prior", i, T, var))

    def add_between(i, j, T, var, k):
        g.addBetween(i, j, T, var, cauchy=k); factors.append(("between", i, j, T, var, k))

    def after_step(n, ops):
        event = n in spec["events"]
        if event:      # before this step's optimize: the upload of what the step added, by itself
            h = fresh_graph(g.poses(), factors)
            try:
                assert g.size() == h.size() and same_bits(g.linearize(), h.linearize()), ("before optimize", n)
                assert same_optimisation(g, h), ("this step's optimize", n)
            finally:
                h.close()
            assert g.last["iterations"] >= 1, n      # the event moved the graph: the pose buffers were swapped
        else:
            g.optimize()
        seen["iterations"] += g.last["iterations"]
        h = fresh_graph(g.poses(), factors)
        try:
            assert g.size() == h.size() == (len(g.poses()), len(factors), h.size()[2]), n
            assert same_bits(g.linearize(), h.linearize()), ("after optimize", n)
            seen["compared"] += 1
            if event or n % 10 == 0:
                assert same_optimisation(g, h), ("a further optimize", n)
                seen["optimised"] += 1
        finally:
            h.close()

    try:
        rt.grow_life(steps, tw.T_of(spec["initial"][0]), g.addPose, add_prior, add_between, lambda: g.poses()[-1], after_step)
        assert g.size() == (rt.LIFE_POSES, len(spec["factors"]), 6) and len(factors) == len(spec["factors"])
        assert seen["compared"] == len(steps) and seen["optimised"] == len(set(spec["events"]) | set(range(0, len(steps), 10)))
        t = rt.build_life(spec)
        want = t.optimize("direct", **tw.STRICT)
        r = g.optimize(pgo_params(**tw.STRICT))
        dt, dr = tw.pose_distance(list(g.poses()), t.poses)
        print(f"{len(steps)} steps, {seen['iterations']} accepted iterations on the way; at the end cost {r['final_cost']!r} / {want['final_cost']!r}, poses against the "
              f"statement's optimum {dt:.3e} m {dr:.3e} rad")
        assert abs(r["final_cost"] - want["final_cost"]) <= 1e-9 * want["final_cost"]
        bm, br = bars(TWIN_LIFE)
        assert dt <= bm and dr <= br
    finally:
        g.close()
