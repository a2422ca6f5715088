"""GPU: GroundPriorCloser over a resident key map and the batched loop ICP, on the scene of tests/prior_assoc_cases.py (twelve key poses, five history entries:
outside the radius, other terrain, a planted roll, a good one, one more good one behind it), held to the CPU statement — icp_twin.icp per candidate plus
prior_association_gates — and the factor's way into the pose graph."""
import numpy as np
import pytest

import icp_twin as T
import prior_assoc_cases as pa
from rolo_amd.backend import GroundPriorCloser, KeyFrameMap, LoopIcp, PoseGraph, PriorFactor, pose6_to_T, prior_association_gates

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
BAR_M, BAR_RAD = 1e-4, 1e-5   # BASELINE.json's bars for the ICP's pose against the twin


@pytest.fixture(scope="module")
def icp():
    h = LoopIcp()
    yield h
    h.close()


def run_closer(icp, batch):
    km = KeyFrameMap()
    try:
        c = GroundPriorCloser(km, icp=icp, groundPatchSize=pa.PATCH, priorFactorWeight=pa.WEIGHT, batch=batch)
        empty = np.zeros((0, 4), f32)
        told = pa.feed(c, lambda k: km.addKeyFrame(empty, empty, pa.key_pose(k), pa.KEY_TIMES[k]))
        assert told == [True] * 5 and len(km) == pa.N_KEYS
        f = c.performPriorAssociation()
        return c, f
    finally:
        km.close()


@pytest.fixture(scope="module")
def runs(icp):
    return {batch: run_closer(icp, batch) for batch in (1, 2, 8)}


def test_the_factor_is_the_good_entrys(runs):
    c, f = runs[8]
    assert isinstance(f, PriorFactor) and (f.linked_key, f.current_key) == (10, 11)
    judged = [(r["entry"], r["rejected"]) for r in c.last if r["rejected"] != "unused"]
    assert judged == [(1, "fitness"), (2, "roll"), (3, None)]          # entry 0, outside the radius, never reached the ICP
    assert 0 not in [r["entry"] for r in c.last]
    assert c.priorVisContainer[11][0] == 10 and np.array_equal(c.priorVisContainer[11][1], np.asarray(pa.ENTRIES["good"][1], f32))
    assert len(c.priorPosePatchHistory) == 5                           # never popped


def test_later_entries_and_chunks(runs):
    """entry 4 is never judged. batch 1 never aligns it; a chunk that holds it next to entry 3 (batch 2: (1, 2), (3, 4); batch 8: all four) has aligned it and says so"""
    for batch, unused in ((1, []), (2, [4]), (8, [4])):
        c, _ = runs[batch]
        assert [r["entry"] for r in c.last if r["rejected"] == "unused"] == unused
        assert [r["entry"] for r in c.last] == [1, 2, 3] + unused


def test_every_batch_size_gives_the_same_bits(runs):
    _, f1 = runs[1]
    for batch in (2, 8):
        _, f = runs[batch]
        assert f[:2] == f1[:2]
        for a, b in zip(f[2:], f1[2:]):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        for ra, rb in zip(runs[batch][0].last[:3], runs[1][0].last[:3]):
            assert np.array_equal(ra["icp"]["T"], rb["icp"]["T"]) and ra["icp"]["fitness"] == rb["icp"]["fitness"] and ra["icp"]["iterations"] == rb["icp"]["iterations"]


def test_against_the_cpu_statement(runs):
    c, f = runs[8]
    tw = pa.twin_results()
    for r in c.last:
        name = pa.ENTRY_NAMES[r["entry"]]
        want, got = tw[name], r["icp"]
        assert want["margin"] > 1e-3
        dt = np.linalg.norm(got["T"][:3, 3].astype(f64) - want["T"][:3, 3])
        dr = T.rot_angle(got["T"][:3, :3].astype(f64) @ want["T"][:3, :3].astype(f64).T)
        print(name, "state", got["state"], want["state"], "iterations", got["iterations"], want["iterations"], "fitness", got["fitness"], want["fitness"],
              "pose %.3g m %.3g rad" % (dt, dr))
        assert got["state"] == want["state"] and got["iterations"] == want["iterations"] and got["converged"] == want["converged"]
        assert dt <= BAR_M and dr <= BAR_RAD
        assert abs(got["fitness"] - want["fitness"]) <= 1e-6 * want["fitness"] + 1e-12
    # the factor from the twin's ICP through the same gates: poseFrom has no ICP in it; poseTo carries a fifth of the ICP's rotation difference (slerp's weight)
    # and, through the linked pose's 4 m lever, that angle times 4 m
    linked, current = pose6_to_T(pa.key_pose(10)), pose6_to_T(pa.key_pose(11))
    g = prior_association_gates(linked, current, pose6_to_T(np.asarray(pa.ENTRIES["good"][1], f32)), tw["good"]["T"], tw["good"]["fitness"], c.rot_tol, c.trans_tol, c.weight)
    assert g["rejected"] is None
    assert np.array_equal(f.poseFrom, g["poseFrom"])
    dr = T.rot_angle(f.poseTo[:3, :3] @ g["poseTo"][:3, :3].T)
    dt = np.linalg.norm(f.poseTo[:3, 3] - g["poseTo"][:3, 3])
    lever = float(np.linalg.norm(linked[:3, 3]))
    print("poseTo against the statement: %.3g m %.3g rad" % (dt, dr))
    assert dr <= BAR_RAD and dt <= BAR_M + BAR_RAD * lever
    assert np.allclose(f.variances, g["variances"], rtol=2e-6, atol=0) and np.array_equal(f.variances[2:5], g["variances"][2:5])


def graph_of_the_keys():
    g = PoseGraph()
    for k in range(pa.N_KEYS):
        assert g.addOdomFactor(pa.key_pose(k)) == k
    return g


def test_add_prior_factor_is_add_between(runs):
    _, f = runs[8]
    a, b = graph_of_the_keys(), graph_of_the_keys()
    try:
        a.addPriorFactor(f)
        b.addBetween(10, 11, np.linalg.inv(f.poseFrom) @ f.poseTo, f.variances)
        assert a.size() == b.size() and a.size()[1] == pa.N_KEYS + 1
        for x, y in zip(a.linearize(), b.linearize()):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
        for x, y in zip(a.factorErrors(), b.factorErrors()):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
        ra, rb = a.optimize(), b.optimize()
        assert ra == rb and a.poses().tobytes() == b.poses().tobytes()
    finally:
        a.close(); b.close()


def test_optimise_moves_roll_pitch_z_toward_the_prior(runs):
    """in terms of the step from key 10 to key 11 (what both factors on that edge measure): the prior factor's variances on roll, pitch and z are about the
    odometry's 1e-6 (pa.WEIGHT), so the optimum sits between the two measurements there; on yaw, x and y the factor repeats the odometry (blended yaw and
    translation are the odometry's), so they stay within the odometry factor's sigma (1e-3 rad, 1e-2 m)"""
    _, f = runs[8]
    g = graph_of_the_keys()
    try:
        def step():
            P = g.poses()
            M = np.linalg.inv(P[10]) @ P[11]
            return np.array([np.arctan2(M[2, 1], M[2, 2]), np.arcsin(-M[2, 0]), np.arctan2(M[1, 0], M[0, 0]), M[0, 3], M[1, 3], M[2, 3]])
        before = step()
        Z = np.linalg.inv(f.poseFrom) @ f.poseTo
        z6 = np.array([np.arctan2(Z[2, 1], Z[2, 2]), np.arcsin(-Z[2, 0]), np.arctan2(Z[1, 0], Z[0, 0]), Z[0, 3], Z[1, 3], Z[2, 3]])
        g.addPriorFactor(f)
        r = g.optimize()
        after = step()
        print("state", r["state"], "step before", before, "measured", z6, "after", after)
        assert r["final_cost"] < r["initial_cost"]
        for k in (0, 1, 5):   # roll, pitch, z
            gap = abs(before[k] - z6[k])
            assert gap > 1e-4, (k, gap)                                  # of the test's own inputs: there is something to move toward
            assert abs(after[k] - z6[k]) < gap and (after[k] - before[k]) * (z6[k] - before[k]) > 0, k
        assert abs(after[2] - before[2]) <= 1e-3 and abs(after[3] - before[3]) <= 1e-2 and abs(after[4] - before[4]) <= 1e-2
    finally:
        g.close()
