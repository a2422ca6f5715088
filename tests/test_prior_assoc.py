"""CPU: the ground-prior association's host side (rolo_amd/backend.py: prior_association_gates, GroundPriorCloser.priorInfoHandler and its candidate walk) and the
scene of tests/prior_assoc_cases.py that the device test uses.

prior_association_gates is float32 in Eigen's operation order; it is held to a float64 statement of the same formulas written with scipy's Rotation and Slerp.
THE BOUND, counted and not fitted: from the inputs to poseTo the float32 chain is the 3 x 3 inverse by cofactors (10 roundings per entry), two 3 x 4 products
(7 each), a quaternion from a matrix with its normalisation (15), three Euler extractions (atan2 / asin of a quotient: 3 each), three half-angle quaternions
and their two products (6 + 14), a normalisation (9), slerp (dot 7, acos, three sines, two quotients, the combination 3: 16), a normalisation (9), the matrix
of a quaternion (6), the product with the linked pose (7) and the last Euler extraction (3): about 120 roundings, each at most 2^-24 of the magnitude it works
on. asin amplifies by 1 / cos(pitch) < 2 for the |pitch| < 1 used here. K = 256 covers both; SCALE is the largest magnitude in play: 1 for rotation entries
and angles, the largest |translation| of the inputs and of current * linked^-1 for lengths. Bound = K * 2^-24 * scale."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation, Slerp

import icp_twin as T
import prior_assoc_cases as pa
from rolo_amd import backend as B
from rolo_amd.backend import GroundPriorCloser, PriorFactor, pose6_to_T, prior_association_gates

f32, f64 = np.float32, np.float64
K = 256
EPS = 2.0 ** -24
TOL_ROT = float(f32(f32(5.0) * np.pi / f32(180.0)))
TOL_Z = 1.0


def euler64(M):
    return M[0, 3], M[1, 3], M[2, 3], np.arctan2(M[2, 1], M[2, 2]), np.arcsin(-M[2, 0]), np.arctan2(M[1, 0], M[0, 0])


def wrap(a):
    return np.arctan2(np.sin(a), np.cos(a))


def gates64(linked, current, relative, Ticp):
    """the float64 statement -> (diffs, odom 6, prior 6, priorTrans, poseTo)"""
    linked, current, relative, Ticp = (np.asarray(x, f32).astype(f64) for x in (linked, current, relative, Ticp))
    A = current @ np.linalg.inv(linked)
    P = Ticp @ relative
    o, p = euler64(A), euler64(P)
    diffs = (abs(o[2] - p[2]), abs(wrap(o[3] - p[3])), abs(wrap(o[4] - p[4])))
    target = Rotation.from_euler("ZYX", [o[5], p[4], p[3]])   # Rz(odom yaw) Ry(prior pitch) Rx(prior roll)
    odom_R = Rotation.from_matrix(A[:3, :3])
    blended = Slerp([0.0, 1.0], Rotation.concatenate([odom_R, target]))(B.PRIOR_WEIGHT)
    prior_trans = np.eye(4)
    prior_trans[:3, :3] = blended.as_matrix()
    prior_trans[:3, 3] = A[:3, 3]
    return diffs, o, p, prior_trans, prior_trans @ linked


def scale_of(linked, current, relative, Ticp):
    A = np.asarray(current, f64) @ np.linalg.inv(np.asarray(linked, f64))
    return max(1.0, *(float(np.abs(np.asarray(M, f64)[:3, 3]).max()) for M in (linked, current, relative, Ticp, A)))


def hold_to_statement(linked, current, relative, Ticp, fitness=2e-5):
    got = prior_association_gates(linked, current, relative, Ticp, fitness, TOL_ROT, TOL_Z, 100.0)
    diffs, o, p, prior_trans, pose_to = gates64(linked, current, relative, Ticp)
    scale = scale_of(linked, current, relative, Ticp)
    bound_rot, bound_len = K * EPS, K * EPS * scale
    err = [abs(float(got["diff"][0]) - diffs[0]), abs(float(got["diff"][1]) - diffs[1]), abs(float(got["diff"][2]) - diffs[2])]
    print("scale %.3g  diff errors %.3g %.3g %.3g  bounds %.3g (length) %.3g (angle)" % (scale, *err, bound_len, bound_rot))
    assert err[0] <= bound_len and err[1] <= bound_rot and err[2] <= bound_rot
    for k in range(3):
        assert abs(float(got["odom"][k]) - o[k]) <= bound_len and abs(float(got["prior"][k]) - p[k]) <= bound_len
        assert abs(wrap(float(got["odom"][3 + k]) - o[3 + k])) <= bound_rot and abs(wrap(float(got["prior"][3 + k]) - p[3 + k])) <= bound_rot
    want_rej = "z" if diffs[0] > TOL_Z else ("roll" if diffs[1] > TOL_ROT else ("pitch" if diffs[2] > TOL_ROT else None))
    assert got["rejected"] == want_rej
    if want_rej is None:
        e_rot = np.abs(got["priorTrans"][:3, :3].astype(f64) - prior_trans[:3, :3]).max()
        e_t = np.abs(got["priorTrans"][:3, 3].astype(f64) - prior_trans[:3, 3]).max()
        e_to_rot = np.abs(got["poseTo"][:3, :3] - pose_to[:3, :3]).max()
        e_to_t = np.abs(got["poseTo"][:3, 3] - pose_to[:3, 3]).max()
        print("priorTrans %.3g %.3g  poseTo %.3g %.3g" % (e_rot, e_t, e_to_rot, e_to_t))
        assert e_rot <= bound_rot and e_t <= bound_len and e_to_rot <= bound_rot and e_to_t <= bound_len
        assert got["poseTo"].dtype == f64 and np.array_equal(got["poseTo"][3], [0, 0, 0, 1])
        # poseFrom is the linked pose through its float Euler angles
        assert np.abs(got["poseFrom"][:3, :3] - np.asarray(linked, f64)[:3, :3]).max() <= bound_rot
        assert np.array_equal(got["poseFrom"][:3, 3], np.asarray(linked, f32)[:3, 3].astype(f64))
    return got


def P6(roll, pitch, yaw, x, y, z, dtype=f32):
    return pose6_to_T([roll, pitch, yaw, x, y, z], dtype)


# ---- the gates' arithmetic against the float64 statement --------------------------------------------------------------------------------------------------
GENERIC = [
    (P6(0.02, -0.01, 0.3, 4.0, 0.2, 0.1), P6(0.03, -0.02, 0.35, 4.4, 0.3, 0.12), P6(0.004, -0.003, 0.005, 0.05, -0.02, 0.01), P6(0.012, -0.02, 0.03, 0.05, -0.04, 0.03)),
    (P6(-0.3, 0.4, -2.0, -7.0, 3.0, 1.0), P6(-0.28, 0.38, -1.9, -6.5, 3.2, 1.1), P6(0.01, 0.02, -0.03, 0.2, 0.1, -0.05), P6(-0.03, 0.02, 0.1, -0.1, 0.2, 0.05)),
    (np.eye(4, dtype=f32), P6(0.0, 0.0, 0.0, 0.4, 0.0, 0.0), np.eye(4, dtype=f32), np.eye(4, dtype=f32)),
]


@pytest.mark.parametrize("case", range(len(GENERIC)))
def test_gates_equal_the_float64_statement(case):
    got = hold_to_statement(*GENERIC[case])
    assert got["rejected"] is None


def test_roll_and_pitch_near_the_pi_wrap():
    """odometry roll +3.13, prior roll -3.135: 0.018 apart across the wrap, not 6.26; the pitch pair straddles nothing but is taken the same way"""
    linked = np.eye(4, dtype=f32)
    current = P6(3.13, 0.3, 0.1, 0.3, 0.1, 0.0)
    Ticp = P6(-3.135, 0.31, 0.12, 0.1, 0.0, 0.05)
    got = hold_to_statement(linked, current, np.eye(4, dtype=f32), Ticp)
    assert got["rejected"] is None and abs(float(got["diff"][1]) - (2 * np.pi - 3.13 - 3.135)) < 1e-5
    # ... and one that is out across the wrap
    got = hold_to_statement(linked, current, np.eye(4, dtype=f32), P6(-3.0, 0.31, 0.12, 0.1, 0.0, 0.05))
    assert got["rejected"] == "roll"


def test_slerp_sign_flip_between_hemispheres():
    """a relative yaw of -3.0: the quaternion of the matrix comes out with w < 0 (its largest diagonal entry decides the branch), Rz Ry Rx's with w > 0"""
    linked = P6(0.0, 0.0, 0.2, 1.0, 0.0, 0.0)
    current = (P6(0.01, 0.02, -3.0, 0.0, 0.0, 0.0).astype(f64) @ linked.astype(f64)).astype(f32)
    Ticp = P6(0.03, -0.01, -2.9, 0.2, 0.1, 0.0)
    A = B._mul34(current, B._inv34(linked))
    o, p = B._euler34(A), B._euler34(Ticp)
    qa = B._quat_norm(B._quat_from_R(A[:3, :3]))
    qb = B._quat_norm(B._quat_mul(B._quat_mul(B._quat_axis(o[5], 2), B._quat_axis(p[4], 1)), B._quat_axis(p[3], 0)))
    assert float(np.dot(qa, qb)) < -0.9   # of the test's own inputs: opposite hemispheres
    got = hold_to_statement(linked, current, np.eye(4, dtype=f32), Ticp)
    assert got["rejected"] is None


def test_slerp_linear_branch_for_a_nearly_identical_pair():
    linked = P6(0.0, 0.0, 0.0, 2.0, 0.0, 0.0)
    current = P6(1e-4, -1e-4, 0.05, 2.4, 0.0, 0.0)
    Ticp = P6(1.5e-4, -0.5e-4, 0.0, 0.0, 0.0, 0.0)
    A = B._mul34(current, B._inv34(linked))
    o, p = B._euler34(A), B._euler34(Ticp)
    qa = B._quat_norm(B._quat_from_R(A[:3, :3]))
    qb = B._quat_norm(B._quat_mul(B._quat_mul(B._quat_axis(o[5], 2), B._quat_axis(p[4], 1)), B._quat_axis(p[3], 0)))
    assert abs(float(np.dot(qa, qb))) >= 1.0 - float(np.finfo(f32).eps)   # of the test's own inputs: Eigen's linear branch
    hold_to_statement(linked, current, np.eye(4, dtype=f32), Ticp)


# ---- each gate from both sides ------------------------------------------------------------------------------------------------------------------------------
def planted(which, excess):
    """linked, current, relative, T with the `which` difference at its tolerance + excess, the other two well inside"""
    linked = P6(0.01, -0.02, 0.1, 2.0, 0.5, 0.1)
    current = P6(0.02, -0.01, 0.15, 2.4, 0.6, 0.15)
    A = current.astype(f64) @ np.linalg.inv(linked.astype(f64))
    x, y, z, r, p, yw = euler64(A)
    dz = (TOL_Z + excess) if which == "z" else 0.01
    dr = (TOL_ROT + excess) if which == "roll" else 0.002
    dp = (TOL_ROT + excess) if which == "pitch" else -0.003
    return linked, current, np.eye(4, dtype=f32), pose6_to_T([r + dr, p + dp, yw + 0.01, x, y, z + dz], f64).astype(f32)


@pytest.mark.parametrize("which", ["z", "roll", "pitch"])
def test_each_gate_from_both_sides(which):
    """the planted excess is 1e-3 either way: 16 times the bound at this scale (256 * 2^-24 * 2.4 = 3.7e-5)"""
    under = hold_to_statement(*planted(which, -1e-3))
    over = hold_to_statement(*planted(which, +1e-3))
    assert under["rejected"] is None and over["rejected"] == which


def test_gate_order_is_z_then_roll_then_pitch():
    linked, current, rel, _ = planted("z", 0.5)
    A = current.astype(f64) @ np.linalg.inv(linked.astype(f64))
    x, y, z, r, p, yw = euler64(A)
    all_out = pose6_to_T([r + 0.5, p + 0.5, yw, x, y, z + 2.0], f64).astype(f32)
    rp_out = pose6_to_T([r + 0.5, p + 0.5, yw, x, y, z], f64).astype(f32)
    assert prior_association_gates(linked, current, rel, all_out, 1e-3, TOL_ROT, TOL_Z)["rejected"] == "z"
    assert prior_association_gates(linked, current, rel, rp_out, 1e-3, TOL_ROT, TOL_Z)["rejected"] == "roll"


def test_variances_and_their_order():
    args = GENERIC[0]
    v = prior_association_gates(*args, 2.5e-3, TOL_ROT, TOL_Z, 100.0)["variances"]
    s = f64(f32(2.5e-3) * f32(100.0))
    small = f64(f32(1e-6))
    assert v.dtype == f64 and np.array_equal(v, [s, s, small, small, small, s])   # roll, pitch | yaw, x, y | z: gtsam's rotation-first order
    v = prior_association_gates(*args, 1e-9, TOL_ROT, TOL_Z, 100.0)["variances"]   # the floor: max((float)fitness, 1e-6f)
    assert np.array_equal(v, [f64(f32(1e-6) * f32(100.0))] * 2 + [small] * 3 + [f64(f32(1e-6) * f32(100.0))])
    v = prior_association_gates(*args, 0.5, TOL_ROT, TOL_Z, 0.25)["variances"]
    assert v[0] == 0.125 and v[5] == 0.125 and v[2] == small


# ---- priorInfoHandler ---------------------------------------------------------------------------------------------------------------------------------------
def closer_on(keys, **kw):
    return GroundPriorCloser(keys, icp=object(), groundPatchSize=pa.PATCH, **kw)   # no ICP is reached in these tests


PATCH3 = np.zeros((3, 4), f32)


def test_handler_needs_key_ten():
    keys = pa.Keys()
    c = closer_on(keys)
    assert not c.priorInfoHandler(0.0, np.zeros(6), PATCH3)          # no key pose at all
    for k in range(10):
        keys.add(k)
    assert len(keys.poses) == 10 and not c.priorInfoHandler(pa.KEY_TIMES[9], np.zeros(6), PATCH3)   # latestKeyID 9
    keys.add(10)
    assert c.priorInfoHandler(pa.KEY_TIMES[10], np.zeros(6), PATCH3)                                 # latestKeyID 10
    assert c.priorTimeKeyQueue == [(pa.KEY_TIMES[10], 10)] and len(c.priorPosePatchHistory) == 1


def test_handler_time_gate_and_synced_interval():
    keys = pa.Keys(12)
    c = closer_on(keys)
    t = pa.KEY_TIMES[11]
    assert c.priorInfoHandler(t + 0.009, np.zeros(6), PATCH3) and not c.priorInfoHandler(t + 0.011, np.zeros(6), PATCH3)
    assert c.priorInfoHandler(t - 0.009, np.zeros(6), PATCH3) and not c.priorInfoHandler(t - 0.011, np.zeros(6), PATCH3)
    assert len(c.priorTimeKeyQueue) == 2
    c = closer_on(keys, priorSyncedInterval=0.005)
    assert c.priorInfoHandler(t, np.zeros(6), PATCH3)
    assert not c.priorInfoHandler(t + 0.004, np.zeros(6), PATCH3)    # within the interval of the last accepted entry
    assert c.priorInfoHandler(t + 0.006, np.zeros(6), PATCH3)
    assert [k for _, k in c.priorTimeKeyQueue] == [11, 11]
    pose = c.priorPosePatchHistory[0][0]
    assert pose.dtype == f64 and pose.shape == (6,)


# ---- the scene of the device test: the twin alone gives the intended verdicts -------------------------------------------------------------------------------
def test_scene_sizes_and_twin_verdicts():
    target, sources = pa.scene()
    assert 300 <= len(target) <= 2000 and all(300 <= len(s) <= 2000 for s in sources.values())
    tw = pa.twin_results()
    for name, r in tw.items():
        print(name, "state", r["state"], "iterations", r["iterations"], "margin", r["margin"], "fitness", r["fitness"])
        assert r["converged"] and r["margin"] > 1e-3, name   # no exit is left to rounding
    assert tw["other_terrain"]["fitness"] > 0.01 * 2          # fails the fitness gate, and not by rounding
    for name in ("rolled", "good", "good_after"):
        assert tw[name]["fitness"] < 0.01 / 2 and tw[name]["fitness"] > 1e-6   # passes it; above the noise score's floor


def test_scene_walk_with_the_twin_as_the_icp():
    """GroundPriorCloser's own walk with icp_twin.icp in LoopIcp's place: the radius keeps entry 0 away from the ICP, the fitness and roll gates turn away
    entries 1 and 2, entry 3 gives the factor and entry 4 is never judged"""
    class TwinIcp:
        def alignBatch(self, sources, target, params, guesses=None):
            assert guesses is None and params.max_iterations == 100 and params.max_correspondence_distance == pa.PATCH
            assert params.transformation_epsilon == 1e-6 and params.euclidean_fitness_epsilon == 1e-6
            self.calls.append(len(sources))
            return [T.icp(s, target, max_correspondence_distance=pa.PATCH) for s in sources]

    facts = {}
    for batch in (1, 2, 8):
        keys = pa.Keys()
        icp = TwinIcp(); icp.calls = []
        c = GroundPriorCloser(keys, icp=icp, groundPatchSize=pa.PATCH, priorFactorWeight=pa.WEIGHT, batch=batch)
        assert c.performPriorAssociation() is None                       # nothing stored yet
        assert pa.feed(c, keys.add) == [True] * 5
        assert [e for e, _, _, _ in c.candidates()] == [1, 2, 3, 4]        # entry 0 is outside the radius
        f = c.performPriorAssociation()
        assert isinstance(f, PriorFactor) and (f.linked_key, f.current_key) == (10, 11)
        assert [(r["entry"], r["rejected"]) for r in c.last if r["rejected"] != "unused"] == [(1, "fitness"), (2, "roll"), (3, None)]
        # entry 4 is never judged; a chunk that holds it next to entry 3 has aligned it (batch 2: chunks (1, 2), (3, 4)), batch 1 never touches it
        assert [r["entry"] for r in c.last if r["rejected"] == "unused"] == ([] if batch == 1 else [4])
        assert icp.calls == {1: [1, 1, 1], 2: [2, 2], 8: [4]}[batch]
        assert c.priorVisContainer[11][0] == 10 and np.array_equal(c.priorVisContainer[11][1], np.asarray(pa.ENTRIES["good"][1], f32))
        assert len(c.priorPosePatchHistory) == 5                         # never popped
        facts[batch] = f
    for batch in (2, 8):
        for a, b in zip(facts[1][2:], facts[batch][2:]):
            assert np.array_equal(a, b)
    # the factor is the statement's for entry 3
    linked, current = pose6_to_T(pa.key_pose(10)), pose6_to_T(pa.key_pose(11))
    tw = pa.twin_results()["good"]
    g = prior_association_gates(linked, current, pose6_to_T(np.asarray(pa.ENTRIES["good"][1], f32)), tw["T"], tw["fitness"], TOL_ROT, TOL_Z, pa.WEIGHT)
    assert np.array_equal(facts[1].poseTo, g["poseTo"]) and np.array_equal(facts[1].variances, g["variances"])
