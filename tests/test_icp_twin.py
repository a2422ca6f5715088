"""CPU: the numpy twin of the loop closure's ICP (tests/icp_twin.py) does what the statement says — it recovers a known motion, reaches every exit, survives
the reflection and the collinear case — and the host detector rolo_keyposes_detect_loop_distance agrees with its numpy statement."""
import numpy as np
import pytest

import icp_twin as T
from rolo_amd import synth
from rolo_amd.backend import detect_loop_distance

f32 = np.float32


def room(n, seed, noise=0.0):
    """n points on the floor and the four walls of a 20 x 14 x 5 m hall with a step in one wall (no direction ICP could slide along), float32 n x 3"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 5, n); a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    x = np.where(f == 1, -10.0, np.where(f == 2, 10.0, 20 * a - 10))
    y = np.where(f == 0, 14 * b - 7, np.where((f == 1) | (f == 2), 14 * a - 7, np.where(f == 3, -7.0, 7.0 - 3.0 * (a > 0.6))))
    z = np.where(f == 0, 0.0, 5 * b)
    return (np.stack([x, y, z], axis=1) + rng.normal(0, noise, (n, 3))).astype(f32)


def motion(rpy=(0.01, -0.02, 0.03), t=(0.15, -0.1, 0.05)):
    M = np.eye(4); M[:3, :3] = synth.rpy_to_R(*rpy); M[:3, 3] = t
    return M


def moved_pair(n_tgt=3000, n_src=800, seed=1, noise=0.01, M=None):
    """(source, target, M): the source is a subsample of the target moved by M^-1, so M is the truth"""
    M = motion() if M is None else M
    tgt = room(n_tgt, seed, noise)
    sub = tgt[np.random.default_rng(seed + 1).choice(n_tgt, n_src, replace=False)]
    src = ((sub.astype(np.float64) - M[:3, 3]) @ M[:3, :3]).astype(f32)
    return src, tgt, M


def pose_error(T4, M):
    return np.linalg.norm(T4[:3, 3].astype(np.float64) - M[:3, 3]), T.rot_angle(T4[:3, :3].astype(np.float64) @ M[:3, :3].T)


def test_recovers_a_known_motion_to_float_rounding():
    src, tgt, M = moved_pair(noise=0.0)
    r = T.icp(src, tgt, max_correspondence_distance=2.0)
    dt, dr = pose_error(r["T"], M)
    # coordinates up to 10 m carry 1e-6 m of float rounding each; the fit averages 800 of them
    assert r["converged"] and dt < 2e-6 and dr < 1e-6, (dt, dr)
    assert r["fitness"] < 1e-11 and r["n_last"] == len(src)


CASES = {
    T.TRANSFORM: dict(max_correspondence_distance=2.0),
    T.ITERATIONS: dict(max_correspondence_distance=2.0, max_iterations=2),
    T.ABS_MSE: dict(max_correspondence_distance=2.0, transformation_epsilon=1e-30, max_iterations=40),
    T.REL_MSE: dict(max_correspondence_distance=2.0, transformation_epsilon=1e-30, euclidean_fitness_epsilon=0.5),
    T.NO_CORRESPONDENCES: dict(max_correspondence_distance=1e-4),
}


@pytest.mark.parametrize("state", sorted(CASES))
def test_every_exit_is_reachable(state):
    src, tgt, _ = moved_pair(noise=0.0 if state == T.ABS_MSE else 0.01)
    r = T.icp(src, tgt, **CASES[state])
    assert r["state"] == state, (r["state"], r["iterations"])
    assert r["converged"] == (state != T.NO_CORRESPONDENCES)
    assert len(r["trace"]) == r["iterations"] + (2 if state == T.NO_CORRESPONDENCES else 1)


def test_reflection_case_gives_a_rotation():
    """mirrored correspondences: the unconstrained optimum has det -1; diag(1, 1, -1) brings back a proper rotation"""
    p = room(200, 5).astype(np.float64)
    q = p * np.array([1.0, 1.0, -1.0])
    terms = np.concatenate([np.ones((200, 1)), np.zeros((200, 1)), p, q, (p[:, :, None] * q[:, None, :]).reshape(200, 9)], axis=1)
    R, t = T.umeyama(terms.sum(axis=0))
    assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.allclose(R @ R.T, np.eye(3), atol=1e-12)


def test_collinear_correspondences_give_a_rotation_that_maps_the_line():
    s = np.linspace(-3, 3, 50)
    d0, d1 = np.array([1.0, 2.0, -1.0]) / np.sqrt(6.0), np.array([0.0, 1.0, 1.0]) / np.sqrt(2.0)
    p = s[:, None] * d0 + np.array([0.5, 0.0, 1.0]); q = s[:, None] * d1 + np.array([-1.0, 2.0, 0.0])
    terms = np.concatenate([np.ones((50, 1)), np.zeros((50, 1)), p, q, (p[:, :, None] * q[:, None, :]).reshape(50, 9)], axis=1)
    R, t = T.umeyama(terms.sum(axis=0))
    assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.allclose(R @ R.T, np.eye(3), atol=1e-12)
    assert np.allclose(p @ R.T + t, q, atol=1e-12)


def test_association_ties_cap_and_duplicates():
    tgt = np.array([[2, 0, 0], [0, 2, 0], [0, 2, 0], [-2, 0, 0], [5, 5, 5]], f32)
    src = np.array([[0, 0, 0], [5, 5, 2]], f32)
    idx, d2 = T.associate(src, tgt, 2.0)
    assert idx.tolist() == [0, -1] and d2[0] == 4.0 and np.isinf(d2[1])      # four at d2 = 4: the smallest index; exactly at the cap: kept
    idx, d2 = T.associate(src, tgt, np.nextafter(2.0, 0.0))
    assert idx.tolist() == [-1, -1]
    idx, d2 = T.associate(src[:1] + f32(0.1), tgt[1:3])
    assert idx.tolist() == [0]                                                # duplicated target points: the first


# ---- detectLoopClosureDistance ------------------------------------------------------------------------------------------------------------------------------
def both(xyz, times, time_cur, radius=30.0, time_diff=30.0):
    got = detect_loop_distance(xyz, times, time_cur, radius, time_diff)
    assert got == T.detect_loop_distance(xyz, times, time_cur, radius, time_diff)
    return got


def test_detect_time_gate_two_sides():
    xyz = [[0, 0, 0], [1, 0, 0], [50, 0, 0], [0.5, 0, 0]]          # keys 0 and 1 are equally near the last one, key 2 is outside the radius
    assert both(xyz, [0.0, 69.0, 80.0, 100.0], 100.0) == 0       # both are old enough: the smaller index
    assert both(xyz, [70.0, 69.0, 80.0, 100.0], 100.0) == 1      # |70 - 100| = 30 is not > 30: key 0 fails the gate, key 1 (31 s) passes
    assert both(xyz, [71.0, 70.0, 0.0, 100.0], 100.0) == -1      # the only old key is outside the radius
    assert both(xyz, [200.0, 70.0, 0.0, 100.0], 100.0) == 0      # the gate is on the absolute difference


def test_detect_last_key_as_the_only_hit():
    xyz = [[0, 0, 0], [100, 0, 0]]
    assert both(xyz, [0.0, 10.0], 100.0) == -1                   # the last key qualifies by time (stamped 10, asked at 100) and is itself: no loop
    assert both(xyz, [0.0, 10.0], 10.0) == -1


def test_detect_ties_go_to_the_smaller_index():
    xyz = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, 0, 0]]
    assert both(xyz, [0.0, 0.0, 0.0, 0.0, 100.0], 100.0) == 0
    assert both(xyz, [90.0, 0.0, 0.0, 0.0, 100.0], 100.0) == 1
    assert both(xyz, [0.0, 0.0, 0.0, 0.0, 100.0], 100.0, radius=1.0) == -1   # d2 = 1 is not below 1


def test_detect_empty_store():
    assert both(np.zeros((0, 3)), np.zeros(0), 5.0) == -1
