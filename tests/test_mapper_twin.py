"""CPU: the mapper's three host-only functions (rolo_mapper_initial_guess / _save_frame / _incremental: the mapping node's float pose bookkeeping) against the float64
statement tests/mapper_twin.py, within the bound that file derives from the float operations and the operand magnitudes; angles up to +-3 rad, translations up to
10^3 m. Also here: rolo_mapper_create without a GPU, the defaults, and the build of the C++ demo."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from rolo_amd import _lib
from rolo_amd.backend import mapper_initial_guess, mapper_save_frame, mapper_incremental, mapper_params
import mapper_twin as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
IDENT12 = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], f32)


def draw_pose(rng, tmax=1e3, amax=3.0):
    return np.concatenate([rng.uniform(-amax, amax, 3), rng.uniform(-tmax, tmax, 3)]).astype(f32)


def stored_affine(pose6):
    """the float lastOdomTransformation the library stores for a first guess (:540-543)"""
    _, last, avail = mapper_initial_guess(np.zeros(6, f32), True, pose6, IDENT12, False)
    assert avail
    return last


def within(got, want, bound, what):
    err = np.abs(np.asarray(got, np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    assert np.all(err <= bound), (what, err, bound)
    return worst


def test_initial_guess_branches_are_exact():
    rng = np.random.default_rng(1)
    tf, guess = draw_pose(rng), draw_pose(rng)
    last = stored_affine(draw_pose(rng))
    # no key frame: roll, pitch, yaw zeroed, the rest and the odometry memory untouched, with or without a guess (:524-531)
    for g in (None, guess):
        out, lo, avail = mapper_initial_guess(tf, False, g, last, True)
        assert np.array_equal(out, np.concatenate([np.zeros(3, f32), tf[3:]])) and np.array_equal(lo, last) and avail
    # no odometry: nothing changes (:536)
    out, lo, avail = mapper_initial_guess(tf, True, None, last, True)
    assert out.tobytes() == tf.tobytes() and np.array_equal(lo, last) and avail
    # the first available guess is only stored (:540-543)
    out, lo, avail = mapper_initial_guess(tf, True, guess, IDENT12, False)
    want = tw.initial_guess(tf, True, guess, IDENT12, False)
    assert out.tobytes() == tf.tobytes() and avail
    b = np.concatenate([np.full(3, want["last"].dR), [0.0]] * 3) * tw.SLACK
    within(lo, want["last"].M.reshape(12), b, "lastOdomTransformation")
    assert np.array_equal(lo.reshape(3, 4)[:, 3], guess[3:])


@pytest.mark.parametrize("tmax", [10.0, 1e3])
def test_initial_guess_moves_the_pose_by_the_odometry_increment(tmax):
    rng = np.random.default_rng(int(tmax))
    worst, n = 0.0, 0
    while n < 300:
        tf, guess, prev = draw_pose(rng, tmax), draw_pose(rng, tmax), draw_pose(rng, tmax)
        last = stored_affine(prev)
        want = tw.initial_guess(tf, True, guess, last, True)
        if want["cos_pitch"] < tw.MIN_COS_PITCH:
            continue
        n += 1
        out, lo, avail = mapper_initial_guess(tf, True, guess, last, True)
        worst = max(worst, within(out, want["tf"], want["tf_bound"], "transformTobeMapped"))
        assert avail and np.array_equal(lo, stored_affine(guess))   # :551
    print(f"updateInitialGuess, translations to {tmax}: largest error / bound {worst:.3f}")
    # a small increment behind a pose is recovered: guess = prev * delta moves tf to tf * delta
    tf, prev = draw_pose(rng, tmax), draw_pose(rng, tmax)
    delta = np.array([0.01, -0.02, 0.03, 0.5, -0.2, 0.1], f32)
    out, _, _ = mapper_initial_guess(tf, True, tw.compose(prev, delta), stored_affine(prev), True)
    want = tw.xyzrpy(tw.mul(tw.aff_of_pose(tf), tw.aff_of_pose(delta)))[0]
    assert np.abs(out[3:] - want[:3]).max() < 1e-3 * max(1.0, tmax / 10) and np.abs(out[:3] - want[3:]).max() < 1e-3


def planted_save_frame_cases():
    """(name, last key pose, pose, expected): one step quantity 1.1 x 10^-3 below or above its threshold, the others far below theirs"""
    rng = np.random.default_rng(7)
    out = []
    for q, name in enumerate(("roll", "pitch", "yaw", "distance")):
        for side, expect in ((-1.1e-3, False), (+1.1e-3, True)):
            for sign in (1.0, -1.0):
                last = np.concatenate([rng.uniform(-3, 3, 3), rng.uniform(-10, 10, 3)]).astype(f32)
                delta = np.array([0.01, -0.02, 0.015, 0.1, -0.05, 0.02])
                if q < 3:
                    delta[q] = sign * (0.2 + side)
                else:
                    d = rng.normal(size=3); d /= np.linalg.norm(d)
                    delta[3:] = sign * d * (1.0 + side)
                out.append((f"{name} {'above' if expect else 'below'} {'+' if sign > 0 else '-'}", last, tw.compose(last, delta.astype(f32)), expect))
    return out


def test_save_frame_at_planted_thresholds():
    assert mapper_save_frame(None, np.zeros(6, f32)) is True   # :1073-1074
    for name, last, tf, expect in planted_save_frame_cases():
        want = tw.save_frame(last, tf, 1.0, 0.2)
        assert want["margin"] >= 1e-3 and want["bounds"].max() < want["margin"], (name, want)   # the case sits where it was planted, and float cannot move it across
        assert want["save"] is expect, name
        assert mapper_save_frame(last, tf, 1.0, 0.2) is expect, name
    # everything below: not saved; other thresholds are honoured
    last = np.array([0.1, -0.2, 2.5, 3.0, -4.0, 0.5], f32)
    tf = tw.compose(last, np.array([0.05, 0.05, 0.05, 0.3, 0.3, 0.3], f32))
    assert mapper_save_frame(last, tf, 1.0, 0.2) is False and mapper_save_frame(last, tf, 0.5, 0.2) is True and mapper_save_frame(last, tf, 1.0, 0.04) is True


def test_save_frame_on_random_pairs():
    rng = np.random.default_rng(9)
    decided = 0
    for _ in range(400):
        last = draw_pose(rng, 1e3)
        tf = tw.compose(last, np.concatenate([rng.uniform(-0.4, 0.4, 3), rng.uniform(-1.2, 1.2, 3)]).astype(f32)) if rng.random() < 0.7 else draw_pose(rng, 1e3)
        want = tw.save_frame(last, tf, 1.0, 0.2)
        if want["cos_pitch"] < tw.MIN_COS_PITCH or np.any(want["margins"] <= want["bounds"]):
            continue   # float may put a quantity on either side of its threshold: no statement
        decided += 1
        assert mapper_save_frame(last, tf, 1.0, 0.2) is want["save"], (last, tf, want)
    assert decided > 100   # (of 400 draws: the generator has not drifted into cases without a statement)


def test_incremental_pose():
    rng = np.random.default_rng(11)
    # the first call takes the pose itself (:1365-1369)
    tf = draw_pose(rng)
    inc, pose = mapper_incremental(np.zeros(6, f32), np.zeros(6, f32), tf, False, IDENT12)
    want = tw.incremental(None, None, tf, False, None)
    b = np.concatenate([np.full(3, want["incre"].dR), [0.0]] * 3) * tw.SLACK
    within(inc, want["incre"].M.reshape(12), b, "increOdomAffine")
    worst, n = 0.0, 0
    for tmax in (10.0, 1e3):
        n = 0
        while n < 300:
            start, front = draw_pose(rng, tmax), draw_pose(rng, tmax)
            back = tw.compose(front, np.concatenate([rng.uniform(-0.3, 0.3, 3), rng.uniform(-2, 2, 3)]).astype(f32)) if rng.random() < 0.5 else draw_pose(rng, tmax)
            inc0, _ = mapper_incremental(front, back, start, False, IDENT12)
            want = tw.incremental(front, back, None, True, inc0)
            if want["cos_pitch"] < tw.MIN_COS_PITCH:
                continue
            n += 1
            inc1, pose = mapper_incremental(front, back, start, True, inc0)
            worst = max(worst, within(pose, want["pose"], want["pose_bound"], "incremental pose"))
            bm = np.concatenate([np.full(3, want["incre"].dR), [want["incre"].dt]] * 3) * tw.SLACK
            within(inc1, want["incre"].M.reshape(12), bm, "increOdomAffine")
    print(f"publishOdometry: largest error / bound {worst:.3f}")
    # front == back: the increment is the identity to rounding and the pose stays
    p = draw_pose(rng, 10.0)
    inc0, pose0 = mapper_incremental(p, p, p, False, IDENT12)
    _, pose1 = mapper_incremental(p, p, p, True, inc0)
    assert np.abs(pose1 - pose0).max() < 1e-4


def test_defaults_are_the_reference_s():
    p = mapper_params()
    assert (p.mappingProcessInterval, p.edgeFeatureMinValidNum, p.surfFeatureMinValidNum, p.sc_input) == (0.15, 10, 100, 1)
    assert [f32(v) for v in (p.mappingCornerLeafSize, p.mappingSurfLeafSize, p.surroundingKeyframeSearchRadius, p.surroundingKeyframeDensity,
                             p.surroundingkeyframeAddingDistThreshold, p.surroundingkeyframeAddingAngleThreshold, p.sc_leaf)] == [f32(v) for v in (0.2, 0.2, 50, 1, 1.0, 0.2, 0.5)]
    assert p.z_tollerance == np.finfo(f32).max and p.rotation_tollerance == np.finfo(f32).max


def test_create_without_a_gpu_is_a_loud_error():
    L = _lib.lib()
    h = ctypes.c_void_p()
    rc = L.rolo_mapper_create(0, None, ctypes.byref(h))
    if L.rolo_device_count() > 0:
        assert rc == 0 and h.value
        L.rolo_mapper_destroy(h)
    else:
        assert rc == -6 and b"no HIP device" in L.rolo_last_error() and not h.value


def test_mapper_demo_compiles_and_links():
    """MapOptimization of include/rolo_nodes_hip.hpp builds with plain g++ against the C ABI"""
    out = os.path.join(tempfile.mkdtemp(), "mapper_demo")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "mapper_demo.cpp"), "-o", out,
           "-L", os.path.join(ROOT, "rolo_amd"), "-lrolo_hip", "-Wl,-rpath," + os.path.join(ROOT, "rolo_amd"), "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
