"""GPU: the device-resident key-frame store and sub-map assembly (rolo_keymap_*, rolo_amd/csrc/submap.hip) against the CPU oracle, bit for bit:
pcl::VoxelGrid for clouds of any size (pyorc.voxelgrid), extractCloud (pyorc.get_transformation + transform_cloud_f + voxelgrid composed), the hand-over
to the scan-to-submap registration (rolo_scan2map_set_submap_keymap) and the whole chain selectNearby -> extractCloud -> setSubmapFrom -> optimise.
Every comparison of clouds is np.array_equal on float32 arrays."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from oracle import pyorc
from rolo_amd import synth
from rolo_amd.backend import KeyFrameMap, Scan2Map

pytestmark = pytest.mark.gpu

CFG = dict(n_scan=16, horizon_scan=1800)
CORNER_LEAF, SURF_LEAF = 0.2, 0.4
f32 = np.float32


def features(R, t, seed):
    fo = pyorc.front_params(**CFG)
    fr = synth.make_frame("vlp16", R, t, seed)
    e = pyorc.extract_features(fo, pyorc.project(fo, fr.xyz, fr.ring))
    return e["corner"], e["surface"]


def frame_pose(k):
    """key frame k of the test trajectory: 0.6 m apart, turning slowly; (R, t, transformTobeMapped order roll pitch yaw x y z)"""
    R = synth.rpy_to_R(0.002 * k, -0.001 * k, 0.03 * k)
    t = np.array([0.6 * k, 0.05 * k, 0.0])
    return R, t, np.concatenate([Rotation.from_matrix(R).as_euler("xyz"), t]).astype(f32)


@pytest.fixture(scope="module")
def trajectory():
    """thirteen VLP-16 frames: the oracle front end's features, down-sampled at 0.2 / 0.4 as the reference's key frames are (downsampleCurrentScan)"""
    out = []
    for k in range(13):
        R, t, pose = frame_pose(k)
        c, s = features(R, t, synth.SEED + k)
        out.append((pyorc.voxelgrid(c, CORNER_LEAF), pyorc.voxelgrid(s, SURF_LEAF), pose, 0.5 * k))
    return out


def oracle_extract(frames, poses, indices, corner_leaf=CORNER_LEAF, surf_leaf=SURF_LEAF):
    cc, ss = [np.zeros((0, 4), f32)], [np.zeros((0, 4), f32)]
    for k in indices:
        p = [float(v) for v in poses[k]]
        T = pyorc.get_transformation(p[3], p[4], p[5], p[0], p[1], p[2])
        for dst, cloud in ((cc, frames[k][0]), (ss, frames[k][1])):
            if len(cloud):
                # the coordinates through the oracle's transform (on the n x 3 block: handed n x 4 records it takes slot 3 for the homogeneous w and
                # writes 1 there), the intensity copied as transformPointCloud :317 does
                moved = cloud.copy()
                moved[:, :3] = pyorc.transform_cloud_f(np.ascontiguousarray(cloud[:, :3]), T)
                dst.append(moved)
    cc = np.concatenate(cc); ss = np.concatenate(ss)
    return pyorc.voxelgrid(cc, corner_leaf), pyorc.voxelgrid(ss, surf_leaf), cc, ss


def filled_keymap(trajectory, n=12):
    km = KeyFrameMap()
    for k in range(n):
        c, s, pose, tm = trajectory[k]
        assert km.addKeyFrame(c, s, pose, tm) == k
    return km


# ---- 1. the voxel filter ---------------------------------------------------------------------------------------------------------------------------------

def _clouds(trajectory):
    rng = np.random.default_rng(11)
    corner263, _ = features(np.eye(3), np.zeros(3), synth.SEED)
    poses = [fr[2] for fr in trajectory]
    _, _, _, fused_surf = oracle_extract(trajectory, poses, range(12))
    n = 1_500_000
    uniform = np.concatenate([rng.uniform(-60, 60, (n, 2)), rng.uniform(-3, 8, (n, 1)), rng.uniform(0, 100, (n, 1))], axis=1).astype(f32)
    negative = (-rng.uniform(5, 40, (20000, 4))).astype(f32)
    one_cell = np.concatenate([rng.uniform(0.01, 0.19, (5000, 3)) + np.array([4.0, -2.0, 1.0]), rng.uniform(0, 1, (5000, 1))], axis=1).astype(f32)
    dup = np.repeat(rng.uniform(-10, 10, (700, 4)).astype(f32), 3, axis=0)[rng.permutation(2100)]
    base = {
        "n0": np.zeros((0, 4), f32), "n1": uniform[:1].copy(), "n2": uniform[:2].copy(),
        "vlp16_corner_263": corner263, "fused_surface_80k": fused_surf, "uniform_1p5M": uniform, "all_negative": negative,
        "one_cell_5000": one_cell, "exact_duplicates": dup,
        "too_many_cells": np.array([[0, 0, 0, 1], [3000, 3000, 3000, 2], [1, 1, 1, 3]], f32),
    }
    return base, rng


def _lattice(leaf, rng):
    k = rng.integers(-40, 40, (6000, 3))
    return np.concatenate([(k.astype(f32) * f32(leaf)).astype(f32), rng.uniform(0, 1, (6000, 1)).astype(f32)], axis=1)


@pytest.mark.parametrize("leaf", [0.2, 0.4, 2.0])
def test_downsample_equals_the_oracles_voxelgrid(trajectory, leaf):
    clouds, rng = _clouds(trajectory)
    clouds["lattice_corners"] = _lattice(leaf, rng)
    assert clouds["vlp16_corner_263"].shape[0] == 263
    km = KeyFrameMap()
    for name, pts in clouds.items():
        want = pyorc.voxelgrid(pts, leaf)
        got = km.downsample(pts, leaf)
        again = km.downsample(pts, leaf)
        print(f"leaf {leaf} {name}: {len(pts)} -> {len(want)} cells (gpu {len(got)})")
        assert got.shape == want.shape and np.array_equal(got, want), name
        assert got.tobytes() == again.tobytes(), name
    assert len(pyorc.voxelgrid(clouds["too_many_cells"], leaf)) == 3          # PCL's "leaf size is too small": copied through
    assert len(pyorc.voxelgrid(clouds["one_cell_5000"], leaf)) == 1            # the long run: 5 000 points, one serial chain
    km.close()


def test_downsample_of_four_million_points():
    """the header promises ROLO_KEYMAP_MAX_POINTS (2^26); at least 4 M must work: 4.2 M points of a 100 m x 100 m x 12 m block at the surface leaf"""
    rng = np.random.default_rng(3)
    n = 4_200_000
    pts = np.concatenate([rng.uniform(-50, 50, (n, 2)), rng.uniform(-2, 10, (n, 1)), rng.uniform(0, 255, (n, 1))], axis=1).astype(f32)
    km = KeyFrameMap()
    want = pyorc.voxelgrid(pts, SURF_LEAF)
    got = km.downsample(pts, SURF_LEAF)
    print(f"{n} -> {len(want)} cells (gpu {len(got)})")
    assert got.shape == want.shape and np.array_equal(got, want)
    km.close()


def test_downsample_refuses_non_finite_points():
    from rolo_amd._lib import RoloError
    km = KeyFrameMap()
    pts = np.ones((100, 4), f32); pts[37, 1] = np.nan
    with pytest.raises(RoloError) as ei:
        km.downsample(pts, 0.4)
    assert ei.value.code == -11
    pts[37, 1] = 1.0
    assert len(km.downsample(pts, 0.4)) == 1                                   # and the key map works on
    km.close()


# ---- 2. extractCloud -------------------------------------------------------------------------------------------------------------------------------------

def check_extract(km, frames, poses, indices):
    wc, ws, cc, ss = oracle_extract(frames, poses, indices)
    mc, ms = km.extractCloud(indices)
    gc, gs = km.submap()
    print(f"extract {len(indices)} frames: corner {len(cc)} -> {len(wc)} (gpu {mc}), surface {len(ss)} -> {len(ws)} (gpu {ms})")
    assert (mc, ms) == (len(wc), len(ws))
    assert np.array_equal(gc, wc) and np.array_equal(gs, ws)
    return gc, gs


def test_extract_cloud_equals_the_oracle_composition(trajectory):
    poses = [fr[2].copy() for fr in trajectory]
    km = filled_keymap(trajectory)
    check_extract(km, trajectory, poses, list(range(12)))
    check_extract(km, trajectory, poses, [3, 4, 4, 5, 3])                      # a repeated index: its cloud goes in twice
    check_extract(km, trajectory, poses, [11, 2, 7, 0, 9, 5])                  # not ascending
    check_extract(km, trajectory, poses, [4, 5])                               # a smaller list, then a larger one
    check_extract(km, trajectory, poses, list(range(2, 12)))
    check_extract(km, trajectory, poses, [])                                   # nothing listed: two empty sub-maps
    # correctPoses: two frames move; the next extraction equals a fresh computation with the new poses
    for k, d in ((3, [0.001, -0.002, 0.01, 0.08, -0.05, 0.02]), (8, [-0.002, 0.001, -0.015, -0.06, 0.04, 0.01])):
        poses[k] = (poses[k] + np.array(d, f32)).astype(f32)
        km.setPose(k, poses[k])
    a = check_extract(km, trajectory, poses, list(range(12)))
    fresh = KeyFrameMap()
    for k in range(12):
        fresh.addKeyFrame(trajectory[k][0], trajectory[k][1], poses[k], trajectory[k][3])
    b = check_extract(fresh, trajectory, poses, list(range(12)))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    fresh.close(); km.close()


def test_extract_cloud_with_an_empty_corner_cloud(trajectory):
    frames = [list(fr) for fr in trajectory[:6]]
    frames[2][0] = np.zeros((0, 4), f32)
    poses = [fr[2] for fr in frames]
    km = KeyFrameMap()
    for c, s, pose, tm in frames:
        km.addKeyFrame(c, s, pose, tm)
    check_extract(km, frames, poses, [0, 1, 2, 3, 4, 5])
    check_extract(km, frames, poses, [2])
    km.close()


def test_extract_cloud_after_many_small_key_frames():
    """past the reference's cache-clear size (laserCloudMapContainer.size() > 1000): 1 100 key frames, the list over the last 60"""
    rng = np.random.default_rng(5)
    frames, poses = [], []
    km = KeyFrameMap()
    for k in range(1100):
        c = np.concatenate([rng.uniform(-3, 3, (7 + k % 5, 3)), rng.uniform(0, 1, (7 + k % 5, 1))], axis=1).astype(f32)
        s = np.concatenate([rng.uniform(-5, 5, (40 + k % 11, 3)), rng.uniform(0, 1, (40 + k % 11, 1))], axis=1).astype(f32)
        pose = np.array([0.01 * np.sin(k), 0.01 * np.cos(k), 0.002 * k, 0.05 * k, 0.01 * k, 0.0], f32)
        frames.append((c, s, pose, 0.1 * k)); poses.append(pose)
        assert km.addKeyFrame(c, s, pose, 0.1 * k) == k
    assert len(km) == 1100
    check_extract(km, frames, poses, list(range(1040, 1100)))
    km.close()


# ---- 3. hand-over to the registration ---------------------------------------------------------------------------------------------------------------------

def scan_and_guess(trajectory):
    corner, surf, truth, _ = trajectory[12]
    guess = (truth + np.array([0.004, -0.003, 0.01, 0.06, -0.04, 0.02], f32)).astype(f32)
    return corner, surf, truth, guess


def test_set_submap_from_keymap_equals_the_uploaded_submap(trajectory):
    corner, surf, _, guess = scan_and_guess(trajectory)
    km = filled_keymap(trajectory)
    km.extractCloud(list(range(12)))
    a, b = Scan2Map(), Scan2Map()
    a.setSubmapFrom(km)
    tf_a, sel_a, co_a = a.scan2MapOptimization(corner, surf, None, None, guess, want_debug=True)
    b.setSubmap(*km.submap())
    tf_b, sel_b, co_b = b.scan2MapOptimization(corner, surf, None, None, guess, want_debug=True)
    sa, sb = a.last_stats, b.last_stats
    assert sa.skipped == 0 and sa.iterations >= 1
    assert (sa.skipped, sa.iterations, sa.converged, sa.degenerate, sa.n_selected) == (sb.skipped, sb.iterations, sb.converged, sb.degenerate, sb.n_selected)
    assert tf_a.tobytes() == tf_b.tobytes() and np.array_equal(sel_a, sel_b) and co_a.tobytes() == co_b.tobytes()
    # a second extraction and hand-over into the same context: again the same bits as the upload route
    km.extractCloud([6, 7, 8, 9, 10, 11])
    a.setSubmapFrom(km); b.setSubmap(*km.submap())
    r_a = a.scan2MapOptimization(corner, surf, None, None, guess, want_debug=True)
    r_b = b.scan2MapOptimization(corner, surf, None, None, guess, want_debug=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(r_a, r_b)) and a.last_stats.iterations == b.last_stats.iterations
    # a surface sub-map with fewer than five points: nothing to search, skipped = 2, the pose untouched
    tiny = KeyFrameMap()
    tiny.addKeyFrame(trajectory[0][0], trajectory[0][1][:3], trajectory[0][2], 0.0)
    assert tiny.extractCloud([0])[1] < 5
    a.setSubmapFrom(tiny)
    tf = a.scan2MapOptimization(corner, surf, None, None, guess)
    assert a.last_stats.skipped == 2 and np.array_equal(tf, guess)
    for x in (a, b, km, tiny):
        x.close()


def test_set_submap_from_keymap_needs_an_extraction(trajectory):
    from rolo_amd._lib import RoloError
    km = filled_keymap(trajectory, 2)
    g = Scan2Map()
    with pytest.raises(RoloError) as ei:
        g.setSubmapFrom(km)
    assert ei.value.code == -5
    g.close(); km.close()


# ---- 4. the whole chain -----------------------------------------------------------------------------------------------------------------------------------

def test_select_extract_handover_optimise_recovers_the_pose(trajectory):
    raw_c, raw_s = features(*frame_pose(12)[:2], synth.SEED + 12)
    _, _, truth, guess = scan_and_guess(trajectory)
    km = filled_keymap(trajectory)
    corner, surf = km.downsample(raw_c, CORNER_LEAF), km.downsample(raw_s, SURF_LEAF)       # downsampleCurrentScan
    assert np.array_equal(corner, trajectory[12][0]) and np.array_equal(surf, trajectory[12][1])
    idx = km.selectNearby(time_cur=0.5 * 12)
    assert set(idx.tolist()) <= set(range(12)) and len(idx) >= 12                          # everything is within 50 m and 10 s: radius hits and recent poses
    mc, ms = km.extractCloud(idx)
    wc, ws, _, _ = oracle_extract(trajectory, [fr[2] for fr in trajectory], idx.tolist())
    gc, gs = km.submap()
    assert np.array_equal(gc, wc) and np.array_equal(gs, ws)
    g = Scan2Map()
    g.setSubmapFrom(km)
    tf = g.scan2MapOptimization(corner, surf, None, None, guess)
    st = g.last_stats
    print("chain:", len(idx), "listed,", mc, "+", ms, "sub-map points, iterations", st.iterations, "error", np.abs(tf - truth))
    assert st.skipped == 0 and st.converged == 1
    assert np.abs(tf[3:] - truth[3:]).max() < 0.03 and np.abs(tf[:3] - truth[:3]).max() < 3e-3
    assert np.abs(guess[3:] - truth[3:]).max() > 0.05
    g.close(); km.close()
