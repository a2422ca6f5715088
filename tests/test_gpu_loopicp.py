"""GPU: the loop closure on the device (rolo_amd/csrc/loopicp.hip, rolo_keymap_loop_cloud in submap.hip) against the numpy twin (tests/icp_twin.py) and the CPU
oracle. The association is held to the twin's brute force bit for bit (np.array_equal on indices and d2), the 17 sums to numpy's fp64 sums within the
summation bound, whole alignments to the twin's state, iteration count, per-iteration pair counts and pose (BASELINE.json's bars: 1e-4 m, 1e-5 rad), the loop
clouds to pyorc's transform + ONE voxel grid bit for bit."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import icp_twin as T
from oracle import pyorc
from rolo_amd import synth
from rolo_amd._lib import RoloError
from rolo_amd.backend import KeyFrameMap, LoopCloser, LoopIcp, ScanContextManager, loop_icp_params, pose6_to_T
from test_icp_twin import CASES, moved_pair, motion, pose_error, room

pytestmark = pytest.mark.gpu

f32 = np.float32
BAR_M, BAR_RAD = 1e-4, 1e-5   # BASELINE.json


def xyzi(xyz):
    return np.concatenate([np.asarray(xyz, f32)[:, :3], np.zeros((len(xyz), 1), f32)], axis=1)


@pytest.fixture(scope="module")
def icp():
    h = LoopIcp()
    yield h
    h.close()


# ---- 1. association, bit for bit ----------------------------------------------------------------------------------------------------------------------------
def check_association(icp, src, tgt, Tm=None, cap=np.inf):
    moved = src if Tm is None else T.transform(Tm, src)
    want_i, want_d = T.associate(moved, tgt, cap)
    got_i, got_d = icp.associate(xyzi(src), xyzi(tgt), Tm, cap)
    assert np.array_equal(got_i, want_i), np.flatnonzero(got_i != want_i)[:8]
    assert np.array_equal(got_d, want_d)
    return want_i, want_d, moved


@pytest.mark.parametrize("nt", [1, 2, 65, 5000])
@pytest.mark.parametrize("ns", [1, 3, 63, 64, 65, 257, 2000])
def test_association_sizes(icp, ns, nt):
    rng = np.random.default_rng(1000 * ns + nt)
    src = rng.uniform(-10, 10, (ns, 3)).astype(f32); tgt = rng.uniform(-10, 10, (nt, 3)).astype(f32)
    check_association(icp, src, tgt)                                  # cap = inf
    i, d, _ = check_association(icp, src, tgt, motion(), cap=0.7)     # moved on the device; 5000 points in 8000 m^3 are about 0.65 m from a random point: the cap splits them
    if ns >= 257 and nt == 5000:
        assert 0 < (i < 0).sum() < ns


def test_association_planted_equal_distances(icp):
    """every source point sits in the middle of six target points at the same float distance, on a lattice where the differences are exact: the smallest index wins"""
    rng = np.random.default_rng(3)
    c = rng.integers(-20, 20, (300, 3)).astype(f32) * f32(4.0)
    c = np.unique(c, axis=0)
    offs = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32)
    tgt = (c[:, None, :] + offs[None, :, :]).reshape(-1, 3)
    tgt = tgt[rng.permutation(len(tgt))]
    i, d, _ = check_association(icp, c, tgt)
    assert np.all(d == 1.0)
    for k in range(len(c)):   # the winner is the smallest index among the six
        assert i[k] == np.flatnonzero(np.abs(tgt - c[k]).sum(axis=1) == 1.0).min()


def test_association_duplicated_target_points(icp):
    rng = np.random.default_rng(4)
    base = rng.uniform(-5, 5, (400, 3)).astype(f32)
    tgt = np.repeat(base, 3, axis=0)[rng.permutation(1200)]
    src = rng.uniform(-5, 5, (500, 3)).astype(f32)
    i, d, _ = check_association(icp, src, tgt)
    same = np.all(tgt[:, None, :] == tgt[i][None, :, :], axis=2)   # 1200 x 500: the copies of each winner
    assert np.array_equal(i, np.argmax(same, axis=0))               # ... and the winner is the first of them


def test_association_at_the_cap_and_one_float_above(icp):
    tgt = np.array([[2, 0, 0], [100, 2, 6.9e-4]], f32)
    src = np.array([[0, 0, 0], [100, 0, 0]], f32)
    want_i, want_d = T.associate(src, tgt, 2.0)
    assert want_d[0] == f32(4.0) and want_i.tolist() == [0, -1]            # exactly at the cap: kept
    _, raw = T.associate(src, tgt)
    assert raw[1] == np.nextafter(f32(4.0), f32(5.0))                       # one float above: dropped
    check_association(icp, src, tgt, cap=2.0)
    check_association(icp, src, tgt, cap=np.nextafter(2.0, 0.0))            # the cap just below: both dropped
    check_association(icp, src, tgt, cap=2.0000002)                         # just above: both kept


def test_association_all_beyond_the_cap_and_no_cap(icp):
    rng = np.random.default_rng(5)
    src = rng.uniform(-5, 5, (300, 3)).astype(f32); tgt = (rng.uniform(-5, 5, (700, 3)) + np.array([50.0, 0, 0])).astype(f32)
    i, d, _ = check_association(icp, src, tgt, cap=10.0)
    assert np.all(i == -1) and np.all(np.isinf(d))
    i, d, _ = check_association(icp, src, tgt)
    assert np.all(i >= 0)
    assert icp.trace()[-1]["n"] == 300


# ---- 2. the sums ------------------------------------------------------------------------------------------------------------------------------------------------
def test_sums_against_numpy_and_run_to_run(icp):
    rng = np.random.default_rng(6)
    src = rng.uniform(-30, 30, (2000, 3)).astype(f32); tgt = rng.uniform(-30, 30, (5000, 3)).astype(f32)
    i, d, moved = check_association(icp, src, tgt, motion(), cap=3.0)
    terms = T.pair_terms(moved, tgt, i, d)
    got = icp.trace()[-1]["sums"]
    assert 0 < len(terms) < 2000 and got[0] == len(terms)
    bound = 1e-12 * np.abs(terms).sum(axis=0)     # the fp64 summation bound for 2000 terms is about 2e-13 of the sum of magnitudes
    err = np.abs(got - terms.sum(axis=0))
    print("sums: worst error / bound", (err / np.maximum(bound, 1e-300)).max())
    assert np.all(err <= bound)
    icp.associate(xyzi(src), xyzi(tgt), motion(), 3.0)
    assert icp.trace()[-1]["sums"].tobytes() == got.tobytes()


@pytest.mark.parametrize("g", [1, 7, 8, 9, 63, 64, 65])
def test_sums_at_the_row_groups_edges(icp, g):
    """256 g source points are g workgroups, so g rows for the row sum (8 groups of lanes, group q adds rows q, q + 8, ...): fewer rows than groups, one full
    round of the groups with and without a remainder, and 64 rows, where a form of the sum with 8 loads in flight takes its second step. The bound is the one of
    test_sums_against_numpy_and_run_to_run."""
    rng = np.random.default_rng(600 + g)
    src = rng.uniform(-30, 30, (256 * g, 3)).astype(f32); tgt = rng.uniform(-30, 30, (2000, 3)).astype(f32)
    i, d, moved = check_association(icp, src, tgt, motion(), cap=4.0)
    terms = T.pair_terms(moved, tgt, i, d)
    got = icp.trace()[-1]["sums"]
    assert 0 < len(terms) < len(src) and got[0] == len(terms)
    bound = 1e-12 * np.abs(terms).sum(axis=0)
    err = np.abs(got - terms.sum(axis=0))
    print("g", g, "pairs", len(terms), "sums: worst error / bound", (err / np.maximum(bound, 1e-300)).max())
    assert np.all(err <= bound)
    icp.associate(xyzi(src), xyzi(tgt), motion(), 4.0)
    assert icp.trace()[-1]["sums"].tobytes() == got.tobytes()


def test_buffers_regrown_inside_one_context_keep_the_bits():
    """the context's loop ICP buffers only grow, and what they outgrow is retired, not freed: after a 300-point pair, a 5 000-point pair on the same context
    (every buffer past one and a half times its first size + 256) gives the result, the trace and the 17 association sums of a fresh context; then the small
    pair gives its first bits again"""
    P = loop_icp_params(2.0)
    small, large = moved_pair(n_tgt=300, n_src=300, seed=11)[:2], moved_pair(n_tgt=5000, n_src=5000, seed=12)[:2]
    cap = lambda need: need + need // 2 + 256                          # what a buffer that needed `need` elements holds
    rows = lambda n: ((n + 15) // 16 * 16 + 255) // 256                # workgroups: 256 points each of the source padded to whole leaves of 16
    assert 5000 > cap(300) and 17 * rows(5000) > cap(17 * rows(300))   # the clouds and per-point arrays; the workgroups' rows of 17 sums

    def run(h, pair):
        src, tgt = xyzi(pair[0]), xyzi(pair[1])
        r = h.align(src, tgt, P)
        tr = h.trace()
        idx, d2 = h.associate(src, tgt, motion(), 2.0)
        return (r["T"].tobytes(), np.float64(r["fitness"]).tobytes(), r["converged"], r["iterations"], r["state"], r["n_source"], r["n_target"], r["n_last"],
                [(x["n"], np.float64(x["mse"]).tobytes(), x["sums"].tobytes(), x["increment"].tobytes()) for x in tr],
                idx.tobytes(), d2.tobytes(), h.trace()[-1]["sums"].tobytes())

    g, fresh = LoopIcp(), LoopIcp()
    try:
        first = run(g, small)
        grown = run(g, large)
        want = run(fresh, large)
        assert grown[3] >= 1 and grown[2] and len(grown[8]) == grown[3] + 1
        assert grown == want
        assert run(g, small) == first
    finally:
        g.close(); fresh.close()


def test_alignment_is_bit_reproducible(icp):
    src, tgt, _ = moved_pair()
    P = loop_icp_params(2.0)
    runs = []
    for _ in range(2):
        r = icp.align(xyzi(src), xyzi(tgt), P)
        tr = icp.trace()
        runs.append((r["T"].tobytes(), np.float64(r["fitness"]).tobytes(), r["iterations"], r["state"],
                     b"".join(x["sums"].tobytes() + x["increment"].tobytes() + np.float64(x["mse"]).tobytes() for x in tr), [x["n"] for x in tr]))
    assert runs[0] == runs[1]


def test_single_form_bits_are_the_recorded_ones(golden_dir):
    """LoopIcp.align + trace() on the inputs of test_gpu_loopicp_batch.py's "batch equals single" comparisons (loopicp_bits_cases.py) against the bytes recorded
    on an MI355X at the commit the file's meta names (profiles/tools/record_loopicp_bits.py): the single form was an ICP loop of its own then, so the batch
    tests' comparisons with it say something about a single form that is a batch of one"""
    import os
    import loopicp_bits_cases as rec
    want = np.load(os.path.join(golden_dir, rec.FILE))
    print(str(want["meta"]))
    h = LoopIcp()   # a fresh context, as the recorder's
    try:
        got = rec.run(h)
    finally:
        h.close()
    assert sorted(got) == sorted(k for k in want.files if k != "meta")
    assert got["names"].tolist() == want["names"].tolist() and len(got["names"]) == 2 * 2 * 7 + 2 * 5
    for k in got:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(rec.raw(got[k]), rec.raw(want[k])), (k, np.flatnonzero(np.any((rec.raw(got[k]) != rec.raw(want[k])).reshape(len(got[k]), -1), axis=1))[:8])


# ---- 3. whole alignments against the twin -----------------------------------------------------------------------------------------------------------------------
def against_twin(icp, src, tgt, guess=None, **kw):
    want = T.icp(src, tgt, guess, **kw)
    assert want["margin"] > 1e-3, want["margin"]   # of the test's own inputs: no exit decision of the twin hangs on rounding
    got = icp.align(xyzi(src), xyzi(tgt), loop_icp_params(**kw), guess)
    tr = icp.trace()
    print("state", got["state"], want["state"], "iterations", got["iterations"], want["iterations"], "n", [x["n"] for x in tr], "fitness", got["fitness"], want["fitness"])
    assert got["state"] == want["state"] and got["iterations"] == want["iterations"] and got["converged"] == want["converged"]
    assert [x["n"] for x in tr] == [x["n"] for x in want["trace"]]
    assert got["n_last"] == want["n_last"] and got["n_source"] == len(src) and got["n_target"] == len(tgt)
    dt = np.linalg.norm(got["T"][:3, 3].astype(np.float64) - want["T"][:3, 3])
    dr = T.rot_angle(got["T"][:3, :3].astype(np.float64) @ want["T"][:3, :3].astype(np.float64).T)
    print("pose against the twin: %.3g m %.3g rad" % (dt, dr))
    assert dt <= BAR_M and dr <= BAR_RAD
    assert np.array_equal(got["T"][3], [0, 0, 0, 1])
    if want["trace"][-1]["n"]:
        assert abs(got["fitness"] - want["fitness"]) <= 1e-6 * want["fitness"] + 1e-12
    return got, want


@pytest.mark.parametrize("seed", [1, 7, 21])
def test_alignment_equals_the_twin(icp, seed):
    src, tgt, _ = moved_pair(seed=seed)
    against_twin(icp, src, tgt, max_correspondence_distance=2.0)


def test_alignment_with_a_guess_equals_the_twin(icp):
    src, tgt, M = moved_pair(seed=3, M=motion((0.02, 0.01, 0.4), (1.0, -2.0, 0.1)))
    guess = motion((0.0, 0.0, 0.38), (0.9, -1.9, 0.0)).astype(f32)
    got, _ = against_twin(icp, src, tgt, guess, max_correspondence_distance=2.0)
    dt, dr = pose_error(got["T"], M)
    assert dt < 0.01 and dr < 1e-3   # (the final transform carries the guess)


# ---- 4. exits ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_exit_fewer_than_three_pairs(icp):
    src, tgt, _ = moved_pair()
    got, _ = against_twin(icp, src, tgt, **CASES[T.NO_CORRESPONDENCES])
    assert got["state"] == T.NO_CORRESPONDENCES and not got["converged"] and got["iterations"] == 0 and got["n_last"] < 3
    assert np.array_equal(got["T"], np.eye(4, dtype=f32))
    src3 = np.array([[0, 0, 0], [1, 0, 0], [50, 50, 50]], f32)     # exactly two pairs inside the cap
    tgt3 = np.array([[0.25, 0.25, 0.25], [1.25, 0.25, 0.25], [90, 90, 90]], f32)
    got = icp.align(xyzi(src3), xyzi(tgt3), loop_icp_params(1.0))
    assert got["state"] == T.NO_CORRESPONDENCES and got["n_last"] == 2 and not got["converged"]


@pytest.mark.parametrize("iters", [1, 2])
def test_exit_max_iterations(icp, iters):
    src, tgt, _ = moved_pair()
    got, _ = against_twin(icp, src, tgt, max_correspondence_distance=2.0, max_iterations=iters)
    assert got["state"] == T.ITERATIONS and got["iterations"] == iters and got["converged"]


def test_exit_identical_clouds_stop_on_the_first_iteration(icp):
    tgt = room(1500, 9, 0.01)
    got, _ = against_twin(icp, tgt, tgt, max_correspondence_distance=2.0)
    assert got["iterations"] == 1 and got["state"] == T.TRANSFORM and got["fitness"] < 1e-20
    assert np.allclose(got["T"], np.eye(4), rtol=0, atol=1e-12)


@pytest.mark.parametrize("state", [T.TRANSFORM, T.REL_MSE, T.ABS_MSE])
def test_exit_constructed(icp, state):
    src, tgt, _ = moved_pair(noise=0.0 if state == T.ABS_MSE else 0.01)
    got, _ = against_twin(icp, src, tgt, **CASES[state])
    assert got["state"] == state and got["converged"]


def test_empty_clouds(icp):
    src, tgt, _ = moved_pair()
    for a, b in ((src[:0], tgt), (src, tgt[:0])):
        got = icp.align(xyzi(a), xyzi(b), loop_icp_params(2.0))
        assert got["state"] == T.NO_CORRESPONDENCES and not got["converged"] and got["iterations"] == 0


# ---- 5. truth ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_truth_on_a_synth_scene(icp):
    """a VLP-16 frame of the synthetic hall, thinned at 0.4 m; every third point moved back by a known small motion is the source"""
    fr = synth.make_frame("vlp16", np.eye(3), np.zeros(3), synth.SEED, col_stride=4)
    tgt = pyorc.voxelgrid(xyzi(fr.xyz), 0.4)[:, :3]
    M = motion((0.004, -0.006, 0.02), (0.12, -0.08, 0.03))
    src = ((tgt[::3].astype(np.float64) - M[:3, 3]) @ M[:3, :3]).astype(f32)
    got, want = against_twin(icp, src, tgt, max_correspondence_distance=2.0)
    (dt, dr), (wt, wr) = pose_error(got["T"], M), pose_error(want["T"], M)
    print("truth: device %.3g m %.3g rad, twin %.3g m %.3g rad, %d x %d points" % (dt, dr, wt, wr, len(src), len(tgt)))
    assert dt <= wt + BAR_M and dr <= wr + BAR_RAD


# ---- 6. loop clouds ---------------------------------------------------------------------------------------------------------------------------------------------
LEAF = 0.4


def frame_pose(k):
    R = synth.rpy_to_R(0.002 * k, -0.001 * k, 0.03 * k)
    t = np.array([0.6 * k, 0.05 * k, 0.0])
    return R, t, np.concatenate([Rotation.from_matrix(R).as_euler("xyz"), t]).astype(f32)


@pytest.fixture(scope="module")
def trajectory():
    """seven key frames: five VLP-16 frames' features, one frame without corner points, one without any point"""
    fo = pyorc.front_params(n_scan=16, horizon_scan=1800)
    out = []
    for k in range(7):
        R, t, pose = frame_pose(k)
        fr = synth.make_frame("vlp16", R, t, synth.SEED + k, col_stride=4)
        e = pyorc.extract_features(fo, pyorc.project(fo, fr.xyz, fr.ring))
        c, s = pyorc.voxelgrid(e["corner"], 0.2), pyorc.voxelgrid(e["surface"], 0.4)
        if k == 3: c = c[:0]
        if k == 5: c, s = c[:0], s[:0]
        out.append((c, s, pose, 0.5 * k))
    return out


@pytest.fixture(scope="module")
def keymap(trajectory):
    km = KeyFrameMap()
    for k, (c, s, pose, tm) in enumerate(trajectory):
        assert km.addKeyFrame(c, s, pose, tm) == k
    yield km
    km.close()


def oracle_loop_cloud(frames, poses, key, search_num, wrt_key=None, leaf=LEAF):
    parts = [np.zeros((0, 4), f32)]
    for k in range(key - search_num, key + search_num + 1):
        if k < 0 or k >= len(frames):
            continue
        p = [float(v) for v in poses[k if wrt_key is None else wrt_key]]
        Tm = pyorc.get_transformation(p[3], p[4], p[5], p[0], p[1], p[2])
        for cloud in frames[k][:2]:   # corner, then surface
            if len(cloud):
                moved = cloud.copy()
                moved[:, :3] = pyorc.transform_cloud_f(np.ascontiguousarray(cloud[:, :3]), Tm)
                parts.append(moved)
    cat = np.concatenate(parts)
    return pyorc.voxelgrid(cat, leaf) if len(cat) else cat


@pytest.mark.parametrize("slot,key,num,wrt", [(0, 2, 0, None), (1, 1, 3, None), (1, 6, 2, None), (0, 4, 1, 0), (1, 2, 25, 6), (0, 5, 0, None), (1, 5, 0, 2), (0, 3, 0, None)])
def test_loop_cloud_equals_the_oracle(trajectory, keymap, slot, key, num, wrt):
    """searchNum 0, clipping at key 0 and at the last key, the wrt_key form, empty frames (5 has no point: m = 0; 3 has no corner)"""
    poses = [fr[2] for fr in trajectory]
    want = oracle_loop_cloud(trajectory, poses, key, num, wrt)
    m = keymap.loopCloud(slot, key, num, wrt, LEAF)
    got = keymap.loopCloudPoints(slot, m)
    print(key, num, wrt, "->", m, "points")
    assert m == len(want) and (m > 0) == (key != 5 or num > 0)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_loop_cloud_after_set_pose_and_bad_keys(trajectory):
    km = KeyFrameMap()
    try:
        with pytest.raises(RoloError) as e:                       # no loop cloud has been built in this map
            km.loopIcp(loop_icp_params(2.0))
        assert e.value.code == -5
        assert km.loopCloud(0, 3, 2) == 0                         # an empty store: an empty cloud, whatever the key
        for c, s, pose, tm in trajectory:
            km.addKeyFrame(c, s, pose, tm)
        poses = [fr[2].copy() for fr in trajectory]
        poses[2] = (poses[2] + np.array([0.01, -0.02, 0.3, 1.5, -0.7, 0.2], f32)).astype(f32)
        km.setPose(2, poses[2])
        for wrt in (None, 2):
            want = oracle_loop_cloud(trajectory, poses, 2, 1, wrt)
            m = km.loopCloud(1, 2, 1, wrt, LEAF)
            assert np.array_equal(km.loopCloudPoints(1, m), want)
        for key, wrt in ((1, 7), (1, 100), (7, None), (-1, None)):
            with pytest.raises(RoloError) as e:
                km.loopCloud(0, key, 1, wrt, LEAF)
            assert e.value.code == -1
    finally:
        km.close()


def test_keymap_icp_equals_the_host_route(trajectory, keymap, icp):
    """the resident route (loop clouds -> rolo_keymap_loop_icp) and the host route on the downloaded clouds: the same bits"""
    ms, mt = keymap.loopCloud(0, 4, 0, None, LEAF), keymap.loopCloud(1, 1, 2, None, LEAF)
    src, tgt = keymap.loopCloudPoints(0, ms), keymap.loopCloudPoints(1, mt)
    P = loop_icp_params(60.0)
    a = keymap.loopIcp(P)
    b = icp.align(src, tgt, P)
    assert a["n_source"] == ms and a["n_target"] == mt and a["iterations"] >= 1
    assert a["T"].tobytes() == b["T"].tobytes() and a["fitness"] == b["fitness"] and (a["state"], a["iterations"], a["n_last"]) == (b["state"], b["iterations"], b["n_last"])
    assert [x["sums"].tobytes() for x in keymap.loopTrace()] == [x["sums"].tobytes() for x in icp.trace()]
    assert keymap.loopLastMs()[3] > 0 and keymap.loopLastMs()[4] > 0
    keymap.loopCloud(0, 5, 0, None, LEAF)                         # an empty source: a result, not an error
    e = keymap.loopIcp(P)
    assert e["state"] == T.NO_CORRESPONDENCES and not e["converged"] and e["n_source"] == 0


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------------------------------------------
def scene_pose(k):
    """the loop scene of tests/test_gpu_scancontext.py: an ellipse through the hall, one lap in 60 key frames; frame 70 stands where frame 10 stood, yawed by 48 degrees"""
    kk = 10 if k == 70 else k
    phi = (kk - 10) * 2.0 * np.pi / 60.0
    yaw = 0.01 * kk + (np.deg2rad(48.0) if k == 70 else 0.0)
    return synth.rpy_to_R(0.0, 0.0, yaw), np.array([20.0 * np.cos(phi), 12.0 * np.sin(phi), 0.0])


def test_loop_closure_end_to_end():
    """Key frames 0 .. 70 of the Scan Context test's scene (the frames after the revisit play no part), one second apart, every fourth firing column — at every
    eighth, as that test samples, two scans of one place from headings 48 degrees apart are 0.8 m apart on the far walls and no alignment reaches the fitness
    gate (0.77 on the CPU, against 0.13 here). Poses are relative to key frame 0, as a map that starts at its first key frame has them: the SC form moves both
    clouds by key 0's pose and its yaw guess turns about that origin. Checked on the CPU before the scene was fixed: without a guess (the reference as written)
    the ICP stays in a local minimum 48 degrees off (fitness 0.77), so the LoopCloser takes the guess, with the sign that turns frame 70 onto frame 10."""
    fo = pyorc.front_params(n_scan=16, horizon_scan=1800)
    R0, t0 = scene_pose(0)
    km = KeyFrameMap()
    frames = []
    try:
        sc = ScanContextManager(km)
        for k in range(71):
            Rk, tk = scene_pose(k)
            fr = synth.make_frame("vlp16", Rk, tk, synth.SEED + k, col_stride=4)
            e = pyorc.extract_features(fo, pyorc.project(fo, fr.xyz, fr.ring))
            pose = np.concatenate([Rotation.from_matrix(R0.T @ Rk).as_euler("xyz"), R0.T @ (tk - t0)]).astype(f32)
            frames.append((pyorc.voxelgrid(e["corner"], 0.2), pyorc.voxelgrid(e["surface"], 0.4), pose, float(k)))
            assert km.addKeyFrame(*frames[-1]) == k
            assert sc.makeAndSaveScancontextAndKeys(e["surface"]) == k
        lc = LoopCloser(km, sc_yaw_guess=-1.0)
        got = lc.performSCLoopClosure(sc)
        assert sc.last is not None and sc.last.loop_id == 10
        assert got is not None, lc.last
        cur, pre, pose_from, pose_to, noise = got
        print("SC form:", lc.last["state"], lc.last["iterations"], "iterations, fitness", lc.last["fitness"], "sizes", lc.last["n_source"], lc.last["n_target"], "ms", km.loopLastMs())
        assert (cur, pre) == (70, 10) and lc.last["converged"] and lc.last["fitness"] < lc.fitness_score and noise == f32(lc.last["fitness"])
        assert np.array_equal(pose_to, np.eye(4)) and lc.loopIndexContainer == {70: 10}
        # frame 70 is frame 10 turned by 48 degrees about the sensor: that is what the correction must say
        dyaw = Rotation.from_matrix(pose_from[:3, :3]).as_euler("xyz")[2]
        print("SC form: yaw", np.rad2deg(dyaw), "translation", pose_from[:3, 3])
        assert abs(dyaw - np.deg2rad(48.0)) < 0.05 and np.linalg.norm(pose_from[:3, 3]) < 0.5
        # the RS form finds the same pair by distance (frame 10 and frame 70 are both at distance 0: the smaller index first, and it is 60 s old)
        rs = LoopCloser(km)
        assert km.detect_loop_distance(70.0, 30.0, 30.0) == 10 == T.detect_loop_distance([p[3:6] for p in km.poses], km.times, 70.0, 30.0, 30.0)
        got = rs.performRSLoopClosure(70.0)
        assert got is not None, rs.last
        print("RS form:", rs.last["state"], rs.last["iterations"], "iterations, fitness", rs.last["fitness"], "sizes", rs.last["n_source"], rs.last["n_target"], "ms", km.loopLastMs())
        assert got[:2] == (70, 10) and rs.last["fitness"] < rs.fitness_score
        # tCorrect = T tWrong stays near the stored pose of 70 (it IS where frame 10 stood), poseTo is key 10's pose
        assert np.allclose(got[2], pose6_to_T(km.poses[70], np.float64), atol=0.05) and np.allclose(got[3], pose6_to_T(km.poses[10], np.float64), atol=1e-6)
        assert rs.performRSLoopClosure(70.0) is None                 # key 70 has its loop
    finally:
        km.close()
    # the size gates: thinned clouds are turned down before any ICP (two key frames, searchNum 0: the current one thinned below 300 points, then the earlier one below 1000)
    for thin_cur, thin_pre in ((20, 1), (1, 5)):
        km = KeyFrameMap()
        try:
            for k, step in ((10, thin_pre), (70, thin_cur)):
                c, s, pose, tm = frames[k]
                km.addKeyFrame(c[::step], s[::step], pose, tm)
            n_cur, n_pre = km.loopCloud(0, 1, 0), km.loopCloud(1, 0, 0)
            print("size gates:", n_cur, n_pre)
            assert (n_cur < 300 and n_pre >= 1000) if thin_cur > 1 else (n_cur >= 300 and n_pre < 1000)
            lc = LoopCloser(km, historyKeyframeSearchNum=0)
            assert km.detect_loop_distance(70.0) == 0 and lc.performRSLoopClosure(70.0) is None and lc.last is None
        finally:
            km.close()
