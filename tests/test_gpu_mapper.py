"""GPU: the mapping node's per-scan step as one call (rolo_mapper_scan, rolo_amd/csrc/mapper.hip; MapOptimization in rolo_amd/backend.py) against the same step
composed call by call from the public pieces it is made of: KeyFrameMap.downsample / selectNearby / extractCloud, Scan2Map.setSubmapFrom / scan2MapOptimization,
addKeyFrame, PoseGraph, scAddSurface and the three host-only rolo_mapper_* functions (class Route below). Every comparison is of bytes.
The scans are the VLP-16 trajectory of tests/test_gpu_keymap.py, restated here: 13 frames, 16 x 1800, the oracle front end's features, 0.6 m apart, 0.5 s apart."""
import math

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from oracle import pyorc
from rolo_amd import synth
from rolo_amd._lib import RoloError
from rolo_amd.backend import (KeyFrameMap, Scan2Map, PoseGraph, MapOptimization, mapper_params, mapper_initial_guess, mapper_save_frame, mapper_incremental, select_nearby)

pytestmark = pytest.mark.gpu

CFG = dict(n_scan=16, horizon_scan=1800)
CORNER_LEAF, SURF_LEAF, DENSITY = 0.2, 0.4, 2.0
f32 = np.float32
IDENT12 = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], f32)
N_SCANS = 13


def frame_pose(k):
    R = synth.rpy_to_R(0.002 * k, -0.001 * k, 0.03 * k)
    t = np.array([0.6 * k, 0.05 * k, 0.0])
    return R, t, np.concatenate([Rotation.from_matrix(R).as_euler("xyz"), t]).astype(f32)


@pytest.fixture(scope="module")
def scans():
    """per scan: (stamp, extracted corner cloud, extracted surface cloud, cloud_projected as n x 4, the front end's pose as the odometry guess)"""
    fo = pyorc.front_params(**CFG)
    out = []
    for k in range(N_SCANS):
        R, t, pose = frame_pose(k)
        fr = synth.make_frame("vlp16", R, t, synth.SEED + k)
        e = pyorc.extract_features(fo, pyorc.project(fo, fr.xyz, fr.ring))
        raw = np.concatenate([fr.xyz.astype(f32), fr.ring.astype(f32)[:, None]], axis=1)
        out.append((0.5 * k, e["corner"], e["surface"], np.ascontiguousarray(raw), pose))
    return out


def params(**kw):
    return mapper_params(mappingSurfLeafSize=SURF_LEAF, surroundingKeyframeDensity=DENSITY, **kw)


# ---- the graph's measurements in double, in the library's operation order (mapper.hip: T16_of_rpyxyz, T16_between), with libm's cos / sin ----
def T16_of_pose(p):
    r, q, y = float(p[0]), float(p[1]), float(p[2])
    A, B, C, D, E, F = math.cos(y), math.sin(y), math.cos(q), math.sin(q), math.cos(r), math.sin(r)
    DE, DF = D * E, D * F
    return [[A * C, A * DF - B * E, B * F + A * DE, float(p[3])], [B * C, A * E + B * DF, B * DE - A * F, float(p[4])], [-D, C * F, C * E, float(p[5])], [0.0, 0.0, 0.0, 1.0]]


def T16_between(Fm, Tm):
    d = [Tm[0][3] - Fm[0][3], Tm[1][3] - Fm[1][3], Tm[2][3] - Fm[2][3]]
    Z = [[0.0] * 4 for _ in range(4)]
    for i in range(3):
        for j in range(3):
            Z[i][j] = Fm[0][i] * Tm[0][j] + Fm[1][i] * Tm[1][j] + Fm[2][i] * Tm[2][j]
        Z[i][3] = Fm[0][i] * d[0] + Fm[1][i] * d[1] + Fm[2][i] * d[2]
    Z[3][3] = 1.0
    return Z


class Route:
    """laserCloudInfoHandler :420-457 call by call, every cloud through the host; its sub-map is rebuilt every scan"""

    def __init__(self, P):
        self.P = P
        self.km = KeyFrameMap(0, P.mappingCornerLeafSize, P.mappingSurfLeafSize)
        self.s2m = Scan2Map(0, P.edgeFeatureMinValidNum, P.surfFeatureMinValidNum)
        self.g = PoseGraph()
        self.tf = np.zeros(6, f32); self.time_last = -1.0
        self.last12, self.avail = IDENT12.copy(), False
        self.front6 = np.zeros(6, f32); self.back6 = np.zeros(6, f32)
        self.inc, self.started = IDENT12.copy(), False
        self.loops = []
        self.frames = []   # the key frames' clouds, for oracle_extract

    def close(self):
        for x in (self.s2m, self.g, self.km):
            x.close()

    def scan(self, stamp, corner, surf, guess=None):
        P, km = self.P, self.km
        r = dict(processed=False)
        if not (stamp - self.time_last >= P.mappingProcessInterval):
            return r
        self.time_last = stamp
        have = len(km) > 0
        self.front6 = self.tf.copy()
        self.tf, self.last12, self.avail = mapper_initial_guess(self.tf, have, guess, self.last12, self.avail)
        r.update(processed=True, s2m_ran=have, s2m=(0, 0, 0, 0, 0), sub=None, keyframe=-1, loops_added=0, poses_corrected=False, desc=None)
        if have:
            idx = km.selectNearby(stamp, P.surroundingKeyframeSearchRadius, P.surroundingKeyframeDensity, 10.0)
            km.extractCloud(idx)
            r["sub"] = km.submap()
            self.s2m.setSubmapFrom(km)
        cds, sds = km.downsample(corner, P.mappingCornerLeafSize), km.downsample(surf, P.mappingSurfLeafSize)
        r["ds"] = (cds, sds)
        if have:
            self.tf = self.s2m.scan2MapOptimization(cds, sds, None, None, self.tf)
            s = self.s2m.last_stats
            r["s2m"] = (s.skipped, s.iterations, s.converged, s.degenerate, s.n_selected)
            if s.skipped != 1:   # transformUpdate; the tolerances are FLT_MAX
                self.back6 = self.tf.copy()
        if mapper_save_frame(km.poses[-1] if have else None, self.tf, P.surroundingkeyframeAddingDistThreshold, P.surroundingkeyframeAddingAngleThreshold):
            K = len(km)
            To = T16_of_pose(self.tf)
            assert self.g.addPose(To) == K
            if K == 0:
                self.g.addPrior(0, To, PoseGraph.PRIOR_VARIANCES)
            else:
                self.g.addBetween(K - 1, K, T16_between(T16_of_pose(km.poses[-1]), To), PoseGraph.ODOM_VARIANCES)
            for i, j, Z, var, k in self.loops:
                self.g.addBetween(i, j, Z, var, cauchy=k)
            r["loops_added"] = len(self.loops)
            r["pgo"] = self.g.optimize()
            p6 = self.g.poses6()
            self.tf = p6[K].copy()
            r["poses6"] = p6.copy()
            assert km.addKeyFrame(cds, sds, self.tf, stamp) == K
            self.frames.append((cds, sds))
            r["desc"] = km.scDescriptor(km.scAddSurface(K))
            r["keyframe"] = K
            if self.loops:
                km.setPoses(p6)
                r["poses_corrected"] = True
            self.loops = []
        self.inc, r["incremental6"] = mapper_incremental(self.front6, self.back6, self.tf, self.started, self.inc)
        self.started = True
        r["transformTobeMapped"] = self.tf.copy()
        return r


def same_bytes(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def compare_scan(m, got, want, k):
    """one scan of the mapper `m` (its result dict `got`) against the route's record `want`"""
    assert got["processed"] == want["processed"], k
    if not want["processed"]:
        return
    assert same_bytes(got["transformTobeMapped"], want["transformTobeMapped"]), (k, got["transformTobeMapped"], want["transformTobeMapped"])
    assert got["s2m_ran"] == want["s2m_ran"] and got["s2m"] == want["s2m"], (k, got["s2m"], want["s2m"])
    c, s = m.lastScan()
    assert same_bytes(c, want["ds"][0]) and same_bytes(s, want["ds"][1]), k
    assert (got["n_corner_ds"], got["n_surf_ds"]) == (len(c), len(s))
    if want["s2m_ran"]:
        assert (got["m_corner"], got["m_surf"]) == (len(want["sub"][0]), len(want["sub"][1])), k
        gc, gs = m.keymap.submap()
        assert same_bytes(gc, want["sub"][0]) and same_bytes(gs, want["sub"][1]), k
    assert got["keyframe"] == want["keyframe"], k
    assert same_bytes(got["incremental6"], want["incremental6"]), (k, got["incremental6"], want["incremental6"])
    assert got["loops_added"] == want["loops_added"] and got["poses_corrected"] == want["poses_corrected"], k
    if want["keyframe"] >= 0:
        assert got["sc_index"] == want["keyframe"]
        for a, b in zip(m.keymap.scDescriptor(got["sc_index"]), want["desc"]):
            assert same_bytes(a, b), k
        assert got["pgo"] == want["pgo"], (k, got["pgo"], want["pgo"])
    else:
        assert got["sc_index"] == -1


def compare_keyframes(m, route):
    poses, times = m.keyPoses()
    assert len(poses) == len(route.km) == len(m.keymap) and len(m.graph) == len(route.g)
    assert same_bytes(poses, np.array(route.km.poses, f32).reshape(-1, 6)) and list(times) == list(route.km.times)
    assert same_bytes(m.graph.poses(), route.g.poses())
    for k in range(len(poses)):   # the clouds, read back through the unfiltered export at the (equal) poses
        assert same_bytes(m.keymap.globalCloud([k]), route.km.globalCloud([k])), k


def run_route(scans, P, loop_after=None):
    route, rec = Route(P), []
    for k, (stamp, c, s, _, pose) in enumerate(scans):
        rec.append(route.scan(stamp, c, s, pose))
        if loop_after is not None and k == loop_after:
            for args in loop_factors(route.km.poses):
                route.loops.append(args)
    return route, rec


def loop_factors(poses):
    """a plain and a Cauchy loop factor from the newest key to key 0, each 0.3 m off what the poses say"""
    n = len(poses) - 1
    Z = np.linalg.inv(np.array(T16_of_pose(poses[n]))) @ np.array(T16_of_pose(poses[0]))
    Z[0, 3] += 0.3
    var = np.full(6, 0.05)
    return [(n, 0, Z.copy(), var, None), (n, 0, Z.copy(), var, 1.0)]


@pytest.fixture(scope="module")
def route_default(scans):
    route, rec = run_route(scans, params())
    yield route, rec
    route.close()


@pytest.fixture(scope="module")
def route_every(scans):
    route, rec = run_route(scans, params(surroundingkeyframeAddingDistThreshold=0.5), loop_after=10)
    yield route, rec
    route.close()


# ---- 1. the step equals the call-by-call route ---------------------------------------------------------------------------------------------------------

def test_step_equals_the_route_with_default_thresholds(scans, route_default):
    route, rec = route_default
    m = MapOptimization(0, params())
    kept = 0
    for k, (stamp, c, s, _, pose) in enumerate(scans):
        got = m.scan(stamp, c, s, initialGuess=pose)
        compare_scan(m, got, rec[k], k)
        kept += int(got["s2m_ran"] and not got["submap_rebuilt"])
        print(k, "key", got["keyframe"], "s2m", got["s2m"], "rebuilt", got["submap_rebuilt"], "listed", got["n_listed"], "ms", np.round(m.lastMs(), 3))
    assert [r["keyframe"] for r in rec] == [0, -1, 1, -1, 2, -1, 3, -1, 4, -1, 5, -1, 6]   # 0.6 m steps against 1.0 m: every second scan
    assert kept >= 1                                                                       # the route rebuilds every scan; the mapper keeps what has not changed
    err = np.abs(rec[-1]["transformTobeMapped"] - scans[-1][4])
    print("converged", sum(r["s2m"][2] for r in rec), "of 12; last pose against the truth:", err)
    assert sum(r["s2m"][2] for r in rec) >= 1                                              # and the registrations are real ones
    compare_keyframes(m, route)
    m.close()


def test_step_equals_the_route_when_every_scan_is_saved_and_a_loop_closes(scans, route_every):
    """distance threshold 0.5: every scan becomes a key frame. After scan 10 a plain and a Cauchy loop factor are queued (test 4 of the issue rides on this run)"""
    route, rec = route_every
    m = MapOptimization(0, params(surroundingkeyframeAddingDistThreshold=0.5))
    for k, (stamp, c, s, _, pose) in enumerate(scans):
        got = m.scan(stamp, c, s, initialGuess=pose)
        compare_scan(m, got, rec[k], k)
        if k == 10:
            for i, j, Z, var, cauchy in loop_factors(list(m.keyPoses()[0])):
                m.queueLoopBetween(i, j, Z, var, cauchy)
        if k == 11:   # the next key frame takes both factors, and correctPoses writes the graph's poses into the key map
            assert got["loops_added"] == 2 and got["poses_corrected"] and got["keyframe"] == 11
            corrected, times = m.keyPoses()
            assert same_bytes(corrected, rec[11]["poses6"])
            before = np.array(rec[10]["poses6"], f32)
            print("the loop moved key 10 by", np.abs(corrected[10, 3:] - before[10, 3:]).max(), "m")
            assert np.abs(corrected[:11] - before).max() > 1e-3   # two 0.3 m loops against eleven tight odometry factors: the poses do move
        if k == 12:   # the sub-map this scan registered against is the oracle's extraction at the corrected poses
            assert got["submap_rebuilt"]
            idx = select_nearby(corrected[:, 3:6], times, stamp, 50.0, DENSITY, 10.0)
            wc, ws = oracle_extract(route.frames, corrected, idx.tolist())
            gc, gs = m.keymap.submap()
            assert same_bytes(gc, wc) and same_bytes(gs, ws)
    assert [r["keyframe"] for r in rec] == list(range(N_SCANS))
    assert rec[11]["pgo"]["iterations"] >= 1   # the loop moved the graph
    compare_keyframes(m, route)
    m.close()


def oracle_extract(frames, poses, indices):
    """extractCloud by the CPU oracle, as tests/test_gpu_keymap.py composes it: transformPointCloud of the listed key frames' clouds, concatenated, VoxelGrid"""
    cc, ss = [np.zeros((0, 4), f32)], [np.zeros((0, 4), f32)]
    for k in indices:
        p = [float(v) for v in poses[k]]
        T = pyorc.get_transformation(p[3], p[4], p[5], p[0], p[1], p[2])
        for dst, cloud in ((cc, frames[k][0]), (ss, frames[k][1])):
            if len(cloud):
                dst.append(moved_by(cloud, T))
    return pyorc.voxelgrid(np.concatenate(cc), CORNER_LEAF), pyorc.voxelgrid(np.concatenate(ss), SURF_LEAF)


def moved_by(cloud, T):
    moved = cloud.copy()
    moved[:, :3] = pyorc.transform_cloud_f(np.ascontiguousarray(cloud[:, :3]), T)   # the intensity is copied, as transformPointCloud :317 does
    return moved


# ---- 2. device clouds -------------------------------------------------------------------------------------------------------------------------------------

def test_device_clouds_give_the_bytes_of_host_clouds(scans, route_default):
    import torch
    _, rec = route_default
    m = MapOptimization(0, params())
    dev = torch.device("cuda", 0)
    for k, (stamp, c, s, raw, pose) in enumerate(scans):
        got = m.scan(stamp, torch.from_numpy(c).to(dev), torch.from_numpy(s).to(dev), raw=torch.from_numpy(raw).to(dev), initialGuess=pose)
        compare_scan(m, got, rec[k], k)
    m.close()


# ---- 3. gates ---------------------------------------------------------------------------------------------------------------------------------------------

def test_interval_gate_holds_scans_back_and_changes_nothing(scans):
    m = MapOptimization(0, params())
    processed = []
    for k in range(6):   # stamps 0.1 s apart against 0.15 s: every second scan
        _, c, s, _, pose = scans[k]
        before = None
        if k:
            before = (m.lastScan(), m.registered(), m.keyPoses(), m.graph.size(), len(m.keymap), m.keymap.scSize())
        got = m.scan(0.1 * k, c, s, initialGuess=pose)
        processed.append(got["processed"])
        if not got["processed"]:
            assert set(got) >= {"processed"} and got["keyframe"] == -1
            after = (m.lastScan(), m.registered(), m.keyPoses(), m.graph.size(), len(m.keymap), m.keymap.scSize())
            assert all(same_bytes(a, b) for a, b in zip(before[0] + (before[1],) + before[2], after[0] + (after[1],) + after[2])) and before[3:] == after[3:]
    assert processed == [True, False, True, False, True, False]
    m.close()


def test_first_scan_and_a_scan_with_too_few_corners(scans, route_default):
    P = params()
    m, route = MapOptimization(0, P), Route(P)
    out = []
    for k in range(5):
        stamp, c, s, _, pose = scans[k]
        if k == 4:
            c = c[:40:8].copy()   # five corner points: n_corner_ds <= edgeFeatureMinValidNum
        want = route.scan(stamp, c, s, pose)
        tf_before = m.last["transformTobeMapped"].copy() if k else None
        got = m.scan(stamp, c, s, initialGuess=pose)
        compare_scan(m, got, want, k)
        out.append(got)
    # the first scan: no registration, and key frame 0 has roll = pitch = yaw = 0 (:524-531)
    assert not out[0]["s2m_ran"] and out[0]["keyframe"] == 0 and np.array_equal(m.keyPoses()[0][0, :3], np.zeros(3, f32))
    # the thin scan: skipped, the pose is the guess, the scan still goes through saveFrame (1.2 m behind key 1: saved), and the incremental pose advances by the
    # previous scan's step. Scan 3 was no key frame, so its back pose is its result, which is this scan's front: that step is the identity
    g = out[4]
    assert g["n_corner_ds"] <= 10 and g["s2m"] == (1, 0, 0, 0, 0) and g["keyframe"] == 2
    guess, _, _ = mapper_initial_guess(tf_before, True, scans[4][4], route_last12_before_scan4(scans), True)
    # through the graph and back the translation is exact and an angle moves by at most an ulp of a float below 4
    assert np.array_equal(g["transformTobeMapped"][3:], guess[3:]) and np.abs(g["transformTobeMapped"][:3] - guess[:3]).max() <= 2.0 ** -22
    assert np.linalg.norm(g["transformTobeMapped"][3:] - tf_before[3:]) > 0.5           # the pose moved by the odometry step
    assert np.abs(g["incremental6"] - out[3]["incremental6"]).max() < 1e-3              # the incremental pose did not (an identity step in float at 2 m: below 10^-4)
    m.close(); route.close()


def route_last12_before_scan4(scans):
    """lastOdomTransformation going into scan 4: the affine of scan 3's guess"""
    return mapper_initial_guess(np.zeros(6, f32), True, scans[3][4], IDENT12, False)[1]


# ---- 5. registered clouds ---------------------------------------------------------------------------------------------------------------------------------

def test_registered_clouds_and_the_raw_descriptor(scans):
    m = MapOptimization(0, params(sc_input=2))
    ref = KeyFrameMap(0, CORNER_LEAF, SURF_LEAF)
    for k in range(3):
        stamp, c, s, raw, pose = scans[k]
        got = m.scan(stamp, c, s, raw=raw, initialGuess=pose)
        p = [float(v) for v in got["transformTobeMapped"]]
        T = pyorc.get_transformation(p[3], p[4], p[5], p[0], p[1], p[2])
        cds, sds = m.lastScan()
        assert same_bytes(m.registered(), np.concatenate([moved_by(cds, T), moved_by(sds, T)])), k
        assert same_bytes(m.registeredRaw(len(raw)), moved_by(raw, T)), k
        if got["keyframe"] >= 0:   # scan_raw (:1186-1196): downSizeFilterSC at 0.5, then the descriptor
            want = ref.scDescriptor(ref.scAddCloud(raw, 0.5))
            assert got["sc_index"] == ref.scSize() - 1
            for a, b in zip(m.keymap.scDescriptor(got["sc_index"]), want):
                assert same_bytes(a, b), k
    assert ref.scSize() == 2
    with pytest.raises(RoloError) as ei:   # a scan without a raw cloud has none to register
        m.scan(scans[3][0], scans[3][1], scans[3][2], initialGuess=scans[3][4])
        m.registeredRaw(10)
    assert ei.value.code == -5
    m.close(); ref.close()


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------------------------------

def test_a_nan_scan_leaves_the_mapper_as_it_was(scans, route_default):
    _, rec = route_default
    m = MapOptimization(0, params())
    for k in range(5):
        stamp, c, s, _, pose = scans[k]
        compare_scan(m, m.scan(stamp, c, s, initialGuess=pose), rec[k], k)
    stamp, c, s, _, pose = scans[5]
    bad = s.copy(); bad[len(bad) // 2, 1] = np.nan
    state = (m.keyPoses(), m.graph.size(), m.keymap.scSize())
    with pytest.raises(RoloError) as ei:
        m.scan(stamp, c, bad, initialGuess=pose)
    assert ei.value.code == -11
    after = (m.keyPoses(), m.graph.size(), m.keymap.scSize())
    assert same_bytes(state[0][0], after[0][0]) and state[1:] == after[1:]
    # the same scan clean, and the rest of the run: the bytes of a mapper that never saw the NaN (the route's record)
    for k in range(5, 8):
        stamp, c, s, _, pose = scans[k]
        compare_scan(m, m.scan(stamp, c, s, initialGuess=pose), rec[k], k)
    m.close()
