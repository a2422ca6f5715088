"""GPU: long-lived objects against fresh ones. A context, a front end and a pooled context that have seen other cloud sizes, sensors and owners give, byte for
byte, what a context created for the one step gives — no buffer that was outgrown, kept or handed on shows in a result — and a step that needs no larger
buffer than an earlier one allocates nothing (rolo_alloc_count)."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import pyorc
from rolo_amd import synth
from rolo_amd._lib import lib
from rolo_amd.frontend import FrontEnd, deskew_params, front_params
from rolo_amd.odometry import LidarOdometry
from rolo_amd.rotvgicp import RotVGICP

pytestmark = pytest.mark.gpu

SIZES = (700, 9000, 700, 40000, 9000)
GUESS = -np.asarray(synth.PREV_STEP_T, np.float64)


@functools.lru_cache(maxsize=None)
def pair(n):
    """source and target of n points each, thinned evenly from the synthetic VLP-16 pair; the pair has fewer than 40 000 points, so that one step is thinned
    from the OS1-64 pair instead"""
    src, tgt, _ = synth.dense_pair("vlp16")
    if min(src.shape[0], tgt.shape[0]) < n:
        src, tgt, _ = synth.dense_pair("os1-64")
    thin = lambda a: np.ascontiguousarray(a[np.linspace(0, a.shape[0] - 1, n).astype(np.int64)])   # noqa: E731
    return thin(src), thin(tgt)


def alloc_count():
    return int(lib().rolo_alloc_count())


def prepare(g, fused_lm):
    """default parameters but for the POLAR resolution every caller sets (lidarOdometry.cpp:462): the default's zeros leave no voxel inside the key range"""
    g.setPolarResolution(0.175, 0.175, 2.0)
    g.setUseGraph(True); g.setLoadHint(0)
    if fused_lm is not None:
        g.setFusedLm(fused_lm)


def run_step(g, n):
    """three frames on the same pair (the first runs eagerly, the second is captured, the third replayed — the clouds are set again before each, as a frame loop
    does), then the source covariances, the voxel count and the stats. Returns (every result as bytes, rolo_alloc_count after each frame and at the end)."""
    src, tgt = pair(n)
    out, counts = [], []
    for _ in range(3):
        g.setInputTarget(tgt.copy()); g.setInputSource(src.copy())
        g.register_async(None, np.zeros(3), GUESS, GUESS)
        Tf, Td, t = g.register_wait()
        out += [Tf.tobytes(), Td.tobytes(), t.tobytes(), bytes(g.last_stats), bytes(g.last_translation_stats)]
        counts.append(alloc_count())
    out.append(g.getSourceCovariances().tobytes())
    out.append(int(lib().rolo_num_voxels(g._h)))
    out += [bytes(g.last_stats), bytes(g.last_translation_stats)]
    counts.append(alloc_count())
    return out, counts


@functools.lru_cache(maxsize=None)
def fresh_step(n, fused_lm):
    g = RotVGICP(); prepare(g, fused_lm)
    out, _ = run_step(g, n)
    g.close()
    return out


@pytest.mark.parametrize("fused_lm", [None, 0])   # None: the default; 0: pass + controller launches, which size `partials` by the pass grid
def test_one_context_across_sizes(fused_lm):
    g = RotVGICP(); prepare(g, fused_lm)
    largest = 0
    for step, n in enumerate(SIZES):
        before = alloc_count()
        out, counts = run_step(g, n)
        assert counts[0] == counts[1] == counts[2], (step, n, counts)       # the captured and the replayed frame allocate nothing
        if n <= largest:
            assert counts[3] == before, (step, n, before, counts)           # nothing outgrown: the whole step allocates nothing
        largest = max(largest, n)
        ref = fresh_step(n, fused_lm)                                        # (after the counts are taken: creating a context allocates)
        assert len(out) == len(ref)
        for k, (a, b) in enumerate(zip(out, ref)):
            assert a == b, (step, n, k)
    c = g.counters()
    assert c["graph_captures"] >= 1 and c["graph_replays"] >= 1, c           # the captured path did run
    g.close()


def test_pooled_context_across_owners():
    L = lib()
    L.rolo_ctx_pool_clear()
    h = C.c_void_p(); assert L.rolo_ctx_acquire(0, C.byref(h)) == 0
    a = RotVGICP(0, _borrowed=h.value); prepare(a, None)
    out, _ = run_step(a, 9000)
    assert out == fresh_step(9000, None)
    L.rolo_ctx_release(h)
    h2 = C.c_void_p(); assert L.rolo_ctx_acquire(0, C.byref(h2)) == 0
    assert h2.value == h.value
    b = RotVGICP(0, _borrowed=h2.value); prepare(b, None)
    refs = [fresh_step(700, None), fresh_step(9000, None)]
    before = alloc_count()
    outs = [run_step(b, 700)[0], run_step(b, 9000)[0]]
    assert alloc_count() == before                                           # the first owner's buffers serve the second
    for n, out, ref in zip((700, 9000), outs, refs):
        for k, (x, y) in enumerate(zip(out, ref)):
            assert x == y, (n, k)
    L.rolo_ctx_release(h2); L.rolo_ctx_pool_clear()


# ---- front end ------------------------------------------------------------------------------------------------------------------------------------------

CFG = {"vlp16": dict(n_scan=16, horizon_scan=1800), "os1-64": dict(n_scan=64, horizon_scan=1024)}


def thinned(fr, keep):
    """every raw point of `fr` up to an even selection of keep * n of them (firing order kept)"""
    n = fr.xyz.shape[0]
    idx = np.linspace(0, n - 1, max(int(n * keep), 1)).astype(np.int64)
    return synth.Frame(fr.xyz[idx], fr.intensity[idx], fr.ring[idx], fr.time[idx], fr.n_scan, fr.horizon_scan)


def front_step(ctx, sensor, fr, deskew):
    fe = FrontEnd(ctx, front_params(**CFG[sensor]))
    if deskew:
        fe.setDeskew(deskew_params((0.004, -0.006, 0.035), 0.1, 0.0987), fr.time)
    pg = fe.project(fr.xyz, fr.ring, want_range_mat=True)
    eg = fe.extract(pg["n"], debug=True)
    out = dict(pg); out.update(eg)
    return out


def test_one_front_end_across_sensors_and_point_counts():
    vlp = synth.make_frame("vlp16", np.eye(3), np.zeros(3), synth.SEED)
    osf = synth.make_frame("os1-64", np.eye(3), np.zeros(3), synth.SEED)
    third = thinned(vlp, 1.0 / 3.0)
    assert third.xyz.shape[0] < vlp.xyz.shape[0] < osf.xyz.shape[0]
    # (sensor, frame, de-skewed with host times): the image shrinks and grows again, then the point count does — the raw, ring and de-skew-time buffers grow with it
    steps = [("vlp16", vlp, False), ("os1-64", osf, False), ("vlp16", vlp, False), ("vlp16", third, False), ("vlp16", third, True), ("vlp16", vlp, True),
             ("vlp16", vlp, False)]
    ctx = RotVGICP()
    for k, (sensor, fr, dsk) in enumerate(steps):
        got = front_step(ctx, sensor, fr, dsk)
        one = RotVGICP(); ref = front_step(one, sensor, fr, dsk); one.close()
        assert got.keys() == ref.keys() and got["n"] == ref["n"] and got["n"] > 0
        for name in ref:
            assert np.asarray(got[name]).tobytes() == np.asarray(ref[name]).tobytes(), (k, sensor, name)
        if dsk:   # the de-skew did move the points
            plain = front_step(ctx, sensor, fr, False)
            assert np.abs(plain["extracted"][:, :3] - got["extracted"][:, :3]).max() > 1e-3
    ctx.close()


@pytest.mark.parametrize("sensor", ["vlp16", "os1-64"])
def test_fused_odometry_with_rising_point_counts(sensor):
    """five frames of 60 ... 100 % of the sensor's points: the fused driver's staging buffers grow with every frame; counts, states and poses against the staged
    node cores and the oracle chain as test_pipeline_50_frames compares them"""
    cfg = CFG[sensor]
    fo = pyorc.front_params(**cfg); fg = front_params(**cfg)
    oo = pyorc.Odom(pyorc.default_params(polar_resolution=(0.175, 0.175, 2.0)), 0.3)
    staged = LidarOdometry(0, 0.3); fe = FrontEnd(staged.reg, fg)
    fused = LidarOdometry(0, 0.3)
    R = np.eye(3); t = np.zeros(3); frames = []
    for k in range(5):
        frames.append(thinned(synth.make_frame(sensor, R, t, synth.SEED + k), 0.6 + 0.1 * k))
        t = t + R @ np.array([0.3, 0.02 * k, 0.0]); R = R @ synth.rpy_to_R(np.deg2rad(0.3), np.deg2rad(-0.2), np.deg2rad(2.0))
    assert all(a.xyz.shape[0] < b.xyz.shape[0] for a, b in zip(frames, frames[1:]))
    fused.submit(fg, 100.0, frames[0].xyz, frames[0].ring)
    for k, fr in enumerate(frames):
        stamp = 100.0 + 0.1 * k
        if k >= 2:
            oo.backend_odometry(stamp - 0.05); staged.odometryHandler(stamp - 0.05); fused.odometryHandler(stamp - 0.05)
        eo = pyorc.extract_features(fo, pyorc.project(fo, fr.xyz, fr.ring))
        rco, pose_o, R_o, t_o = oo.cloud(stamp, eo["corner"], eo["surface"])
        pg = fe.project(fr.xyz, fr.ring); eg = fe.extract(pg["n"])
        assert np.array_equal(eg["corner"], eo["corner"]) and np.array_equal(eg["surface"], eo["surface"])
        rcs, pose_s, R_s, t_s = staged.cloudHandler(stamp, eg["corner"], eg["surface"])
        if k + 1 < len(frames):
            fused.submit(fg, stamp + 0.1, frames[k + 1].xyz, frames[k + 1].ring)
        rcf, pose_f, R_f, t_f, cnt = fused.collect()
        assert rcs == rcf == rco, (k, rcs, rcf, rco)
        assert cnt == (pg["n"], eg["corner"].shape[0], eg["surface"].shape[0])
        for (p_, R_, t_) in ((pose_s, R_s, t_s), (pose_f, R_f, t_f)):
            assert np.abs(p_[:3] - pose_o[:3]).max() <= 1e-4 and np.abs(p_[3:] - pose_o[3:]).max() <= 1e-5, k
            assert np.abs(R_ - R_o).max() <= 1e-5 and np.abs(t_ - t_o).max() <= 1e-4, k
    staged.close(); fused.close()
