"""GPU: the de-skew step of front.hip — azimuth_flag_kernel, azimuth_time_kernel, deskew_point in ring_scatter_kernel, the time column of unpack_cloud_kernel — on the
constructed clouds of tests/deskew_cases.py. The expectation is pinned on the CPU in test_deskew_cases.py. On every cloud the per-point times and the index of the
point that set halfPassed (rolo_debug_front_times) are the exact statement's, bit for bit — the rule on the correctly rounded float atan2 — and the stored coordinates
of every point lie within the derived bound (deskew_cases.rotation_bound, E = 2 for the device's sinf / cosf) of the float64 statement at that time; the column, the
range and the intensity are the raw point's.

What the planted pairs found: with the device's atan2f (the kernels before they took the angle from the fp64 function) the planted clouds came out on the wrong
side of their threshold — a time off by a scan period, another flag index, or every time of the cloud rescaled — on 27 / 35 / 25 / 40 / 29 / 32 / 30 of the 80 clouds
of thresholds 1 .. 7 (218 of 560), and 445 of the 560 had a time with other bits than the exact statement's; with (float)atan2((double)y, (double)x) none remain of
either. The largest rotation error seen is 2.57 x 2^-24 L1 on the azimuth clouds, 1.89 on the rotation cases (allowed: 15)."""
import numpy as np
import pytest

import deskew_cases as dc
from deskew_cases import F, bits
from rolo_amd import synth
from rolo_amd._lib import CloudLayout, RoloError
from rolo_amd.frontend import FrontEnd, deskew_params, front_params
from rolo_amd.odometry import LidarOdometry
from rolo_amd.rotvgicp import RotVGICP

pytestmark = pytest.mark.gpu

ROT = dc.ROTATIONS[0]            # a large increment: any difference in a time moves the point
DEVICE_BOUND = 5 * dc.DEVICE_TRIG_ULPS + 5


@pytest.fixture(scope="module")
def built():
    return dc.build()


@pytest.fixture(scope="module")
def ctx():
    g = RotVGICP()
    yield g
    g.close()


_FRONT = {}


def front(ctx, cfg):
    key = (id(ctx), cfg["n_scan"])
    if key not in _FRONT:
        _FRONT[key] = FrontEnd(ctx, front_params(**cfg))
    return _FRONT[key]


def dsk(rot, scan_period=dc.SCAN_PERIOD):
    return deskew_params(list(rot["incre_rpy"]), scan_period, rot["odom_time_diff"])


def check_stored(c, pg, stated, title):
    """the projection of a cloud whose points own their pixels: n, column, range and intensity are the raw point's, the coordinates within the bound of `stated`
    (n, 3, raw order); -> the largest error as a multiple of 2^-24 L1"""
    o = c.order
    assert pg["n"] == len(o), (title, pg["n"], len(o))
    assert np.array_equal(pg["point_col_ind"], c.col[o]), title
    assert np.array_equal(bits(pg["point_range"]), bits(dc.float_range(c.xyz)[o])), title
    assert np.array_equal(bits(pg["extracted"][:, 3]), bits(c.ring[o].astype(F) * c.xyz[o, 2])), title
    err = dc.rotation_error(pg["extracted"][:, :3], stated[o], c.xyz[o])
    bad = np.nonzero(~(err <= DEVICE_BOUND))[0]
    assert bad.size == 0, "%s: %d points outside %d x 2^-24 L1 of the float64 statement, the first: raw #%d %r stored %r stated %r (%.1f x)" % (
        title, bad.size, DEVICE_BOUND, o[bad[0]], c.xyz[o[bad[0]]].tolist(), pg["extracted"][bad[0], :3].tolist(), stated[o[bad[0]]].tolist(), err[bad[0]])
    return float(err.max())


def run_azimuth(ctx, c, rot=ROT):
    """de-skew armed without times -> (projection, times, flag index)"""
    fe = front(ctx, c.cfg)
    fe.setDeskewFromCloud(dsk(rot, c.scan_period))
    pg = fe.project(c.xyz, c.ring)
    t, flag = fe.deskewTimes(c.n)
    return pg, t, flag


def check_cloud(ctx, c, rot=ROT):
    pg, t, flag = run_azimuth(ctx, c, rot)
    assert np.array_equal(bits(t), bits(c.exact["times"])) and flag == c.flag, dc.describe(c, t, flag)
    return check_stored(c, pg, dc.deskew_statement(c.xyz, c.exact["times"], rot["incre_rpy"], c.scan_period, rot["odom_time_diff"]), c.title())


@pytest.mark.parametrize("thr", sorted(dc.THRESHOLDS))
def test_planted_thresholds(built, ctx, thr):
    """both clouds of every pair — adjacent floats on either side of the threshold — take the exact statement's side and its bits, kept by the host libm or not"""
    worst = max(check_cloud(ctx, c) for pair in built["planted"][thr] for c in pair)
    print("DESKEW threshold %d [%s]: %d clouds on the exact statement's side, bit for bit; rotation error at most %.2f x 2^-24 L1 (allowed %d)"
          % (thr, dc.THRESHOLDS[thr], 2 * len(built["planted"][thr]), worst, DEVICE_BOUND))


def test_point_orders(built, ctx):
    worst = max(check_cloud(ctx, c, dc.ROTATIONS[j % 3]) for j, c in enumerate(built["orders"]))
    print("DESKEW orders: %d clouds; rotation error at most %.2f x 2^-24 L1 (allowed %d)" % (len(built["orders"]), worst, DEVICE_BOUND))


def test_sizes_and_the_place_of_the_flag(built, ctx):
    """n = 1 .. 1025, the flipping point at a block edge, in the last block, at n - 1, nowhere; the clouds follow each other on one context, so a flag index left
    over from the cloud before (the INT_MAX reset) shows in the clouds that never set it"""
    for c in built["sizes"]:
        check_cloud(ctx, c)
    by = {(c.n, c.exact["flag"]): c for c in built["sizes"]}
    for n, k in ((1025, 1), (1025, None), (2, 1), (2, None), (1025, 255), (1025, 1024), (1025, None)):
        check_cloud(ctx, by[(n, k)])


def test_rotation_cases(built, ctx):
    """handed-over times (0, denormals, up to 1.3 periods, a ramp) with the three increment sets: the bound on every point, the raw bits at time 0"""
    worst = 0.0
    for c in built["rotation"]:
        fe = front(ctx, c.cfg)
        fe.setDeskew(deskew_params(list(c.incre_rpy), c.scan_period, c.odom_time_diff), c.times)
        pg = fe.project(c.xyz, c.ring)
        t, flag = fe.deskewTimes(len(c.xyz))
        assert np.array_equal(bits(t), bits(c.times)) and flag == dc.INT_MAX, c.name
        e = check_stored(c, pg, c.stated, c.name)
        print("DESKEW %s, odom_time_diff %g: rotation error at most %.2f x 2^-24 L1 (allowed %d)" % (c.name, c.odom_time_diff, e, DEVICE_BOUND))
        worst = max(worst, e)
        z = (c.times == 0)[c.order]
        assert z.sum() >= 4 and np.array_equal(bits(pg["extracted"][z, :3]), bits(c.xyz[c.order][z])), c.name
    print("DESKEW rotation: largest error %.2f x 2^-24 L1" % worst)


def test_times_read_back_states(built, ctx):
    """rolo_debug_front_times: ROLO_ESTATE after a projection that was not de-skewed, ROLO_EINVAL for another n"""
    c = built["orders"][0]
    fe = front(ctx, c.cfg)
    fe.project(c.xyz, c.ring)
    with pytest.raises(RoloError) as ei:
        fe.deskewTimes(c.n)
    assert ei.value.code == -5
    fe.setDeskewFromCloud(dsk(ROT))
    fe.project(c.xyz, c.ring)
    with pytest.raises(RoloError) as ei:
        fe.deskewTimes(c.n + 1)
    assert ei.value.code == -1
    fe.deskewTimes(c.n)
    fe.setDeskew(deskew_params(list(ROT["incre_rpy"]), 0.1, 0.1, enabled=False), np.zeros(c.n, F))
    fe.project(c.xyz, c.ring)
    with pytest.raises(RoloError) as ei:
        fe.deskewTimes(c.n)
    assert ei.value.code == -5


# ---- the message route ------------------------------------------------------------------------------------------------------------------
VELODYNE_TIMES = np.array([-0.0, -0.05, 0.03, -1e-45, -0.1, 0.0, -0.099999994, 0.07, -1.17549435e-38, -0.13], F)
OUSTER_TIMES = np.array([0, 2 ** 24 + 1, 99_999_999, 0xFFFFFFFF, 50_000_000, 1, 2 ** 24 + 3, 16_777_216, 123_456_789, 7], np.uint32)


@pytest.fixture(scope="module")
def frame():
    fr = synth.make_frame("vlp16", synth.rpy_to_R(0, 0, 0.4), np.zeros(3), synth.SEED)
    order = np.argsort(-np.arctan2(fr.xyz[:, 1], fr.xyz[:, 0]), kind="stable")      # one sweep, like a spinning sensor
    return np.ascontiguousarray(np.asarray(fr.xyz, F)[order]), np.ascontiguousarray(np.asarray(fr.ring, np.uint16)[order])


def pack(xyz, ring, kind, step):
    """the payload of a sensor_msgs/PointCloud2 with the planted time values, point after point in turn -> (bytes, layout, fabs(time) in seconds as numpy computes
    it). step 22: the drivers' packed records (no alignment); 48: Ouster's padded ones."""
    n = len(ring)
    if kind == "velodyne":
        names, formats = ["x", "y", "z", "intensity", "ring", "time"], ["<f4", "<f4", "<f4", "<f4", "<u2", "<f4"]
        offsets = [0, 4, 8, 12, 16, 18] if step == 22 else [0, 4, 8, 16, 20, 24]
        a = np.zeros(n, np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": step}))
        a["time"] = VELODYNE_TIMES[np.arange(n) % len(VELODYNE_TIMES)]
        rel = np.abs(a["time"])                                                      # deskewCloudInfo :358-359
        L = CloudLayout(step, 0, 4, 8, offsets[4], 2, offsets[5], 1)
    else:
        names, formats = ["x", "y", "z", "intensity", "t", "ring"], ["<f4", "<f4", "<f4", "<f4", "<u4", "u1"]
        offsets = [0, 4, 8, 12, 16, 20] if step == 22 else [0, 4, 8, 16, 20, 26]
        a = np.zeros(n, np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": step}))
        a["t"] = OUSTER_TIMES[np.arange(n) % len(OUSTER_TIMES)]
        rel = np.abs(a["t"].astype(F) * F(1e-9))                                     # dst.time = src.t * 1e-9f (:209): uint32 -> float, a float product
        L = CloudLayout(step, 0, 4, 8, offsets[5], 1, offsets[4], 2)
    a["x"], a["y"], a["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    a["intensity"] = 7.0; a["ring"] = ring
    return a.view(np.uint8).reshape(-1), L, np.ascontiguousarray(rel, F)


def features_of(submit):
    od = LidarOdometry(0, 0.3)
    try:
        submit(od)
        rc, _, _, _, counts = od.collect()                                          # the driver's first frame only stores its features
        assert rc == 0
        return od.features(), counts
    finally:
        od.close()


@pytest.fixture(scope="module")
def plain_features(frame):
    fg = front_params(n_scan=16, horizon_scan=1800)
    return features_of(lambda od: od.submit(fg, 100.0, *frame))


@pytest.mark.parametrize("kind,step", [("velodyne", 22), ("velodyne", 48), ("ouster", 22), ("ouster", 48)])
def test_message_times(frame, plain_features, kind, step):
    """fabsf of Velodyne float seconds (negative values, -0.0, a negative denormal) and uint32 nanoseconds * 1e-9f (0, 2^24 + 1, 99 999 999, 0xFFFFFFFF): the frame's
    feature clouds from the message's own times are, bit for bit, those from the times numpy computes"""
    xyz, ring = frame
    fg = front_params(n_scan=16, horizon_scan=1800)
    payload, L, rel = pack(xyz, ring, kind, step)
    assert not np.signbit(rel).any() and len(np.unique(rel)) >= 8                # (-0.0 and 0.0, 2^24 and 2^24 + 1 give one time each)
    d = dsk(ROT)

    def arrays(od):
        od.setDeskew(d, rel); od.submit(fg, 100.0, xyz, ring)

    def message(od):
        od.setDeskewFromMessage(d); od.submit_msg(fg, 100.0, payload, L)
    (ca, sa), na = features_of(arrays)
    (cm, sm), nm = features_of(message)
    assert na == nm and np.array_equal(bits(cm), bits(ca)) and np.array_equal(bits(sm), bits(sa))
    (cp, sp_), _ = plain_features
    assert ca.shape[0] > 0 and sa.shape[0] > 0 and not (np.array_equal(ca, cp) and np.array_equal(sa, sp_)), "the de-skew moved the features"


def test_message_without_a_time_field_takes_the_azimuth_route(frame, ctx):
    """time_kind 0 with a de-skew armed from the message: the times are interpolated from the azimuth — the same bits as setDeskewFromCloud on the same points"""
    xyz, ring = frame
    cfg = dict(n_scan=16, horizon_scan=1800)
    fg = front_params(**cfg)
    payload, L, _ = pack(xyz, ring, "velodyne", 22)
    L0 = CloudLayout(L.point_step, L.off_x, L.off_y, L.off_z, L.off_ring, L.ring_bytes, 0, 0)
    d = dsk(ROT)

    def message(od):
        od.setDeskewFromMessage(d); od.submit_msg(fg, 100.0, payload, L0)
    (cm, sm), nm = features_of(message)
    fe = FrontEnd(ctx, fg)
    fe.setDeskewFromCloud(d)
    pg = fe.project(xyz, ring); eg = fe.extract(pg["n"])
    t, flag = fe.deskewTimes(len(ring))
    assert 0 < flag < len(ring) and t[0] == 0 and abs(float(t[-1]) - 0.1) < 1e-4 and t.max() > 0.09
    assert nm == (pg["n"], eg["corner"].shape[0], eg["surface"].shape[0])
    assert np.array_equal(bits(cm), bits(eg["corner"])) and np.array_equal(bits(sm), bits(eg["surface"]))
    raw = FrontEnd(ctx, fg).project(xyz, ring)
    assert np.abs(pg["extracted"][:, :3] - raw["extracted"][:, :3]).max() > 1.0
