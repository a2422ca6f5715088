"""GPU: K1 (project_kernel, rolo_amd/csrc/front.hip) on the constructed clouds of tests/projection_cases.py against the C++ oracle — planted pairs of adjacent floats
on either side of every column edge (where one ulp of the device's atan2f is a column), the axes with signed zeros and denormals, ranges at and one float beside
the gates, ring values at and past n_scan. The expectation itself is pinned on the CPU in test_projection_cases.py. Everything is np.array_equal.

What the planted edges found: with the device's atan2f alone 45 % of the kept points (701 of 1538 at H = 1024 ... 2734 of 6086 at H = 4096) came out in the neighbouring
column or lost their pixel to such a neighbour; with the guarded fp64 angle of project_kernel all of them are in the oracle's column, and the dropped points (host
libm not correctly rounded) all in the correctly rounded one."""
import numpy as np
import pytest

import projection_cases as pc
from oracle import pyorc
from rolo_amd.frontend import FrontEnd, front_params
from rolo_amd.rotvgicp import RotVGICP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def built():
    return pc.build()


@pytest.fixture(scope="module")
def ctx():
    g = RotVGICP()
    yield g
    g.close()


def both(ctx, case):
    fo = pyorc.front_params(**case.cfg)
    fe = FrontEnd(ctx, front_params(**case.cfg))
    return fo, pyorc.project(fo, case.xyz, case.ring), fe, fe.project(case.xyz, case.ring, want_range_mat=True)


def check_projection(case, po, pg):
    """the six comparisons of test_gpu_frontend.check_projection, the columns first and point by point: the number alone is useless here"""
    dev, _ = pc.read_back(case, pg)
    ref, _ = pc.read_back(case, po)
    assert np.array_equal(dev, ref), pc.describe(case, dev, ref)
    assert pg["n"] == po["n"], (case.name, pg["n"], po["n"])
    assert np.array_equal(pg["start_ring"], po["start_ring"]) and np.array_equal(pg["end_ring"], po["end_ring"]), case.name
    assert np.array_equal(pg["point_col_ind"], po["point_col_ind"]), case.name
    assert np.array_equal(pg["point_range"], po["point_range"]), case.name
    assert np.array_equal(pg["extracted"], po["extracted"]), case.name
    assert np.array_equal(pg["range_mat"], po["range_mat"]), case.name


@pytest.mark.parametrize("H", pc.EDGE_H)
def test_planted_column_edges(built, ctx, H):
    """every kept point — the host libm's atan2f is the correctly rounded value there — lands in the oracle's column, the third points lose their pixels to the
    earlier ones; then the features of the cloud, so that a pixel off cannot cancel downstream"""
    case = built["edges"][H]["kept"]
    fo, po, fe, pg = both(ctx, case)
    check_projection(case, po, pg)
    assert pg["n"] == case.n
    eo = pyorc.extract_features(fo, po)
    eg = fe.extract(pg["n"], debug=True)
    for k in ("curvature", "picked", "label"):
        assert np.array_equal(eg[k], eo[k]), k
    for k in ("corner", "surface"):
        assert eg[k].shape == eo[k].shape and np.array_equal(eg[k], eo[k]), k
    assert eo["corner"].shape[0] > 0
    print("EDGES H=%d: the device's column is the correctly rounded one on all %d kept points" % (H, len(case.ring)))


@pytest.mark.parametrize("H", pc.EDGE_H)
def test_axes_signed_zeros_and_denormals(built, ctx, H):
    case = built["axes"][H]
    _, po, _, pg = both(ctx, case)
    check_projection(case, po, pg)
    assert pg["n"] == case.n


def test_range_gates(built, ctx):
    """ranges exactly at the gates, one float beside them, and the points that change sides when x*x + y*y + z*z is contracted"""
    for case in built["gates"]:
        _, po, _, pg = both(ctx, case)
        check_projection(case, po, pg)
        assert pg["n"] == case.n


def test_ring_values_and_downsample_rate(built, ctx):
    for case in built["rings"]:
        _, po, _, pg = both(ctx, case)
        check_projection(case, po, pg)
        assert pg["n"] == case.n


def test_dropped_points_are_counted_not_asserted(built, ctx):
    """the planted points where the host libm's atan2f is NOT the correctly rounded value: no device answer can match both statements, so the disagreements with the
    oracle and with the correctly rounded statement are printed (EDGEDIFF, as the POLAR key's are) and nothing about the columns is asserted"""
    for H in pc.EDGE_H:
        case = built["edges"][H]["dropped"]
        _, po, _, pg = both(ctx, case)
        dev, _ = pc.read_back(case, pg)
        ref, _ = pc.read_back(case, po)
        print("EDGEDIFF projection H=%d: %d dropped points, device column != oracle (host libm) column on %d, != the correctly rounded column on %d"
              % (H, len(case.ring), int((dev != ref).sum()), int((dev != case.col_cr).sum())))


def test_edges_through_the_pointcloud2_payload(built):
    """the H = 1800 edge cloud as the bytes of a sensor_msgs/PointCloud2 in the velodyne driver's packed layout (point_step 22: no alignment) through
    rolo_odom_submit_msg. The driver's first frame only stores its features: N and the corner / surface clouds come back through the ABI as it is and are the
    oracle's, bit for bit."""
    from rolo_amd._lib import CloudLayout
    from rolo_amd.odometry import LidarOdometry
    case = built["edges"][1800]["kept"]
    n = len(case.ring)
    dt = np.dtype({"names": ["x", "y", "z", "intensity", "ring", "time"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u2", "<f4"], "offsets": [0, 4, 8, 12, 16, 18],
                   "itemsize": 22})
    a = np.zeros(n, dt)
    a["x"], a["y"], a["z"] = case.xyz[:, 0], case.xyz[:, 1], case.xyz[:, 2]
    a["intensity"] = 7.0; a["ring"] = case.ring; a["time"] = (np.arange(n) / n * 0.1).astype(np.float32)
    fo = pyorc.front_params(**case.cfg)
    po = pyorc.project(fo, case.xyz, case.ring); eo = pyorc.extract_features(fo, po)
    od = LidarOdometry(0, 0.3)
    od.submit_msg(front_params(**case.cfg), 100.0, a.view(np.uint8).reshape(-1), CloudLayout(22, 0, 4, 8, 16, 2, 18, 1))
    rc, _, _, _, counts = od.collect()
    corner, surface = od.features()
    od.close()
    assert rc == 0 and counts == (po["n"], eo["corner"].shape[0], eo["surface"].shape[0])
    assert np.array_equal(corner, eo["corner"]) and np.array_equal(surface, eo["surface"])
