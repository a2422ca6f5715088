"""CPU: the numpy statement of the ground prior (tests/prior_twin.py) held to closed forms, to central differences, to its quirks and branches and to its own
second routes. The device tests (tests/test_gpu_groundprior.py) are judged by this statement.

Route spread recorded here (printed by test_route_spread_record, and in DESIGN.md 10): over the four kinds of ground plus the gentle slope, two vehicles, six poses
each, max |jacobi + LU route - eigh + numpy.linalg.solve route|. The device's bars are 10 x these."""
import math

import numpy as np
import pytest

import prior_cases as pc
import prior_twin as tw

f32 = np.float32


# ---- closed form ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("routes", [("jacobi", "lu"), ("eigh", "solve")])
def test_flat_ground_closed_form(routes):
    """a square vehicle on a flat ground at h rests at z = h + com_z - g / (4 k), roll = pitch = 0: all four contacts carry g / 4"""
    cloud = pc.terrain_cloud("flat")
    P = tw.Params.square(2.0)
    want = pc.FLAT_H + P.vehicle_com_z - P.g / (4.0 * P.k_spring)
    for x, y, yaw in pc.poses(3):
        r = tw.solve(cloud, P, x, y, yaw, eig=routes[0], lin=routes[1])
        assert r["end_reason"] == tw.END_CONVERGED and r["success"]
        assert abs(r["z"] - want) < 1e-8 and abs(r["roll"]) < 1e-8 and abs(r["pitch"]) < 1e-8
        assert np.all(np.abs(r["wheel_distance"] + P.g / (4.0 * P.k_spring)) < 1e-6)   # the nearest point is a float: its z is FLAT_H to 3e-8
        lp = r["lidar_pose"]
        assert abs(lp[2] - (r["z"] + 1.04)) < 1e-12 and abs(lp[0] - x) < 1e-9 and abs(math.remainder(lp[5] - yaw, 2 * math.pi)) < 1e-9


# ---- Jacobian --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle", list(pc.VEHICLES))
def test_jacobian_against_central_differences(vehicle):
    """ground points held fixed (the Jacobian's own premise): d residual / d (z, roll, pitch) with R' = RotX(dr) RotY(dp) R"""
    P = pc.VEHICLES[vehicle]()
    R = tw.mul33(tw.rotz(0.7), tw.mul33(tw.roty(0.05), tw.rotx(-0.08)))
    x, y, z = 0.3, -0.2, 0.9
    pw0 = tw.wheel_points(P, R, x, y, z)
    pn = [[p[0] + 0.01, p[1] - 0.02, p[2] + 0.05 + 0.01 * i] for i, p in enumerate(pw0)]   # above every wheel: all contacts active, none near its switch
    _, J = tw.residual_jacobian(P, R, pw0, pn)

    def res_at(dz, dr, dp):
        Rn = tw.mul33(tw.mul33(tw.rotx(dr), tw.roty(dp)), R)
        return np.array(tw.residual_jacobian(P, Rn, tw.wheel_points(P, Rn, x, y, z + dz), pn)[0])
    h = 1e-6
    for c, d in enumerate(((h, 0, 0), (0, h, 0), (0, 0, h))):
        num = (res_at(*d) - res_at(*(-v for v in d))) / (2 * h)
        assert np.allclose(num, [J[i][c] for i in range(3)], rtol=1e-6, atol=1e-6), (c, num, J)


# ---- quirks and branches -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("yaw", [math.pi - 1e-3, -math.pi + 1e-3, math.pi, -math.pi, 3.3, -3.3])
def test_yaw_is_held_fixed_across_pi(yaw):
    r = tw.solve(pc.terrain_cloud("tilt"), tw.Params(), 0.2, -0.4, yaw)
    assert r["end_reason"] == tw.END_CONVERGED
    assert abs(math.remainder(math.atan2(r["R"][1, 0], r["R"][0, 0]) - yaw, 2 * math.pi)) < 1e-12
    assert abs(r["roll"]) < 0.2 and abs(r["pitch"]) < 0.2   # the slope is 8 % and 5 %: a wrapped yaw would show up as a flipped tilt


def test_average_height_fallbacks():
    c = np.array([[0, 0, 1.0], [0.1, 0, 2.0], [0, 0.1, 3.0], [0.1, 0.1, 4.0], [5, 5, 9.0]], f32)
    q = (0.01, 0.01)   # nearest: point 0
    assert tw.average_height_at(c, tw.Params(ground_avg_radius=0.0), *q) == (1.0, 0)                       # radius <= 0
    assert tw.average_height_at(c, tw.Params(ground_avg_radius=-1.0), *q) == (1.0, 0)
    assert tw.average_height_at(c, tw.Params(ground_avg_radius=1e-30), *q) == (1.0, 0)                     # (float)(r r) = 0: the search finds nothing
    assert tw.average_height_at(c, tw.Params(ground_avg_radius=0.3, ground_min_neighbors=5), *q) == (1.0, 0)    # 4 hits < 5
    assert tw.average_height_at(c, tw.Params(ground_avg_radius=0.3, ground_min_neighbors=4), *q) == (2.5, 0)    # the mean, around the NEAREST point
    assert tw.average_height_at(c, tw.Params(ground_avg_radius=0.12, ground_min_neighbors=1), *q) == (2.0, 0)   # (1 + 2 + 3) / 3: the corner 0.141 away is out
    assert tw.average_height_at(c, tw.Params(ground_avg_radius=0.3, ground_min_neighbors=1), *q, cap=3) == (1.0, tw.STATUS_OVERFLOW)
    # the sum runs in the search's order, (d2, index): a float z whose serial sum depends on the order
    big = np.array([[0, 0, 1e8], [0.05, 0, 1.0], [0.1, 0, -1e8], [0.15, 0, 1.0]], f32)
    h, _ = tw.average_height_at(big, tw.Params(ground_avg_radius=1.0, ground_min_neighbors=1), 0.0, 0.0)
    assert h == ((1e8 + 1.0) + -1e8 + 1.0) / 4.0


@pytest.mark.parametrize("name", list(pc.fit_cases()))
def test_fit_fallbacks_on_constructed_neighbourhoods(name):
    cloud, q, kw, fallback, hits, inliers = pc.fit_cases()[name]
    for eig in ("jacobi", "eigh"):
        g = tw.ground_point(cloud, tw.Params(**kw), q[0], q[1], eig)
        assert (g["fallback"], g["hits"], g["inliers"]) == (fallback, hits, inliers), g
        if fallback == tw.FIT_OK:
            assert g["nearest"] == -1 and g["point"][:2] == [q[0], q[1]]
        else:
            i, _ = tw.nearest_xy(cloud, *q)
            assert g["nearest"] == i and g["point"] == [float(v) for v in cloud[i, :3]]
    if name in ("hits_15", "inliers_15"):   # the plane z = 0.1 x - 0.2 y + 1 through float points
        assert abs(g["point"][2] - (0.1 * q[0] - 0.2 * q[1] + 1.0)) < 1e-6


def test_outlier_bounds_are_inclusive():
    cloud, q, _, _, _, _ = pc.fit_cases()["on_the_bound"]
    pts = cloud[tw.radius_xy(cloud, q[0], q[1], 0.6)[0], :3]
    z = pts[:, 2].astype(np.float64)
    mean = tw.serial_sum(z) / 18.0
    sd = math.sqrt(tw.serial_sum((z - mean) ** 2) / 18.0)
    assert mean == 0.0 and sd == 1.0 and sorted(z)[0] == mean - 3.0 * sd and sorted(z)[-1] == mean + 3.0 * sd   # the two points sit ON the bounds
    assert tw.fit_points(pts, 0.0, 0.0, 3.0, 15)[1] == 18
    assert tw.fit_points(pts, 0.0, 0.0, math.nextafter(3.0, 0.0), 15)[1] == 16   # a hair inside and they go


def test_fit_overflow_takes_the_nearest_point():
    cloud = pc.terrain_cloud("flat")
    g = tw.ground_point(cloud, tw.Params(), 0.0, 0.0, cap=10)
    assert g["fallback"] == tw.FIT_OVERFLOW and g["hits"] > 10 and g["nearest"] == tw.nearest_xy(cloud, 0.0, 0.0)[0]
    r = tw.solve(cloud, tw.Params.square(2.0), 0.0, 0.0, 0.3, cap=10)
    assert r["status"] & tw.STATUS_OVERFLOW and not r["success"]


def test_queries_order_and_strictness():
    c = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [0.6, 0, 0], [0.6, 0, 0]], f32)
    assert tw.nearest_xy(c, 0.0, 0.0)[0] == 4                           # of the two equal points the lower index
    idx, d2 = tw.radius_xy(c, 0.0, 0.0, 1.0)
    assert list(idx) == [4, 5] and np.all(d2 == f32(0.6) * f32(0.6))    # d2 = 1 is not < 1: strict
    idx, _ = tw.radius_xy(c, 0.0, 0.0, 1.0000001)
    assert list(idx) == [4, 5, 0, 1, 2, 3]                              # equal distances in index order
    assert tw.radius_xy(c, 0.0, 0.0, 0.6)[0].size == 0                  # (float)(0.36) is below 0.6f 0.6f = 0.36000004


def test_patch_limits_and_order():
    lo, hi = f32(0.1 - 0.15), f32(0.1 + 0.15)   # a limit whose double value is no float
    xs = [np.nextafter(lo, f32(-1)), lo, np.nextafter(lo, f32(1)), np.nextafter(hi, f32(-1)), hi, np.nextafter(hi, f32(1))]
    c = np.zeros((len(xs) + 3, 5), f32)
    c[:len(xs), 0] = xs
    c[len(xs):, 0] = 0.1
    c[len(xs), 2], c[len(xs) + 1, 2], c[len(xs) + 2, 3] = np.nan, np.inf, np.nan   # non-finite z is dropped, a NaN elsewhere is kept
    c[:, 4] = np.arange(c.shape[0])
    out = tw.extract_patch(c, 0.1, 0.0, 0.3)
    assert list(out[:, 4]) == [1, 2, 3, 4, 8]
    assert tw.extract_patch(c, 50.0, 0.0, 0.3).shape == (0, 5)


# ---- FailureDetection ------------------------------------------------------------------------------------------------------------------------------------------
def test_failure_detection_refusals():
    P = tw.Params.square(2.0)
    pit = pc.ground("flat")
    pit[:, 2] = -10.0
    r = tw.solve(pit, P, 0.1, 0.2, 0.3)
    assert r["end_reason"] == tw.END_CONVERGED and r["z"] < P.z_min and not r["success"]
    tilt = pc.terrain_cloud("tilt")
    r = tw.solve(tilt, tw.Params.square(2.0, pitch_max=0.05), 0.1, 0.2, 0.0)
    assert r["end_reason"] == tw.END_CONVERGED and abs(r["pitch"]) > 0.05 and abs(r["roll"]) <= 0.5 and not r["success"]
    assert tw.solve(tilt, tw.Params.square(2.0, roll_max=0.03), 0.1, 0.2, 0.0)["success"] is False
    assert tw.solve(tilt, P, 0.1, 0.2, 0.0)["success"] is True
    r = tw.solve(tilt, tw.Params.square(2.0, max_iters=1), 0.1, 0.2, 0.0)
    assert r["end_reason"] == tw.END_MAX_ITERS and r["iterations"] == 1 and not r["success"]


# ---- the routes' spread: the record the device's bars derive from ----------------------------------------------------------------------------------------------
def test_route_spread_record(capsys):
    ref, spread = pc.solve_reference()
    with capsys.disabled():
        print("\nroute spread over", len(ref), "terrain x vehicle sets:", {k: "%.3g" % v for k, v in spread.items()})
    # both routes end every pose the same way and agree far below anything a user would see
    for (name, vehicle), (ps, a, b) in ref.items():
        for ra, rb in zip(a, b):
            assert ra["end_reason"] == rb["end_reason"] == tw.END_CONVERGED, (name, vehicle)
    # both routes stop within tol_step = 1e-10 of the same root, whichever iteration each stops at: ten steps is the most they can be apart
    assert all(v < 1e-9 for v in spread.values())
    assert all(v > 0.0 for v in spread.values())   # a zero spread would turn a derived bar into a demand for equal bits


def test_discrete_outcomes_are_decisive_on_the_discrete_terrains(capsys):
    """the cap the device test lives under: at most 10 % of a terrain's poses may have an end reason or iteration count that sits within a factor 10 of a threshold"""
    ref, _ = pc.solve_reference()
    for name in pc.DISCRETE_TERRAINS:
        for vehicle, make in pc.VEHICLES.items():
            ps, a, _ = ref[(name, vehicle)]
            out = [k for k, r in enumerate(a) if not tw.decisive(r, make())]
            with capsys.disabled():
                print(name, vehicle, "iterations", [r["iterations"] for r in a], "left out", out)
            assert len(out) <= 0.1 * len(a)
