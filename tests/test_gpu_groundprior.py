"""GPU: the ground prior (rolo_ground_* / rolo_priorpose_*, rolo_amd/csrc/groundprior.hip) against its numpy statement (tests/prior_twin.py).

Queries and the patch are compared bit for bit (indices, and floats as uint32). The fit's counts and fall-back are exact; its height, and the solver's z, roll,
pitch, cost and wheel distances, are held within 10 x the spread between the statement's own two routes (prior_cases.solve_reference; the record is in
tests/test_prior_twin.py and DESIGN.md 10), the flat ground also to its closed form within 1e-8. End reason and iteration count are asserted on the grounds where
the statement's deciding quantities stay a factor 10 from their thresholds for at least 90 % of the poses (prior_cases.DISCRETE_TERRAINS says why a slope is not
among them); the poses left out are printed."""
import functools

import numpy as np
import pytest

import prior_cases as pc
import prior_twin as tw
from oracle import pyorc
from rolo_amd._lib import RoloError
from rolo_amd.backend import GroundModel, PriorPoseSolver, prior_pose_params

pytestmark = pytest.mark.gpu

f32 = np.float32
EINVAL, ESTATE, ENONFINITE = -1, -5, -11
CAP = 4096


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture
def gm():
    g = GroundModel()
    yield g
    g.close()


def device_params(P):
    """prior_twin.Params -> rolo_priorpose_params"""
    return prior_pose_params(wheel_xy=P.wheel_xy, **{k: getattr(P, k) for k in (
        "vehicle_com_z", "body_to_lidar_t", "body_to_lidar_R", "k_spring", "g", "max_iters", "lm_lambda", "tol_cost", "tol_step", "ground_avg_radius",
        "ground_min_neighbors", "fit_radius", "fit_outlier_factor", "fit_min_points", "z_min", "z_max", "roll_max", "pitch_max", "wheel_distance_max")})


def check_queries(gm, cloud, queries, radii):
    """nearest and every radius at every query, device against statement, bit for bit"""
    q = np.asarray(queries, f32).reshape(-1, 2)
    idx, d2 = gm.nearestXY(q)
    for k, (qx, qy) in enumerate(q):
        wi, wd = tw.nearest_xy(cloud, qx, qy)
        assert (idx[k], bits(d2[k])) == (wi, bits(wd)), ("nearest", k, qx, qy)
    for r in radii:
        got = gm.radiusXY(q, r)
        for k, (qx, qy) in enumerate(q):
            wi, wd = tw.radius_xy(cloud, qx, qy, r)
            cnt, gi, gd = got[k]
            assert cnt == wi.shape[0], ("count", r, k)
            if cnt <= CAP:
                assert np.array_equal(gi, wi) and same(gd, wd), ("radius", r, k)
            else:
                assert gi.size == 0


# ---- queries -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4096, 4097])
def test_queries_n_points_in_one_cell(gm, n):
    """the sort's two forms (by rank up to 256 keys, the network above) and the list's edges: 4096 fills it, 4097 overflows (count only)"""
    rng = np.random.default_rng(n)
    cloud = np.zeros((n, 4), f32)
    cloud[:, :2] = rng.uniform(0.0, 0.5, (n, 2))
    cloud[:, 2] = rng.uniform(-1, 1, n)
    gm.setCloud(cloud)
    info = gm.info()
    assert (info["points"], info["nx"], info["ny"]) == (n, 1, 1)
    check_queries(gm, cloud, [[0.25, 0.25], [0.0, 0.0], [0.6, 0.6], [-3.0, 0.2], cloud[0, :2]], [1.0, 0.2, 0.05])


def test_queries_ties_duplicates_and_the_strict_edge(gm):
    q0 = f32(0.6)
    edge = [q0]
    for _ in range(4):
        edge = [np.nextafter(edge[0], f32(0))] + edge + [np.nextafter(edge[-1], f32(1))]
    pts = [[x, 0.0] for x in edge] + [[0.0, x] for x in edge] + [[-x, 0.0] for x in edge]          # d2 one float apart on either side of (float)(0.36)
    pts += [[0.25, 0.0], [0.0, 0.25], [-0.25, 0.0], [0.0, -0.25], [0.25, 0.0], [0.25, 0.0]]           # planted equal distances, duplicated points
    pts += [[3.0, 3.0], [3.0, 3.0], [-2.0, 5.0]]
    cloud = np.zeros((len(pts), 3), f32)
    cloud[:, :2] = pts
    gm.setCloud(cloud)
    d2 = tw.d2_xy(cloud, 0.0, 0.0)[:len(edge)]
    r2 = f32(0.6 * 0.6)
    assert (d2 < r2).any() and (d2 >= r2).any()   # the planted points straddle the strict test
    check_queries(gm, cloud, [[0.0, 0.0], [3.0, 3.0], [1.5, 1.5]], [0.6, 0.25, 0.2500001, 5.0])
    idx, _ = gm.nearestXY([[0.0, 0.0], [3.0, 3.0]])
    assert list(idx) == [len(edge) * 3, len(pts) - 3]   # the lowest index among equals


def test_queries_line_cloud_corners_outside_and_far(gm):
    t = np.linspace(-40.0, 40.0, 3001)
    cloud = np.zeros((t.size, 3), f32)
    cloud[:, 0], cloud[:, 1], cloud[:, 2] = t, 0.5 * t, 0.01 * t
    gm.setCloud(cloud)
    info = gm.info()
    assert info["nx"] > 1 and info["ny"] > 1
    mn = cloud[:, :2].min(axis=0)
    cell = 0.6 * 2 ** info["doubled"]
    corners = [[mn[0] + cell * i, mn[1] + cell * j] for i, j in ((0, 0), (1, 1), (3, 2), (info["nx"], info["ny"]))]
    off = [[-40.0, 20.0], [40.0, -20.0], [0.0, 19.0], [-45.0, -25.0], [1e4, -1e4], [-1e6, 3.0], [0.3, 0.15]]
    check_queries(gm, cloud, corners + off, [0.6, 0.1, 2.0, 30.0])


@pytest.mark.parametrize("cell,max_cells", [(0.6, 1 << 22), (0.6, 16), (0.05, 1 << 22), (7.0, 1 << 22)])
def test_queries_any_grid_same_answers(gm, cell, max_cells):
    """a radius smaller and larger than a cell, the doubling of the cell size: the grid never shows in an answer"""
    cloud = pc.terrain_cloud("tilt_noise")
    gm.setGrid(cell, max_cells)
    gm.setCloud(cloud)
    info = gm.info()
    assert info["nx"] * info["ny"] <= min(max_cells, 4 * cloud.shape[0] + 1024)
    assert (info["doubled"] > 0) == (max_cells == 16 or cell == 0.05)
    rng = np.random.default_rng(2)
    q = np.vstack([rng.uniform(-7, 7, (12, 2)), cloud[:3, :2], [[-6.0, -6.0], [6.0, 6.0], [9.0, 0.0]]])
    check_queries(gm, cloud, q, [0.6, 0.1, 2.0])


def test_neighbourhood_of_exactly_the_cap_and_one_more(gm):
    rng = np.random.default_rng(9)
    a = rng.uniform(0, 2 * np.pi, CAP + 1)
    rad = np.concatenate([rng.uniform(0.0, 0.5, CAP), [0.55]])   # 4096 points within 0.5 of the origin, one at 0.55
    cloud = np.zeros((CAP + 1, 4), f32)
    cloud[:, 0], cloud[:, 1], cloud[:, 2] = rad * np.cos(a), rad * np.sin(a), 0.1 * rad
    cloud = np.vstack([cloud, np.array([[9.0, 9.0, 0.0, 0.0]], f32)])
    gm.setCloud(cloud)
    check_queries(gm, cloud, [[0.0, 0.0]], [0.52, 0.6])
    got = gm.radiusXY([[0.0, 0.0]], 0.52)[0], gm.radiusXY([[0.0, 0.0]], 0.6)[0]
    assert got[0][0] == CAP and got[0][1].size == CAP and got[1][0] == CAP + 1 and got[1][1].size == 0
    for fit_radius, want in ((0.52, tw.FIT_OK), (0.6, tw.FIT_OVERFLOW)):
        P = tw.Params(fit_radius=fit_radius)
        f = PriorPoseSolver(gm, device_params(P)).fitSurface([[0.0, 0.0]])
        w = tw.ground_point(cloud, P, 0.0, 0.0)
        assert (f["fallback"][0], f["hits"][0], f["inliers"][0], f["nearest"][0]) == (want, w["hits"], w["inliers"], w["nearest"])


# ---- patch ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_patch_limits_nonfinite_and_empty(gm):
    cx, cy, size = 0.1, -0.3, 0.3   # limits whose double values are no floats
    lim = [f32(cx - 0.15), f32(cx + 0.15), f32(cy - 0.15), f32(cy + 0.15)]
    rows = []
    for axis, v in ((0, lim[0]), (0, lim[1]), (1, lim[2]), (1, lim[3])):
        for x in (np.nextafter(v, f32(-9)), v, np.nextafter(v, f32(9))):   # one float outside / on / one float inside each limit
            p = [cx, cy, 1.0, 7.0, 8.0]
            p[axis] = x
            rows.append(p)
    rows += [[cx, cy, np.nan, 1, 2], [cx, cy, np.inf, 1, 2], [cx, cy, -np.inf, 1, 2], [cx, cy, 0.5, np.nan, np.inf]]
    cloud = np.array(rows, f32)
    cloud[:, 4] = np.arange(cloud.shape[0])
    gm.setCloud(cloud)
    want = tw.extract_patch(cloud, cx, cy, size)
    assert want.shape[0] == 9   # 2 of 3 at each limit, and the record whose NaN is not a coordinate
    assert same(gm.extractPatch(cx, cy, size), want)
    assert gm.extractPatch(50.0, 50.0, size).shape == (0, 5)
    assert gm.extractPatch(cx, cy, -1.0).shape == (0, 5)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_patch_order_across_workgroup_edges(gm, n):
    """kept: the first and last point of every 256-point block and of the cloud, plus a seeded few; order must be the caller's. Transformed form against the
    oracle's orc_transform_cloud_f of the untransformed patch"""
    rng = np.random.default_rng(n)
    cloud = np.zeros((n, 4), f32)
    cloud[:, :3] = rng.uniform(50.0, 60.0, (n, 3))       # outside the square
    i = np.arange(n)
    keep = (i % 256 == 0) | (i % 256 == 255) | (i == n - 1) | (rng.uniform(size=n) < 0.01)
    cloud[keep, :2] = rng.uniform(-1.0, 1.0, (int(keep.sum()), 2))
    cloud[:, 3] = i % 1000
    gm.setCloud(cloud)
    want = tw.extract_patch(cloud, 0.0, 0.0, 2.0)
    assert want.shape[0] == int(keep.sum())
    got = gm.extractPatch(0.0, 0.0, 2.0)
    assert same(got, want)
    T = pyorc.get_transformation(0.3, -0.2, 1.5, 0.02, -0.03, 0.7).reshape(4, 4)
    moved = want.copy()
    moved[:, :3] = pyorc.transform_cloud_f(np.ascontiguousarray(want[:, :3]), T)
    assert same(gm.extractPatch(0.0, 0.0, 2.0, T), moved)
    assert same(tw.extract_patch(cloud, 0.0, 0.0, 2.0, T), moved)   # the statement says the same


# ---- fit -----------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fit_height_bar():
    """10 x the spread of the fitted height between the statement's eigen routes, over the constructed neighbourhoods and a seeded set on every terrain"""
    spread = 0.0
    for cloud, q, kw, *_ in pc.fit_cases().values():
        a, b = (tw.ground_point(cloud, tw.Params(**kw), q[0], q[1], e) for e in ("jacobi", "eigh"))
        spread = max(spread, abs(a["point"][2] - b["point"][2]))
    for name in pc.TERRAINS:
        for q in pc.poses(55)[:, :2] * 3.0:
            a, b = (tw.ground_point(pc.terrain_cloud(name), tw.Params(), q[0], q[1], e) for e in ("jacobi", "eigh"))
            spread = max(spread, abs(a["point"][2] - b["point"][2]))
    assert spread > 0.0
    return 10.0 * spread


@pytest.mark.parametrize("name", list(pc.fit_cases()))
def test_fit_constructed_neighbourhoods(gm, name):
    cloud, q, kw, fallback, hits, inliers = pc.fit_cases()[name]
    P = tw.Params(**kw)
    gm.setCloud(cloud)
    f = PriorPoseSolver(gm, device_params(P)).fitSurface([q])
    w = tw.ground_point(cloud, P, q[0], q[1])
    assert (w["fallback"], w["hits"], w["inliers"]) == (fallback, hits, inliers)
    assert (f["fallback"][0], f["hits"][0], f["inliers"][0], f["nearest"][0]) == (fallback, hits, inliers, w["nearest"])
    bar = fit_height_bar()
    print(name, "height", f["point"][0, 2], "statement", w["point"][2], "bar", bar)
    assert np.all(np.abs(f["point"][0] - w["point"]) <= [0.0, 0.0, bar if fallback == tw.FIT_OK else 0.0])


@pytest.mark.parametrize("name", list(pc.TERRAINS))
def test_fit_on_terrains(gm, name):
    cloud = pc.terrain_cloud(name)
    gm.setCloud(cloud)
    q = np.vstack([pc.poses(55, 16)[:, :2] * 3.0, [[6.5, 0.0], [-5.9, 5.9], [20.0, 20.0]]])   # inside, at the rim (few hits), outside
    f = PriorPoseSolver(gm).fitSurface(q)
    bar = fit_height_bar()
    worst = 0.0
    for k, (qx, qy) in enumerate(q):
        w = tw.ground_point(cloud, tw.Params(), qx, qy)
        assert (f["fallback"][k], f["hits"][k], f["inliers"][k], f["nearest"][k]) == (w["fallback"], w["hits"], w["inliers"], w["nearest"]), k
        worst = max(worst, abs(f["point"][k, 2] - w["point"][2]))
        assert f["point"][k, 0] == w["point"][0] and f["point"][k, 1] == w["point"][1]
    print(name, "worst height difference", worst, "bar", bar)
    assert worst <= bar


# ---- solve ---------------------------------------------------------------------------------------------------------------------------------------------------
def bars():
    _, spread = pc.solve_reference()
    return {k: 10.0 * v for k, v in spread.items()}


@pytest.mark.parametrize("vehicle", list(pc.VEHICLES))
@pytest.mark.parametrize("name", list(pc.TERRAINS) + ["gentle"])
def test_solve_against_statement(gm, name, vehicle):
    ref, _ = pc.solve_reference()
    ps, a, _ = ref[(name, vehicle)]
    P = pc.VEHICLES[vehicle]()
    gm.setCloud(pc.terrain_cloud(name))
    r = PriorPoseSolver(gm, device_params(P)).solve(ps)
    bar = bars()
    for k, w in enumerate(a):
        for q in pc.QUANTITIES:
            diff = float(np.max(np.abs(np.asarray(r[q][k]) - np.asarray(w[q]))))
            print(name, vehicle, k, q, "device - statement", diff, "bar", bar[q])
            assert diff <= bar[q], (q, k)
        assert r["status"][k] == w["status"] == 0 and r["success"][k] == w["success"]
        # the lidar pose is (x, y, z, the angles) moved by body_to_lidar, whose lever is 1.04 m: what z, roll and pitch differ by, through that lever
        assert np.max(np.abs(r["lidar_pose"][k] - w["lidar_pose"])) <= bar["z"] + 3.0 * (bar["roll"] + bar["pitch"])
        if name == "flat" and vehicle == "square":   # the closed form again
            assert abs(r["z"][k] - (pc.FLAT_H + P.vehicle_com_z - P.g / (4.0 * P.k_spring))) < 1e-8 and abs(r["roll"][k]) < 1e-8 and abs(r["pitch"][k]) < 1e-8


@pytest.mark.parametrize("vehicle", list(pc.VEHICLES))
@pytest.mark.parametrize("name", list(pc.DISCRETE_TERRAINS))
def test_solve_end_reason_and_iterations(gm, name, vehicle):
    ref, _ = pc.solve_reference()
    ps, a, _ = ref[(name, vehicle)]
    P = pc.VEHICLES[vehicle]()
    gm.setCloud(pc.terrain_cloud(name))
    r = PriorPoseSolver(gm, device_params(P)).solve(ps)
    left_out = [k for k, w in enumerate(a) if not tw.decisive(w, P)]
    print(name, vehicle, "left out", left_out, "device iterations", list(r["iterations"]), "statement", [w["iterations"] for w in a])
    assert len(left_out) <= 0.1 * len(a)
    for k, w in enumerate(a):
        if k not in left_out:
            assert (r["end_reason"][k], r["iterations"][k]) == (w["end_reason"], w["iterations"]), k


def result_bytes(r, k):
    return b"".join(np.ascontiguousarray(r[q][k]).tobytes() for q in ("z", "roll", "pitch", "R", "cost", "wheel_distance", "lidar_pose", "iterations", "end_reason", "success", "status"))


def test_batching_same_bits_alone_and_in_any_batch(gm):
    """one pose alone, and at positions 0, 1 and B - 1 of batches of 2, 64, 65 and 1000; the same batch twice; a neighbour that overflows or ends at max_iters"""
    cloud = pc.terrain_cloud("tilt_noise")
    rng = np.random.default_rng(8)
    blob = np.zeros((CAP + 200, 4), f32)   # a crowded spot at (4, 4): more than 4096 points inside one fit's disc
    blob[:, :2] = 4.0 + rng.uniform(-0.2, 0.2, (blob.shape[0], 2))
    blob[:, 2] = 0.2
    cloud = np.vstack([cloud, blob])
    gm.setCloud(cloud)
    P = tw.Params.square(2.0)
    s = PriorPoseSolver(gm, device_params(P))
    pose = np.array([0.4, -0.7, 1.1])
    alone = s.solve([pose])
    want = result_bytes(alone, 0)
    assert alone["status"][0] == 0 and alone["end_reason"][0] == tw.END_CONVERGED
    crowd = np.array([3.0, 3.0, 0.0])    # its wheel at (+1, +1) stands on the blob
    for B in (2, 64, 65, 1000):
        for pos in (0, 1, B - 1):
            batch = np.column_stack([rng.uniform(-1.5, 1.5, B), rng.uniform(-1.5, 1.5, B), rng.uniform(-3.3, 3.3, B)])
            batch[pos] = pose
            batch[(pos + 1) % B] = crowd
            r = s.solve(batch)
            assert result_bytes(r, pos) == want, (B, pos)
            assert r["status"][(pos + 1) % B] & tw.STATUS_OVERFLOW and not r["success"][(pos + 1) % B]
            if B == 65 and pos == 1:
                again = s.solve(batch)
                assert all(result_bytes(r, k) == result_bytes(again, k) for k in range(B))   # run to run
    # every pose of a batch under a cap of 3 iterations ends at max_iters next to none that would not: the same bits as each alone
    s3 = PriorPoseSolver(gm, device_params(tw.Params.square(2.0, max_iters=3)))
    batch = np.column_stack([rng.uniform(-1.5, 1.5, 5), rng.uniform(-1.5, 1.5, 5), rng.uniform(-3.3, 3.3, 5)])
    r = s3.solve(batch)
    assert np.all(r["end_reason"] == tw.END_MAX_ITERS) and not r["success"].any()
    for k in range(5):
        assert result_bytes(s3.solve([batch[k]]), 0) == result_bytes(r, k)


def test_failure_detection_each_refusal(gm):
    P = tw.Params.square(2.0)
    tilt = pc.terrain_cloud("tilt")
    pit = pc.ground("flat")
    pit[:, 2] = -10.0
    # no support under one wheel of a pose at the origin: where that wheel comes to rest the ground's returns are gone within 0.25 m but for one, half a metre
    # down. The fit's outlier cut drops it and the solve rests on the plane; the end's distance is to the NEAREST point, which is that return
    w0 = tw.solve(tilt, P, 0.0, 0.0, 0.0)
    pw = tw.wheel_points(P, w0["R"].tolist(), 0.0, 0.0, w0["z"])[1]
    hole = np.vstack([tilt[np.hypot(tilt[:, 0] - pw[0], tilt[:, 1] - pw[1]) > 0.25], np.array([[pw[0], pw[1], pw[2] - 0.5, 0.0]], f32)])
    cases = [("pit past z_min", pit, P, (0.1, 0.2, 0.3)), ("slope past the pitch bound", tilt, tw.Params.square(2.0, pitch_max=0.05), (0.1, 0.2, 0.0)),
             ("slope past the roll bound", tilt, tw.Params.square(2.0, roll_max=0.03), (0.1, 0.2, 0.0)),
             ("missing wheel support", hole, P, (0.0, 0.0, 0.0)), ("max_iters = 1", tilt, tw.Params.square(2.0, max_iters=1), (0.1, 0.2, 0.0)),
             ("none", tilt, P, (0.1, 0.2, 0.0))]
    for what, cloud, Pc, pose in cases:
        w = tw.solve(cloud, Pc, *pose)
        gm.setCloud(cloud)
        r = PriorPoseSolver(gm, device_params(Pc)).solve([pose])
        print(what, "statement: z", w["z"], "roll", w["roll"], "pitch", w["pitch"], "distances", w["wheel_distance"], "end", w["end_reason"], "success", w["success"])
        assert w["success"] == (what == "none") and r["success"][0] == w["success"], what
        assert r["end_reason"][0] == w["end_reason"], what
        if what == "missing wheel support":   # the one refusal is the distance: everything else holds
            assert w["end_reason"] == tw.END_CONVERGED and Pc.z_min <= w["z"] <= Pc.z_max and abs(w["roll"]) <= Pc.roll_max and abs(w["pitch"]) <= Pc.pitch_max
            assert np.max(np.abs(w["wheel_distance"])) > Pc.wheel_distance_max and np.max(np.abs(r["wheel_distance"][0])) > Pc.wheel_distance_max


def test_handle_pose(gm):
    cloud = pc.ground("tilt", stride=5)
    gm.setCloud(cloud)
    s = PriorPoseSolver(gm, groundPatchSize=4.0)
    got = s.handlePose(0.3, -0.2, 0.5)
    assert got is not None
    guess, patch = got
    w = tw.solve(cloud, tw.Params(), 0.3, -0.2, 0.5)
    assert guess.dtype == f32 and np.allclose(guess, w["lidar_pose"], atol=1e-6)
    raw = tw.extract_patch(cloud, w["lidar_pose"][0], w["lidar_pose"][1], 4.0)
    assert patch.shape == raw.shape and same(patch[:, 3:], raw[:, 3:])
    assert np.max(np.abs(patch[:, 2] + (1.0 + 1.04 - 0.0125))) < 0.05   # the ground seen from the lidar: a plane com_z + 1.04 - g / (4 k) below it
    pit = cloud.copy()
    pit[:, 2] = -10.0
    gm.setCloud(pit)
    assert s.handlePose(0.3, -0.2, 0.5) is None


# ---- errors --------------------------------------------------------------------------------------------------------------------------------------------------
def code_of(fn, *a, **kw):
    with pytest.raises(RoloError) as e:
        fn(*a, **kw)
    return e.value.code


def test_errors(gm):
    s = PriorPoseSolver(gm)
    for fn, args in ((gm.nearestXY, ([[0, 0]],)), (gm.radiusXY, ([[0, 0]], 1.0)), (gm.extractPatch, (0, 0, 1)), (s.solve, ([[0, 0, 0]],)), (s.fitSurface, ([[0, 0]],))):
        assert code_of(fn, *args) == ESTATE   # a model without a cloud
    cloud = pc.terrain_cloud("flat")
    gm.setCloud(cloud)
    bad = cloud.copy()
    bad[17, 1] = np.nan
    assert code_of(gm.setCloud, bad) == ENONFINITE
    bad[17, 1] = np.inf
    assert code_of(gm.setCloud, bad) == ENONFINITE
    assert gm.info()["points"] == cloud.shape[0] and s.solve([[0, 0, 0]])["success"][0]   # nothing was stored: the model holds what it held
    assert code_of(s.solve, np.zeros((0, 3))) == EINVAL
    assert code_of(s.solve, np.zeros((65537, 3))) == EINVAL
    assert code_of(s.solve, [[0, np.nan, 0]]) == ENONFINITE
    assert code_of(s.solve, [[np.inf, 0, 0]]) == ENONFINITE
    nine = PriorPoseSolver(gm, prior_pose_params(wheel_xy=[(np.cos(a), np.sin(a)) for a in np.arange(9)]))
    assert code_of(nine.solve, [[0, 0, 0]]) == EINVAL
    assert code_of(PriorPoseSolver(gm, prior_pose_params(k_spring=np.nan)).solve, [[0, 0, 0]]) == ENONFINITE
    assert code_of(gm.nearestXY, [[np.nan, 0]]) == ENONFINITE
    # a cap that is too small: EINVAL, and the size still comes back
    import ctypes as C
    from rolo_amd._lib import lib
    out = np.zeros((4, 4), f32)
    m = C.c_int(0)
    rc = lib().rolo_ground_extract_patch(gm._h, 0.0, 0.0, 4.0, None, out.ctypes.data_as(C.POINTER(C.c_float)), 4, C.byref(m))
    assert rc == EINVAL and m.value == tw.extract_patch(cloud, 0.0, 0.0, 4.0).shape[0] > 4
    gm.setCloud(np.zeros((0, 4), f32))   # n = 0 empties the model
    assert code_of(s.solve, [[0, 0, 0]]) == ESTATE and code_of(gm.extractPatch, 0, 0, 1) == ESTATE
