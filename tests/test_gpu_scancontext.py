"""GPU: Scan Context on the key map (rolo_keymap_sc_*, rolo_amd/csrc/scancontext.hip) against the numpy statement tests/sc_twin.py, bit for bit: every
comparison is np.array_equal (descriptors also by sign bit) or == on what the twin computes — no tolerance, no excluded case."""
import numpy as np
import pytest

import sc_twin as T
from oracle import pyorc
from rolo_amd import synth
from rolo_amd._lib import RoloError
from rolo_amd.backend import KeyFrameMap, ScanContextManager
from test_scancontext_twin import grid_cloud, no_overlap_pair

pytestmark = pytest.mark.gpu

f32 = np.float32
R, S = 20, 60
POSE0 = np.zeros(6, f32)


def cloud_of(xyz):
    a = np.zeros((len(xyz), 4), f32)
    a[:, :3] = np.asarray(xyz, f32).reshape(-1, 3)
    return a


def random_cloud(n, seed, radius=90.0):
    rng = np.random.default_rng(seed)
    return cloud_of(np.concatenate([rng.uniform(-radius, radius, (n, 2)), rng.uniform(-4.0, 12.0, (n, 1))], 1))


def make_map(**kw):
    km = KeyFrameMap()
    p = km.scParams()
    for k, v in kw.items():
        setattr(p, k, v)
    km.scSetParams(p)
    return km, p


def same_entry(got, want):
    """(desc, ring key, sector key, column norms) of the device against the twin's entry"""
    ok = all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))
    return ok and np.array_equal(np.signbit(got[0]), np.signbit(want[0]))


def check_cloud(pts, leaf=0.0, **kw):
    km, _ = make_map(**kw)
    try:
        st = T.Store(**kw)
        i = km.scAddCloud(pts, leaf)
        assert i == 0 and km.scSize() == 1
        assert st.add(pts) == 0
        assert same_entry(km.scDescriptor(0), st.entries[0])
        return st.entries[0][0]
    finally:
        km.close()


# ---- 1. the descriptor -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 20000])
def test_descriptor_cloud_sizes(n):
    d = check_cloud(random_cloud(n, 100 + n))
    assert n < 64 or np.count_nonzero(d) > 0


def test_descriptor_contention_in_one_bin():
    rng = np.random.default_rng(7)
    xyz = np.stack([rng.uniform(10.1, 11.9, 5000), rng.uniform(0.1, 0.9, 5000), rng.uniform(-3.0, 9.0, 5000)], 1)
    d = check_cloud(cloud_of(xyz))
    assert np.count_nonzero(d) == 1


def test_descriptor_ring_edges():
    """r = 4 k exactly (ceil keeps ring k), on the axes and as scaled (3, 4, 5) triples; r = 80 stays, the next float above it is dropped"""
    pts = [[4.0 * k, 0.0, 0.1 * k] for k in range(1, 21)] + [[0.0, -4.0 * k, 0.2 * k] for k in range(1, 21)]
    pts += [[3.0 * m, 4.0 * m, 1.0 + m] for m in (0.8 * 5, 4.0, 8.0, 12.0, 16.0)] + [[-12.0, 16.0, 3.0], [-24.0, -32.0, 4.0], [48.0, -64.0, 5.0]]
    up = np.nextafter(f32(80.0), f32(np.inf))
    pts += [[80.0, 0.0, 7.0], [float(up), 0.0, 50.0], [0.0, 80.0, 7.5], [0.0, float(up), 50.0], [-float(up), 0.0, 50.0]]
    d = check_cloud(cloud_of(pts))
    assert d.max() < 50.0 and d[19, 0] == 9.0   # (80, 0, 7): ring 20, sector 1; nothing from beyond the radius


def test_descriptor_axis_and_signed_zero_cases():
    """xy2theta's branches at their seams: the origin (NaN angle, sector 1), x = 0 with y of both signs (quotient +-inf), y = 0 with x of both signs, and
    -0.0f in either coordinate (it passes >= 0)"""
    nz = -0.0
    pts = [[0.0, 0.0, 1.0], [0.0, 5.0, 1.5], [0.0, -5.0, 2.0], [9.0, 0.0, 2.5], [-9.0, 0.0, 3.0], [nz, 13.0, 3.5], [nz, -13.0, 4.0], [17.0, nz, 4.5], [-17.0, nz, 5.0],
           [nz, nz, 5.5], [nz, 0.0, 0.5], [0.0, nz, 0.25]]
    for one in pts:   # each alone, so no case hides behind another's maximum
        check_cloud(cloud_of([one]))
    check_cloud(cloud_of(pts))


def test_descriptor_no_point_rule():
    """z' = -1000 exactly and below never enter a bin (:158-190); a negative z' above -1000 does; a bin holding only the former is 0"""
    rows = [(5.0, -1002.0), (9.0, -1003.0), (13.0, -500.0), (17.0, -1001.9), (21.0, -1002.0), (21.1, -1003.0), (25.0, -1002.0), (25.1, -3.0), (29.0, -2.0)]
    d = check_cloud(cloud_of([[x, 0.05 * x, z] for x, z in rows]))   # all in sector 1; rings 2, 3, ... 8
    assert d[1, 0] == 0 and d[2, 0] == 0 and d[3, 0] == -498.0 and -1000.0 < d[4, 0] < -999.0 and d[5, 0] == 0 and d[6, 0] == -1.0 and d[7, 0] == 0
    assert np.count_nonzero(d) == 3


def test_descriptor_all_out_of_range():
    xyz = random_cloud(300, 5)[:, :3]
    xyz[:, 0] = np.where(xyz[:, 0] >= 0, 81.0, -81.0) + xyz[:, 0]
    d = check_cloud(cloud_of(xyz))
    assert not d.any()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_descriptor_non_finite_is_an_error_and_stores_nothing(bad):
    km, _ = make_map()
    try:
        good = random_cloud(500, 11)
        assert km.scAddCloud(good, 0.0) == 0
        for col in range(3):
            pts = random_cloud(300, 12)
            pts[177, col] = bad
            with pytest.raises(RoloError) as e:
                km.scAddCloud(pts, 0.0)
            assert e.value.code == -11 and km.scSize() == 1
        other = random_cloud(400, 13)
        assert km.scAddCloud(other, 0.0) == 1
        st = T.Store(); st.add(good); st.add(other)
        assert same_entry(km.scDescriptor(0), st.entries[0]) and same_entry(km.scDescriptor(1), st.entries[1])
    finally:
        km.close()


def test_descriptor_empty_cloud_is_an_error():
    km, _ = make_map()
    try:
        with pytest.raises(RoloError) as e:
            km.scAddCloud(np.zeros((0, 4), f32), 0.0)
        assert e.value.code == -1 and km.scSize() == 0
        k = km.addKeyFrame(random_cloud(10, 1), np.zeros((0, 4), f32), POSE0, 0.0)
        with pytest.raises(RoloError) as e:
            km.scAddSurface(k)
        assert e.value.code == -1 and km.scSize() == 0
    finally:
        km.close()


def test_descriptor_from_resident_surface_equals_from_host_points():
    km, _ = make_map()
    try:
        clouds = [random_cloud(3000 + 17 * k, 20 + k) for k in range(3)]
        for k, c in enumerate(clouds):
            assert km.addKeyFrame(random_cloud(50, 40 + k), c, POSE0, float(k)) == k
        for k in (2, 0, 1):
            km.scAddSurface(k)
        for k in (2, 0, 1):
            km.scAddCloud(clouds[k], 0.0)
        st = T.Store()
        for j, k in enumerate((2, 0, 1)):
            st.add(clouds[k])
            a, b = km.scDescriptor(j), km.scDescriptor(j + 3)
            assert same_entry(a, b) and same_entry(a, st.entries[j])
    finally:
        km.close()


def test_descriptor_with_leaf_equals_twin_of_the_oracle_filter():
    """downSizeFilterSC (backMapping.cpp:1186-1196) on the device, then the descriptor"""
    pts = random_cloud(20000, 31, radius=40.0)
    pts[:, 3] = np.arange(len(pts), dtype=f32)
    km, _ = make_map()
    try:
        assert km.scAddCloud(pts, 0.5) == 0
        ds = pyorc.voxelgrid(pts, 0.5)
        assert 0 < len(ds) < len(pts)
        st = T.Store(); st.add(ds)
        assert same_entry(km.scDescriptor(0), st.entries[0])
    finally:
        km.close()


def test_descriptor_other_geometry():
    kw = dict(num_ring=16, num_sector=40, max_radius=50.0, lidar_height=0.0)
    d = check_cloud(random_cloud(5000, 41, radius=60.0), **kw)
    assert d.shape == (16, 40) and np.count_nonzero(d) > 300
    check_cloud(random_cloud(777, 42, radius=20.0), num_ring=7, num_sector=13, max_radius=25.0, lidar_height=-1.5)   # ring key with a tail of single terms


def test_detection_other_geometry():
    """7 rings: the ring-key distance is one group of four and a tail of three single terms; 13 sectors: a window that is not 60 wide"""
    kw = dict(num_ring=7, num_sector=13, max_radius=25.0, lidar_height=-1.5, search_ratio=0.3)
    km, _ = make_map(**kw)
    try:
        st = T.Store(**kw)
        for i in range(40):
            c = random_cloud(80, 600 + i, radius=20.0)
            km.scAddCloud(c, 0.0); st.add(c)
        for n_search in (5, 39):
            res, idx, dist, align = km.scDetect(39, n_search, want_candidates=True)
            w = st.detect(39, n_search)
            assert idx.tolist() == w["cand"] and np.array_equal(dist, np.array(w["cand_dist"])) and align.tolist() == w["cand_align"]
            assert (res.loop_id, res.nn_idx, res.nn_align, res.min_dist, f32(res.yaw_diff_rad)) == (w["loop_id"], w["nn_idx"], w["nn_align"], w["min_dist"], w["yaw"])
    finally:
        km.close()


def test_geometry_change_after_a_failed_first_add_resizes_the_store():
    """a first add that fails has already sized the store for 20 x 60; nothing is stored, so a larger geometry is accepted and the store must follow it:
    100 descriptors of 64 x 64 (past the first growth step) equal the twin's, and the first ones are still intact at the end"""
    km, p = make_map()
    try:
        bad = random_cloud(100, 50); bad[7, 1] = np.nan
        with pytest.raises(RoloError) as e:
            km.scAddCloud(bad, 0.0)
        assert e.value.code == -11 and km.scSize() == 0
        kw = dict(num_ring=64, num_sector=64, max_radius=70.0, lidar_height=1.0)
        for k, v in kw.items():
            setattr(p, k, v)
        km.scSetParams(p)
        p.num_sector = 60   # the caller's struct changed after the call: the getter sizes its buffers from the library's parameters
        q = km.scGetParams()
        assert (q.num_ring, q.num_sector, q.max_radius, q.lidar_height) == (64, 64, 70.0, 1.0)
        st = T.Store(**kw)
        for i in range(100):
            c = random_cloud(400, 700 + i, radius=75.0)
            assert km.scAddCloud(c, 0.0) == i == st.add(c)
        for i in (0, 18, 19, 63, 64, 65, 99):
            assert same_entry(km.scDescriptor(i), st.entries[i])
        res, idx, dist, align = km.scDetect(99, 99, want_candidates=True)
        w = st.detect(99, 99)
        assert idx.tolist() == w["cand"] and np.array_equal(dist, np.array(w["cand_dist"])) and align.tolist() == w["cand_align"]
    finally:
        km.close()


def test_descriptor_tiny_coordinates():
    """x * x below the smallest normal float (and below the smallest float at all): r is tiny or 0, ring 1 either way; the quotient y / x is an ordinary float"""
    pts = [[1e-20, 2e-20, 1.0], [-3e-21, 1e-20, 2.0], [1e-30, -1e-30, 3.0], [-1e-38, -3e-39, 4.0], [1e-45, 1e-45, 5.0], [1e-23, 0.0, 6.0]]
    for one in pts:
        check_cloud(cloud_of([one]))
    check_cloud(cloud_of(pts))


def test_geometry_is_fixed_once_a_descriptor_is_stored():
    km, p = make_map()
    try:
        km.scAddCloud(random_cloud(100, 3), 0.0)
        p.search_ratio = 1.0; p.num_candidates = 0
        km.scSetParams(p)
        p.num_sector = 40
        with pytest.raises(RoloError) as e:
            km.scSetParams(p)
        assert e.value.code == -5
        for bad in (dict(num_ring=100, num_sector=60), dict(num_sector=1025, num_ring=1), dict(num_candidates=65)):
            q = km.scParams()
            for k, v in bad.items():
                setattr(q, k, v)
            with pytest.raises(RoloError) as e:
                km.scSetParams(q)
            assert e.value.code == -1
    finally:
        km.close()


# ---- 2. candidates and distances over one store -------------------------------------------------------------------------------------------------------------
N_STORE = 1100
DUPES = {3: 0, 40: 0, 200: 0, 1000: 0, 1099: 0, 64: 1, 65: 1, 500: 1}   # index -> which repeated cloud sits there


@pytest.fixture(scope="module")
def store():
    """1 100 descriptors of small random clouds on the device and in the twin; some clouds repeat (equal ring keys and distances); the last one is the query"""
    km, p = make_map()
    st = T.Store()
    rep = [random_cloud(60, 900), random_cloud(60, 901)]
    for i in range(N_STORE):
        c = rep[DUPES[i]] if i in DUPES else random_cloud(30 + i % 50, 1000 + i, radius=70.0)
        assert km.scAddCloud(c, 0.0) == i
        st.add(c)
    yield km, p, st
    km.close()


def detect_both(store, query, n_search, **kw):
    km, p, st = store
    for k, v in kw.items():
        setattr(p, k, v)
    km.scSetParams(p)
    st.P.update(kw)
    res, idx, dist, align = km.scDetect(query, n_search, want_candidates=True)
    return res, idx, dist, align, st


def test_store_entries_equal_the_twin(store):
    km, _, st = store
    for i in (0, 1, 63, 64, 65, 511, 1024, 1099):   # across the store's growth steps
        assert same_entry(km.scDescriptor(i), st.entries[i])


@pytest.mark.parametrize("K", [1, 3, 10, 64])
@pytest.mark.parametrize("n_search", [1, 2, 3, 63, 65, 300, 1025])
def test_candidate_lists(store, K, n_search):
    res, idx, dist, align, st = detect_both(store, N_STORE - 1, n_search, num_candidates=K, search_ratio=0.1, dist_thres=0.4)
    want = T.candidates([e[1] for e in st.entries], N_STORE - 1, n_search, K)
    assert res.n_candidates == min(K, n_search) == len(want)
    assert idx.tolist() == want
    dup = [i for i in sorted(DUPES) if DUPES[i] == 0 and i < n_search][:K]
    assert idx.tolist()[:len(dup)] == dup   # equal (zero) distances: the lowest index first


@pytest.mark.parametrize("query,n_search,ratio", [(N_STORE - 1, 300, 0.1), (N_STORE - 1, 1025, 1.0), (65, 64, 0.1), (500, 300, 1.0), (777, 40, 0.1)])
def test_detection_equals_the_twin(store, query, n_search, ratio):
    res, idx, dist, align, st = detect_both(store, query, n_search, num_candidates=3, search_ratio=ratio, dist_thres=0.4)
    w = st.detect(query, n_search)
    assert idx.tolist() == w["cand"] and np.array_equal(dist, np.array(w["cand_dist"])) and align.tolist() == w["cand_align"]
    assert (res.loop_id, res.nn_idx, res.nn_align, res.min_dist) == (w["loop_id"], w["nn_idx"], w["nn_align"], w["min_dist"])
    assert f32(res.yaw_diff_rad) == w["yaw"]


def test_all_candidates_over_300(store):
    res, idx, dist, align, st = detect_both(store, N_STORE - 1, 300, num_candidates=0, search_ratio=0.1, dist_thres=0.4)
    w = st.detect(N_STORE - 1, 300)
    assert res.n_candidates == 300 and idx.tolist() == list(range(300))
    assert np.array_equal(dist, np.array(w["cand_dist"])) and align.tolist() == w["cand_align"]
    assert (res.loop_id, res.nn_idx, res.nn_align, res.min_dist) == (w["loop_id"], w["nn_idx"], w["nn_align"], w["min_dist"])
    assert res.nn_idx == 3   # the first of the query's copies


def test_threshold_either_side_of_the_minimum(store):
    res, *_ = detect_both(store, 777, 300, num_candidates=10, search_ratio=0.1, dist_thres=0.4)
    m = res.min_dist
    assert 0.0 < m < 10000000.0
    r2, *_ = detect_both(store, 777, 300, dist_thres=m)                        # strict <: not a loop at the minimum itself
    assert r2.loop_id == -1 and r2.nn_idx == res.nn_idx and r2.min_dist == m
    r3, *_ = detect_both(store, 777, 300, dist_thres=float(np.nextafter(m, np.inf)))
    assert r3.loop_id == res.nn_idx and r3.yaw_diff_rad == res.yaw_diff_rad


def test_early_return(store):
    km, _, _ = store
    for n in (0, -5):
        r = km.scDetect(5, n)
        assert (r.loop_id, r.yaw_diff_rad, r.n_candidates) == (-1, 0.0, 0)


# ---- 3. the distance on constructed descriptors ----------------------------------------------------------------------------------------------------------------
def heights(seed, empty_cols=()):
    rng = np.random.default_rng(seed)
    h = [[float(rng.integers(-16, 80)) / 8.0 if rng.random() < 0.7 else None for _ in range(S)] for _ in range(R)]
    for r in range(R):
        for s in empty_cols:
            h[r][s] = None
    return h


def pair_case(clouds, ratios=(0.1, 1.0)):
    """descriptors of `clouds`; the last is the query, searched against all before it, every one a candidate"""
    km, p = make_map(num_candidates=0)
    try:
        st = T.Store(num_candidates=0)
        for c in clouds:
            km.scAddCloud(c, 0.0); st.add(c)
        n = len(clouds)
        out = []
        for ratio in ratios:
            p.search_ratio = ratio; km.scSetParams(p); st.P["search_ratio"] = ratio
            res, idx, dist, align = km.scDetect(n - 1, n - 1, want_candidates=True)
            w = st.detect(n - 1, n - 1)
            assert np.array_equal(dist, np.array(w["cand_dist"])) and align.tolist() == w["cand_align"]
            assert (res.loop_id, res.nn_idx, res.nn_align, res.min_dist, f32(res.yaw_diff_rad)) == (w["loop_id"], w["nn_idx"], w["nn_align"], w["min_dist"], w["yaw"])
            out.append((res, dist, align))
        return out
    finally:
        km.close()


def test_distance_empty_columns():
    ec = (0, 1, 17, 58, 59)
    clouds = [grid_cloud(heights(1, ec)), grid_cloud(heights(2)), grid_cloud(heights(3, ec)), grid_cloud(heights(4, (5, 6, 7))), grid_cloud(heights(5)),   # candidates
              grid_cloud(heights(6, (0, 30, 31)))]                                                                                                          # query: empty columns
    pair_case(clouds)
    pair_case(clouds[:5])   # query without empty columns against candidates with and without


def test_distance_no_overlap_pair():
    a, b = no_overlap_pair()
    (r01, d01, a01), (r10, d10, a10) = pair_case([a, b])
    assert d01[0] == 10000000.0 and a01[0] == 0 and r01.loop_id == -1 and r01.nn_idx == 0 and r01.yaw_diff_rad == 0.0
    assert a10[0] == 20 and r10.loop_id == 0


def test_distance_identical_descriptors():
    c = grid_cloud(heights(9))
    for res, dist, align in pair_case([c, c, c]):
        assert align.tolist() == [0, 0] and res.nn_idx == 0 and res.nn_align == 0 and abs(dist[0]) < 1e-12 and dist[0] == dist[1]


@pytest.mark.parametrize("turn", [0, 1, S - 1, 7, 31])
def test_distance_alignment_wraps(turn):
    """the sector-key alignment lands on `turn`; at 0, 1 and S - 1 the window of +-3 shifts wraps round the end"""
    h = heights(10 + turn)
    for res, dist, align in pair_case([grid_cloud(h), grid_cloud(heights(99)), grid_cloud(h, turn=turn)]):
        assert res.nn_idx == 0 and res.nn_align == turn and res.loop_id == 0 and abs(res.min_dist) < 1e-12


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------------------------------------------
def scene_pose(k):
    """an ellipse through the hall, one lap in 60 key frames: frame 70 stands where frame 10 stood, yawed by 48 degrees (eight sectors)"""
    kk = 10 if k == 70 else k
    phi = (kk - 10) * 2.0 * np.pi / 60.0
    yaw = 0.01 * kk + (np.deg2rad(48.0) if k == 70 else 0.0)
    return synth.rpy_to_R(0.0, 0.0, yaw), np.array([20.0 * np.cos(phi), 12.0 * np.sin(phi), 0.0])


def test_manager_call_for_call_on_a_revisited_place():
    """80 key frames of VLP-16 surface features (every eighth firing column: the ray-cast is the cost of this test), ScanContextManager against the twin's
    manager call for call. Checked on the CPU before the scene was fixed: the twin finds frame 70's loop with key frame 10, 52 sectors (360 - 48 degrees)."""
    fo = pyorc.front_params(n_scan=16, horizon_scan=1800)
    km = KeyFrameMap()
    try:
        gm, tm = ScanContextManager(km), T.Manager()
        got, want = [], []
        for k in range(80):
            Rk, tk = scene_pose(k)
            fr = synth.make_frame("vlp16", Rk, tk, synth.SEED + k, col_stride=8)
            surf = pyorc.extract_features(fo, pyorc.project(fo, fr.xyz, fr.ring))["surface"]
            assert gm.makeAndSaveScancontextAndKeys(surf) == k == tm.makeAndSaveScancontextAndKeys(surf)
            got.append(gm.detectLoopClosureID()); want.append(tm.detectLoopClosureID())
            if k >= 30:
                assert (gm.last.nn_idx, gm.last.nn_align, gm.last.min_dist) == (tm.last["nn_idx"], tm.last["nn_align"], tm.last["min_dist"])
        assert [g[0] for g in got] == [w[0] for w in want]
        assert all(g[1] == w[1] and g[1].dtype == w[1].dtype for g, w in zip(got, want))
        assert got[70][0] == 10 and gm.last is not None and want[70][1] == T.deg2rad(52 * 6.0)
        assert all(g == (-1, f32(0.0)) for g in got[:30])
    finally:
        km.close()
