"""CPU: Scan Context's constants through the library, the numpy statement tests/sc_twin.py on constructed descriptors, and the manager's rebuild period.
The twin is what tests/test_gpu_scancontext.py holds the HIP kernels to, so its own behaviour is pinned here on cases whose answer is known in advance."""
import ctypes as C

import numpy as np

import sc_twin as T
from rolo_amd import _lib
from rolo_amd.backend import ScanContextManager

f32 = np.float32
R, S = 20, 60


def grid_cloud(heights, lidar_height=2.0, max_radius=80.0, turn=0):
    """one point in the middle of every bin whose height is not None: heights[r][s] is the bin's z'; `turn` moves every point on by that many sectors"""
    nr, ns = len(heights), len(heights[0])
    pts = []
    for r in range(nr):
        for s in range(ns):
            if heights[r][s] is None:
                continue
            rad = (r + 0.5) * max_radius / nr
            ang = np.deg2rad(((s + turn) % ns + 0.5) * 360.0 / ns)
            pts.append([rad * np.cos(ang), rad * np.sin(ang), heights[r][s] - lidar_height, 0.0])
    return np.array(pts, f32).reshape(-1, 4)


def test_default_params_are_the_reference_constants():
    """Scancontext.h:80-95 through rolo_sc_default_params (host only)"""
    p = _lib.ScParams()
    _lib.lib().rolo_sc_default_params(C.byref(p))
    got = dict(num_ring=p.num_ring, num_sector=p.num_sector, max_radius=p.max_radius, lidar_height=p.lidar_height, num_exclude_recent=p.num_exclude_recent,
               num_candidates=p.num_candidates, search_ratio=p.search_ratio, dist_thres=p.dist_thres)
    assert got == dict(num_ring=20, num_sector=60, max_radius=80.0, lidar_height=2.0, num_exclude_recent=30, num_candidates=3, search_ratio=0.1, dist_thres=0.4)
    assert got == T.DEFAULTS


def test_grid_cloud_fills_the_bins_it_names():
    rng = np.random.default_rng(1)
    h = [[float(rng.integers(1, 64)) / 8.0 if rng.random() < 0.7 else None for _ in range(S)] for _ in range(R)]
    d = T.make_scancontext(grid_cloud(h))
    want = np.array([[0.0 if v is None else v for v in row] for row in h])
    assert np.array_equal(d, want)


def test_rotation_by_whole_sectors_is_found_with_its_direction():
    """A cloud turned about z by +k sectors (counter-clockwise, every angle k sectors larger) has the original's columns k places further on: query column j is
    the original's column j - k. circshift (:39-59) moves the candidate's columns to the RIGHT, shifted[j] = original[j - s], so the query turned by +k against the
    original reports alignment k, and the original against the turned cloud reports S - k."""
    rng = np.random.default_rng(2)
    h = [[float(rng.integers(1, 64)) / 8.0 if rng.random() < 0.6 else None for _ in range(S)] for _ in range(R)]
    for k in (1, 7, 29, 31, 59):
        st = T.Store()
        st.add(grid_cloud(h)); st.add(grid_cloud(h, turn=k))
        fwd = st.detect(1, 1)
        assert fwd["min_dist"] < 0.05 and fwd["nn_align"] == k and fwd["loop_id"] == 0
        assert fwd["yaw"] == T.deg2rad(k * 6.0)
        d01, a01 = T.distance(st.entries[0], st.entries[1], 0.1)
        assert d01 < 0.05 and a01 == S - k


def no_overlap_pair(sa=10, sb=30):
    """one occupied sector each, heights +1 and -1 in two rings: the column mean is exactly 0, so both sector keys are all zero, every shift of the sector-key
    alignment has norm 0 and the first strict minimum below 10 000 000 is shift 0. The window is then 0 +- 3 of 60 shifts (search_ratio 0.1) and the two occupied
    sectors, 20 apart, never coincide in it"""
    def one(s):
        h = [[None] * S for _ in range(R)]
        h[3][s] = 1.0; h[4][s] = -1.0
        return grid_cloud(h)
    return one(sa), one(sb)


def test_no_overlap_keeps_the_initial_distance():
    a, b = no_overlap_pair()
    st = T.Store()
    st.add(a); st.add(b)
    assert not st.entries[0][2].any() and not st.entries[1][2].any()
    assert T.fast_align(st.entries[1][2], st.entries[0][2]) == 0
    r = st.detect(1, 1)
    assert r["min_dist"] == 10000000.0 and r["nn_align"] == 0 and r["loop_id"] == -1 and r["nn_idx"] == 0 and r["yaw"] == f32(0.0)
    # at shift 20 they do coincide: the exhaustive window finds it
    st.P["search_ratio"] = 1.0
    r = st.detect(1, 1)
    assert r["nn_align"] == 20 and r["min_dist"] < 1e-12 and r["loop_id"] == 0


STAIRCASE = [1] * 10 + [11] * 10 + [21] * 5   # :263-282: one descriptor and one detection per key frame, 30 excluded, the searched set re-taken on every tenth call


def test_twin_manager_rebuild_period():
    m = T.Manager()
    cloud = grid_cloud([[1.0] * S for _ in range(R)])
    for _ in range(55):
        m.makeAndSaveScancontextAndKeys(cloud)
        m.detectLoopClosureID()
    assert m.searched[:30] == [None] * 30 and m.searched[30:] == STAIRCASE


class FakeKeyMap:
    """the calls ScanContextManager makes, without a device: counts descriptors and records what is searched"""

    def __init__(self):
        self.n = 0
        self.calls = []

    def scParams(self):
        p = _lib.ScParams()
        _lib.lib().rolo_sc_default_params(C.byref(p))
        return p

    def scSetParams(self, p):
        self.params = p

    def scAddCloud(self, pts, leaf):
        self.n += 1
        return self.n - 1

    def scSize(self):
        return self.n

    def scDetect(self, query, n_search):
        self.calls.append((query, n_search))
        r = _lib.ScResult()
        r.loop_id = -1
        return r


def test_manager_rebuild_period_is_the_reference_staircase():
    km = FakeKeyMap()
    m = ScanContextManager(km)
    out = []
    for k in range(55):
        assert m.makeAndSaveScancontextAndKeys(np.zeros((1, 4), f32)) == k
        out.append(m.detectLoopClosureID())
    assert all(o == (-1, f32(0.0)) for o in out)
    assert [c[1] for c in km.calls] == STAIRCASE            # the first 30 calls return early and search nothing
    assert [c[0] for c in km.calls] == list(range(30, 55))   # the query is always the newest descriptor
