"""GPU: Scan Context (rolo_amd/csrc/scancontext.hip) on the constructed clouds of tests/sc_cases.py, at the geometry limits the header promises, and over a store
past 2^14 descriptors. Everything goes through KeyFrameMap.scSetParams / scAddCloud / scAddSurface / scDescriptor / scDetect and every comparison is
np.array_equal or == — no tolerance, no excluded point.

The planted clouds (sector edges, the guard zone of sc_theta, ring edges) are held to the CORRECTLY ROUNDED statement of sc_cases (sc_twin's expressions on an
atan rounded once from 200 bits), whatever the host libm does on them; the limit geometries and the large store hold random clouds, which are compared with
sc_twin as it is, as in test_gpu_scancontext.py."""
import numpy as np
import pytest

import sc_cases as sc
import sc_twin as T
from test_gpu_scancontext import POSE0, make_map, random_cloud, same_entry
from test_scancontext_twin import grid_cloud

pytestmark = pytest.mark.gpu

f32 = np.float32
BUILT = sc.build
N_SUITES = {"sectors": len(sc.SECTOR_GEOMS), "guard": sum(P["num_sector"] % 4 == 0 for P in sc.SECTOR_GEOMS), "rings": len(sc.RING_GEOMS)}


def describe(suite, ci, cloud, got, want):
    """the bins in which the device's descriptor of one cloud differs from the statement's, with the planted points that reserve them"""
    lines = ["%s cloud %d (%d points): descriptor differs in %d bins; ring key %s, sector key %s, column norms %s"
             % (suite.name, ci, len(cloud), int((got[0] != want[0]).sum()), *("equal" if np.array_equal(g, w) else "DIFFERS" for g, w in zip(got[1:], want[1:])))]
    owner = {b: p for p in suite.points if p.cloud == ci for b in p.bins}
    for r, s in np.argwhere(got[0] != want[0])[:16]:
        p = owner.get((r + 1, s + 1))
        lines.append("  ring %d sector %d: device %r, statement %r; planted point %s x=%s y=%s" % (r + 1, s + 1, got[0][r, s], want[0][r, s], p and p.meta, p and float(p.x).hex(), p and float(p.y).hex()))
    return "\n".join(lines)


def check_suite(suite, singles=False):
    """every cloud of the suite (and, with `singles`, every planted point alone) as a descriptor of one key map, each against the statement"""
    km, _ = make_map(**suite.P)
    try:
        clouds = list(suite.clouds) + ([sc.single_cloud(p) for p in suite.points] if singles else [])
        for i, c in enumerate(clouds):
            assert km.scAddCloud(c, 0.0) == i
        bad = []
        for i, c in enumerate(clouds):
            got, want = km.scDescriptor(i), sc.expected(c, suite.P)
            if not same_entry(got, want):
                bad.append(describe(suite, i, c, got, want))
        assert not bad, "%d of %d clouds differ\n" % (len(bad), len(clouds)) + "\n".join(bad[:8])
    finally:
        km.close()


# ---- 1. planted descriptors -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", range(N_SUITES["sectors"]))
def test_sector_edges(g):
    """(a): adjacent quotient floats across every sector edge, the float angles that equal an edge among them"""
    check_suite(BUILT()["sectors"][g])


@pytest.mark.parametrize("g", range(N_SUITES["guard"]))
def test_guard_zone(g):
    """(b): quotients whose fp64 angle lies within and just beyond 1e-10 of the midpoint that decides the sector at 90, 180 and 270 degrees, the denormal and
    infinite quotients beside 0 and 360: in their clouds, and each alone in a cloud of one"""
    check_suite(BUILT()["guard"][g], singles=True)


@pytest.mark.parametrize("g", range(N_SUITES["rings"]))
def test_ring_edges(g):
    """(c): adjacent float radii across every ring edge and across max_radius, on the axes and off them, at geometries whose edges or max_radius are no floats"""
    check_suite(BUILT()["rings"][g])


def test_sector_edge_cloud_from_a_resident_surface():
    """the S = 60 edge clouds as key frames' surface clouds: scAddSurface gives the bytes of scAddCloud, and both the statement's"""
    suite = BUILT()["sectors"][0]
    km, _ = make_map(**suite.P)
    try:
        n = len(suite.clouds)
        for k, c in enumerate(suite.clouds):
            assert km.addKeyFrame(random_cloud(20, 70 + k), c, POSE0, float(k)) == k
        for k in range(n):
            assert km.scAddSurface(k) == k
        for k, c in enumerate(suite.clouds):
            assert km.scAddCloud(c, 0.0) == n + k
        for k, c in enumerate(suite.clouds):
            a, b = km.scDescriptor(k), km.scDescriptor(n + k)
            assert same_entry(a, b) and same_entry(a, sc.expected(c, suite.P))
    finally:
        km.close()


# ---- 2. the geometry limits -------------------------------------------------------------------------------------------------------------------------------------
def memo_distance(monkeypatch):
    """sc_twin.distance remembered per (entries, search_ratio): the same pair is asked for with num_candidates 0 and 3. The key is the identity of the two
    entry tuples: Store.entries keeps them alive and Store.detect passes them on as they are, so within one test an id names one entry. Only the twin's run
    time depends on this, nothing that is compared"""
    real, memo = T.distance, {}

    def distance(e1, e2, ratio):
        key = (id(e1), id(e2), ratio)
        if key not in memo:
            memo[key] = real(e1, e2, ratio)
        return memo[key]
    monkeypatch.setattr(T, "distance", distance)


def same_detection(km, p, st, query, n_search, **kw):
    for k, v in kw.items():
        setattr(p, k, v)
    km.scSetParams(p)
    st.P.update(kw)
    res, idx, dist, align = km.scDetect(query, n_search, want_candidates=True)
    w = st.detect(query, n_search)
    assert idx.tolist() == w["cand"] and np.array_equal(dist, np.array(w["cand_dist"])) and align.tolist() == w["cand_align"]
    assert (res.loop_id, res.nn_idx, res.nn_align, res.min_dist, f32(res.yaw_diff_rad)) == (w["loop_id"], w["nn_idx"], w["nn_align"], w["min_dist"], w["yaw"])
    assert f32(res.yaw_diff_rad).dtype == w["yaw"].dtype
    return res, w


@pytest.mark.parametrize("R,S", [(4, 1024), (1, 1024), (4096, 1), (2, 2), (15, 257), (3, 683)])
def test_limit_geometries(R, S, monkeypatch):
    """num_sector = 1024 and num_ring * num_sector = 4096, the limits of rolo_hip.h: the distance kernel's loop over more than 256 shifts, rounds of 2048 / S < 32
    shifts with a shorter last one, a ring key longer than 256; and the degenerate ends (one sector, one ring). Four descriptors, the last against the other three"""
    memo_distance(monkeypatch)
    kw = dict(num_ring=R, num_sector=S, max_radius=80.0, lidar_height=2.0)
    km, p = make_map(**kw)
    try:
        st = T.Store(**kw)
        for i in range(4):
            c = random_cloud(3000, 4000 + 10 * R + S + i)
            assert km.scAddCloud(c, 0.0) == i == st.add(c)
            assert same_entry(km.scDescriptor(i), st.entries[i])
        for ratio in (0.1, 1.0):
            for K in (0, 3):
                res, w = same_detection(km, p, st, 3, 3, num_candidates=K, search_ratio=ratio, dist_thres=0.4)
                assert res.n_candidates == 3
    finally:
        km.close()


def test_alignment_past_256_and_768_sectors():
    """S = 1024: a cloud turned by 300 and by 800 whole sectors. Each thread of the sector-key alignment takes the shifts tid + 256 j: the minimum is one that a
    thread finds on its second, respectively fourth, trip, and the alignment found is the turn"""
    R, S = 4, 1024
    kw = dict(num_ring=R, num_sector=S, max_radius=80.0, lidar_height=2.0, num_candidates=0, search_ratio=0.1)
    rng = np.random.default_rng(5)
    h = [[float(rng.integers(1, 64)) / 8.0 if rng.random() < 0.6 else None for _ in range(S)] for _ in range(R)]
    km, p = make_map(**kw)
    try:
        st = T.Store(**kw)
        for turn in (0, 300, 800):
            c = grid_cloud(h, turn=turn)
            km.scAddCloud(c, 0.0); st.add(c)
        for query, turn in ((1, 300), (2, 800)):
            res, w = same_detection(km, p, st, query, 1)
            assert (res.nn_idx, res.nn_align, res.loop_id) == (0, turn, 0)   # min_dist is the twin's, bit for bit (same_detection)
    finally:
        km.close()


# ---- 3. a store past 2^14 descriptors -----------------------------------------------------------------------------------------------------------------------------
N_BIG = 16900
TRIP = 64 * 256                                    # the ring-key search's stride: SC_RK_BLOCKS workgroups of SC_THREADS
QUERY = N_BIG - 1
# the query's cloud again at: one thread's first and second trip, either side of the first workgroup's end, either side of the stride, the last searched index
COPIES = (5, 5 + TRIP, 255, 256, TRIP - 1, TRIP, N_BIG - 2)
OTHER = (9, 9 + TRIP, 16640)                       # a second repeated cloud, queried from its last copy
PAST = (11 + TRIP, 16500, 16850)                   # a third one, queried from its last copy: its only other copies are keys of a second trip
BIG = dict(num_ring=5, num_sector=4, max_radius=80.0, lidar_height=2.0)   # a ring key of one group of four and a tail of one


@pytest.fixture(scope="module")
def big_store():
    km, p = make_map(**BIG)
    st = T.Store(**BIG)
    rng = np.random.default_rng(20261020)
    pts = np.zeros((N_BIG, 6, 4), f32)
    pts[:, :, :2] = rng.uniform(-70.0, 70.0, (N_BIG, 6, 2))
    pts[:, :, 2] = rng.uniform(-1.0, 9.0, (N_BIG, 6))
    for i in COPIES:
        pts[i] = pts[QUERY]
    for i in OTHER[1:]:
        pts[i] = pts[OTHER[0]]
    for i in PAST[1:]:
        pts[i] = pts[PAST[0]]
    for i in range(N_BIG):
        assert km.scAddCloud(pts[i], 0.0) == i
        st.add(pts[i])
    yield km, p, st
    km.close()


def test_big_store_entries_equal_the_twin(big_store):
    km, _, st = big_store
    assert km.scSize() == N_BIG >= 16641
    for i in (0, 5, 255, 256, TRIP - 1, TRIP, TRIP + 5, 16640, N_BIG - 2, N_BIG - 1):
        assert same_entry(km.scDescriptor(i), st.entries[i])


@pytest.mark.parametrize("K", [1, 3, 64])
@pytest.mark.parametrize("n_search", [TRIP, TRIP + 1, TRIP + 256, TRIP + 257, N_BIG - 1])
def test_big_store_candidate_lists(big_store, n_search, K):
    """64 workgroups, and from 16 385 searched keys on a second trip through the stride loop for the first 1, 256, 257 and 515 threads: the candidate list is
    sc_twin's, the query's copies come first in index order (equal distances: the lower index), and at K = 3 the whole detection is the twin's. The copies
    past the stride (16 384, 16 389, 16 898) are candidates only at K = 64: at K = 1 and 3 the list ends before them"""
    km, p, st = big_store
    for k, v in dict(num_candidates=K, search_ratio=0.1, dist_thres=0.4).items():
        setattr(p, k, v)
    km.scSetParams(p)
    st.P.update(num_candidates=K, search_ratio=0.1, dist_thres=0.4)
    res, idx, dist, align = km.scDetect(QUERY, n_search, want_candidates=True)
    want = T.candidates([e[1] for e in st.entries], QUERY, n_search, K)
    assert res.n_candidates == K == len(want) and idx.tolist() == want
    copies = [i for i in sorted(COPIES) if i < n_search]
    assert len(copies) == {TRIP: 4, TRIP + 1: 5, TRIP + 256: 6, TRIP + 257: 6, N_BIG - 1: 7}[n_search]
    assert idx.tolist()[:len(copies)] == copies[:K]
    if K == 3:
        same_detection(km, p, st, QUERY, n_search)


def test_big_store_second_group_of_copies(big_store):
    """queried from the second repeated cloud's last copy, 16 640 keys searched: its two other copies — one thread's first and second trip — come first"""
    km, p, st = big_store
    res, w = same_detection(km, p, st, OTHER[2], OTHER[2], num_candidates=64, search_ratio=0.1, dist_thres=0.4)
    assert w["cand"][:2] == list(OTHER[:2])


@pytest.mark.parametrize("K", [1, 3])
def test_big_store_nearest_keys_only_on_a_second_trip(big_store, K):
    """queried from the third repeated cloud's last copy, every key below it searched: the two keys at distance zero are ones a thread computes, and reads again
    in the selection, on its second trip through the stride loop, so already the first candidate of K = 1 and the first two of K = 3 depend on that trip"""
    km, p, st = big_store
    assert all(i >= TRIP for i in PAST)
    res, w = same_detection(km, p, st, PAST[2], PAST[2], num_candidates=K, search_ratio=0.1, dist_thres=0.4)
    assert w["cand"][:2] == list(PAST[:2])[:K] and res.nn_idx == PAST[0]


def test_big_store_every_descriptor_a_candidate(big_store):
    """num_candidates = 0 over the whole store: 16 899 workgroups of the distance kernel, every distance and alignment the twin's"""
    km, p, st = big_store
    res, w = same_detection(km, p, st, QUERY, N_BIG - 1, num_candidates=0, search_ratio=0.1, dist_thres=0.4)
    assert res.n_candidates == N_BIG - 1 and res.nn_idx == COPIES[0]
