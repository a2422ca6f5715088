"""GPU: the global map from resident key frames (rolo_keymap_global_*, rolo_amd/csrc/submap.hip; publishGlobalMap, reference src/backMapping.cpp:1611-1665, and
saveGlobalPCDs' cloudGlobal.pcd, :1546-1557) against the CPU oracle, bit for bit.

Targets: pyorc.voxelgrid over the concatenation composed as tests/test_gpu_keymap.py::oracle_extract composes it (pyorc.get_transformation +
pyorc.transform_cloud_f, per listed frame corner then surface), and a serial numpy statement of the same filter (np.add.at in point order) that `oracle` holds
against pyorc.voxelgrid on every input it is used for. Clouds are compared as uint32. Every streamed case asserts through globalInfo() that the streamed form
ran, with the expected number of batches."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyorc
from rolo_amd._lib import RoloError, lib
from rolo_amd.backend import KeyFrameMap, PoseGraph

pytestmark = pytest.mark.gpu

f32 = np.float32
EINVAL, ESTATE, ENONFINITE = -1, -5, -11
E4 = np.zeros((0, 4), f32)
ZERO_POSE = np.zeros(6, f32)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- the targets -----------------------------------------------------------------------------------------------------------------------------------------------

def cell_keys(pts, leaf):
    """pcl::VoxelGrid's cell index of every point as the int it is there (wrapping 32-bit), with the extents' and div_b's products"""
    inv = f32(1.0) / f32(leaf)
    mn, mx = pts[:, :3].min(axis=0), pts[:, :3].max(axis=0)
    ext = ((mx - mn).astype(f32) * inv).astype(np.int64) + 1
    lo = np.floor(mn * inv).astype(np.int64)
    div = np.floor(mx * inv).astype(np.int64) - lo + 1
    ijk = np.floor(pts[:, :3] * inv).astype(np.int64) - lo
    wide = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    key = ((wide + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)
    return key, int(ext[0] * ext[1] * ext[2]), int(div[0] * div[1] * div[2])


def serial_voxelgrid(pts, leaf, chunk=None):
    """cells ascending, per cell the four float sums taken serially in point order (np.add.at is unbuffered and in index order), / float(count).
    chunk: the WRONG statement a chunked filter would make, per-chunk partial sums added afterwards (what the crossing tests tell apart)"""
    if len(pts) == 0:
        return E4.copy()
    key, ext, _ = cell_keys(pts, leaf)
    assert ext <= 2 ** 31 - 1
    uniq, inv = np.unique(key, return_inverse=True)
    sums = np.zeros((len(uniq), 4), f32)
    if chunk is None:
        np.add.at(sums, inv, pts)
    else:
        for a in range(0, len(pts), chunk):
            part = np.zeros_like(sums)
            np.add.at(part, inv[a:a + chunk], pts[a:a + chunk])
            sums = (sums + part).astype(f32)
    return (sums / np.bincount(inv).astype(f32)[:, None]).astype(f32)


def oracle(pts, leaf):
    want = pyorc.voxelgrid(pts, leaf) if len(pts) else E4.copy()
    assert same(serial_voxelgrid(pts, leaf), want)               # the fast target equals the oracle on this input
    return want


def concat(frames, poses, indices):
    """the concatenation: per listed frame its corner, then its surface cloud, moved by the frame's pose (transformPointCloud, intensity copied)"""
    parts = [E4]
    for k in indices:
        p = [float(v) for v in poses[k]]
        T = pyorc.get_transformation(p[3], p[4], p[5], p[0], p[1], p[2])
        for cloud in frames[k][:2]:
            if len(cloud):
                moved = cloud.copy()
                moved[:, :3] = pyorc.transform_cloud_f(np.ascontiguousarray(cloud[:, :3]), T)
                parts.append(moved)
    return np.concatenate(parts)


def keymap_of(frames, poses=None):
    km = KeyFrameMap()
    for k, fr in enumerate(frames):
        assert km.addKeyFrame(fr[0], fr[1], fr[2] if poses is None else poses[k], 0.5 * k) == k
    return km


def run(km, indices, leaf, batch, total):
    """globalMap at `batch`, with the form and the batch count globalInfo() must report for `total` listed points"""
    km.setGlobalBatch(batch)
    got = km.globalMap(indices, leaf)
    info = km.globalInfo()
    assert info["points"] == total and info["cells"] == len(got)
    if total > batch:
        assert info["form"] == "streamed" and info["batches"] == -(-total // batch) and info["table"] >= info["cells"] > 0
    else:
        assert info["form"] == "one-shot" and info["batches"] == (1 if total else 0)
    return got


def cloud(rng, n, lo, hi):
    return np.concatenate([rng.uniform(lo, hi, (n, 3)), rng.uniform(0, 100, (n, 1))], axis=1).astype(f32)


# ---- 1. streamed form = oracle, smallest shapes ----------------------------------------------------------------------------------------------------------------

def _small_frames():
    """53 key frames of 50 .. 700 points on a slowly turning track; 40-44 without corner points, 45-49 without surface points, 50-52 empty"""
    rng = np.random.default_rng(111)
    frames = []
    for k in range(53):
        nc, ns = int(rng.integers(10, 200)), int(rng.integers(40, 500))
        c = cloud(rng, nc, [-8, -8, -1], [8, 8, 3]); s = cloud(rng, ns, [-8, -8, -1], [8, 8, 3])
        if 40 <= k < 45 or k >= 50:
            c = E4.copy()
        if k >= 45:
            s = E4.copy()
        pose = np.array([0.002 * k, -0.001 * k, 0.03 * k, 0.6 * k, 0.05 * k, 0.01 * k], f32)
        frames.append((c, s, pose))
    return frames


SMALL_LISTS = {
    "one_frame": [7],
    "two_small": [45, 46],
    "forty_frames": list(range(40)),
    "repeated_unordered": [11, 2, 7, 2, 30, 0, 9, 5, 11, 11, 39, 17, 3, 3, 28, 1, 36, 2],
    "empty_corner_clouds": [0, 40, 1, 41, 2, 3, 42, 43, 4, 5, 6, 44, 8, 9, 10, 12, 13, 14, 15, 16],
    "empty_surface_clouds": [45, 0, 46, 1, 2, 47, 3, 4, 5, 48, 49, 6, 8, 9, 10, 12, 13, 14, 15, 16],
    "frames_empty_in_both": [50, 0, 1, 51, 2, 3, 4, 5, 6, 8, 52, 9, 10, 12, 13, 14, 15, 16, 50],
    "only_empty_frames": [50, 51, 52],
    "empty_list": [],
}
STREAMED_AT_EVERY_BATCH = ("forty_frames", "repeated_unordered", "empty_corner_clouds", "empty_surface_clouds", "frames_empty_in_both")
LEAVES = (0.4, 1.0, 10.0)
MAX_BATCHES = 700            # a list is run at a batch size when it makes at most this many batches: batch 1 and 7 take the short lists


@pytest.fixture(scope="module")
def small():
    frames = _small_frames()
    poses = [fr[2] for fr in frames]
    cats = {name: concat(frames, poses, idx) for name, idx in SMALL_LISTS.items()}
    wants = {(name, leaf): oracle(cats[name], leaf) for name in SMALL_LISTS for leaf in LEAVES}
    return frames, cats, wants


@pytest.mark.parametrize("batch", [1, 7, 64, 255, 256, 257, 1000, 4096, 4097])
def test_streamed_form_equals_the_oracle(small, batch):
    frames, cats, wants = small
    km = keymap_of(frames)
    ran, streamed = [], 0
    for name, idx in SMALL_LISTS.items():
        total = len(cats[name])
        if total > MAX_BATCHES * batch:
            continue
        if total > batch:
            assert batch == 1 or total % batch != 0, name                 # a last batch that is not full
            streamed += 1
        for leaf in LEAVES:
            got = run(km, idx, leaf, batch, total)
            assert same(got, wants[name, leaf]), (name, leaf, len(got), len(wants[name, leaf]))
        ran.append(name)
    print(f"batch {batch}: {ran}")
    assert "one_frame" in ran and "two_small" in ran and "only_empty_frames" in ran and "empty_list" in ran
    assert streamed >= (1 if batch == 1 else 2)
    if batch >= 64:
        assert set(STREAMED_AT_EVERY_BATCH) <= set(ran) and all(len(cats[n]) > batch for n in STREAMED_AT_EVERY_BATCH)
    assert len(km.globalMap([], 1.0)) == 0 and km.globalInfo()["points"] == 0
    km.close()


# ---- 2. the chain that crosses batches -------------------------------------------------------------------------------------------------------------------------

def _crossing_case(name):
    rng = np.random.default_rng(202)
    if name == "one_cell_from_every_batch":
        # 5 000 points of magnitude 10^3 with random fractions in ONE cell of leaf 10, in three frames, at batch 64: 79 batches feed the one chain
        pts = np.concatenate([rng.uniform(0.5, 9.5, (5000, 3)) + np.array([1000.0, 2000.0, 1500.0]), rng.uniform(0, 1000, (5000, 1))], axis=1).astype(f32)
        return pts, 10.0, 64, [1700, 3900]
    # 16 cells of leaf 1 around (1000, 2000, 50), 4 000 points dealt at random: every batch of 256 reaches every cell
    pts = np.concatenate([rng.uniform(0.05, 3.95, (4000, 2)) + np.array([1000.0, 2000.0]), rng.uniform(50.05, 50.95, (4000, 1)), rng.uniform(0, 1000, (4000, 1))],
                         axis=1).astype(f32)
    return pts, 1.0, 256, [1111, 2500]


@pytest.mark.parametrize("name", ["one_cell_from_every_batch", "every_cell_from_four_batches"])
def test_a_cells_chain_crosses_the_batches(name):
    pts, leaf, batch, cuts = _crossing_case(name)
    parts = np.split(pts, cuts)
    frames = [(parts[0][:300], parts[0][300:], ZERO_POSE), (E4, parts[1], ZERO_POSE), (parts[2][:17], parts[2][17:], ZERO_POSE)]
    cat = concat(frames, [ZERO_POSE] * 3, [0, 1, 2])
    assert same(cat, pts)                                                   # the zero pose moves nothing
    want = oracle(cat, leaf)
    key, _, _ = cell_keys(cat, leaf)
    fed = {c: len(set((np.nonzero(key == c)[0] // batch).tolist())) for c in np.unique(key).tolist()}
    nb = -(-len(cat) // batch)
    if name == "one_cell_from_every_batch":
        assert len(want) == 1 and list(fed.values()) == [nb] and nb == 79
    else:
        assert len(want) == 16 and min(fed.values()) >= 4
    # the input tells the orders apart: partial sums per batch, added afterwards, are NOT the oracle's bits (else this test would be vacuous)
    chunked = serial_voxelgrid(cat, leaf, chunk=batch)
    differ = int((bits(chunked) != bits(want)).any(axis=1).sum())
    print(name, "cells", len(want), "batches", nb, "cells a chunked sum gets wrong:", differ)
    assert differ >= 1
    km = keymap_of(frames)
    got = run(km, [0, 1, 2], leaf, batch, len(cat))
    assert same(got, want)
    km.close()


# ---- 3. insertion places ---------------------------------------------------------------------------------------------------------------------------------------

def _comb(ncells, rng, step=2):
    """two points in each of ncells cells of leaf 1 along x, every `step`-th cell, away from the cell walls"""
    x = np.repeat(step * np.arange(ncells), 2) + rng.uniform(0.25, 0.75, 2 * ncells)
    return np.concatenate([x[:, None], rng.uniform(0.25, 0.75, (2 * ncells, 2)), rng.uniform(0, 10, (2 * ncells, 1))], axis=1).astype(f32)


def _shifted(dx=0.0, dz=0.0):
    return np.array([0, 0, 0, dx, 0, dz], f32)


def test_where_a_later_batch_inserts_its_cells():
    """translated copies of one small frame, one frame per batch: the later batch's cells against the table's, by construction and checked on the keys"""
    rng = np.random.default_rng(303)
    base = _comb(40, rng)
    n = len(base)
    poses = {"base": _shifted(), "up": _shifted(dz=3.0), "down": _shifted(dz=-3.0), "between": _shifted(dx=1.0), "far_up": _shifted(dz=6.0)}
    names = list(poses)
    frames = [(base[:30], base[30:], poses[k]) for k in names]
    at = {k: i for i, k in enumerate(names)}
    km = keymap_of(frames)
    plist = [poses[k] for k in names]
    cases = {
        "only_cells_above": (["base", "up"], lambda old, new: new.min() > old.max()),
        "only_cells_below": (["up", "base"], lambda old, new: new.max() < old.min()),
        "strictly_interleaved": (["base", "between"], lambda old, new: not set(old) & set(new) and len(old) == len(new) and
                                 (np.diff(np.concatenate([np.zeros(len(old)), np.ones(len(new))])[np.argsort(np.concatenate([old, new]))]) != 0).all()),
        "no_new_cell": (["base", "base"], lambda old, new: set(new) == set(old)),
        "only_new_cells": (["base", "far_up"], lambda old, new: not set(old) & set(new)),
        "all_of_them_in_turn": (["base", "up", "down", "between", "base", "far_up", "down", "between"], None),
    }
    for cname, (order, relation) in cases.items():
        idx = [at[k] for k in order]
        cat = concat(frames, plist, idx)
        if relation is not None:
            key, _, _ = cell_keys(cat, 1.0)
            old, new = np.unique(key[:n]).astype(np.int64), np.unique(key[n:]).astype(np.int64)
            assert relation(old, new), cname
        got = run(km, idx, 1.0, n, len(cat))
        assert km.globalInfo()["batches"] == len(order)
        assert same(got, oracle(cat, 1.0)), cname
        for other in (n - 1, n + 1, 13):                                    # and with the cuts inside the frames
            assert same(run(km, idx, 1.0, other, len(cat)), got), (cname, other)
    km.close()


@pytest.mark.parametrize("edge", [256, 4096])
def test_table_sizes_across_a_workgroup_edge(edge):
    """a comb of edge - 1 cells, then copies moved by one and two cells: the table holds edge - 1, edge, edge + 1 cells after its batches, and once more the same"""
    rng = np.random.default_rng(404)
    base = _comb(edge - 1, rng, step=1)
    n = len(base)
    plist = [_shifted(), _shifted(dx=1.0), _shifted(dx=2.0)]
    frames = [(E4, base, p) for p in plist]
    idx = [0, 1, 2, 0]
    cat = concat(frames, plist, idx)
    key, _, _ = cell_keys(cat, 1.0)
    sizes = [len(np.unique(key[:n * (b + 1)])) for b in range(4)]
    assert sizes == [edge - 1, edge, edge + 1, edge + 1]
    km = keymap_of(frames)
    got = run(km, idx, 1.0, n, len(cat))
    assert km.globalInfo()["table"] == edge + 1 and len(got) == edge + 1
    assert same(got, oracle(cat, 1.0))
    km.close()


# ---- 4. one-shot = streamed --------------------------------------------------------------------------------------------------------------------------------------

def test_one_shot_and_streamed_give_the_same_bytes(small):
    frames, cats, wants = small
    km = keymap_of(frames)
    for name in ("forty_frames", "repeated_unordered"):
        idx, total = SMALL_LISTS[name], len(cats[name])
        for leaf in LEAVES:
            a = run(km, idx, leaf, total, total)                            # batch = total: still one shot
            b = run(km, idx, leaf, total + 5, total)
            c = run(km, idx, leaf, total - 1, total)                        # two batches, the second of one point
            d = run(km, idx, leaf, 999, total)
            assert a.tobytes() == b.tobytes() == c.tobytes() == d.tobytes() and same(a, wants[name, leaf])
    # a contiguous list: loopFindNearKeyframes' cloud (rolo_keymap_loop_cloud) is the same statement
    for leaf in (0.4, 1.0):
        m = km.loopCloud(0, 20, 6, leaf=leaf)
        loop = km.loopCloudPoints(0, m)
        idx = list(range(14, 27))
        total = len(concat(frames, [fr[2] for fr in frames], idx))
        assert run(km, idx, leaf, 2 ** 20, total).tobytes() == loop.tobytes() and run(km, idx, leaf, 300, total).tobytes() == loop.tobytes()
    km.setGlobalBatch(0)                                                    # the default again
    assert km.globalMap(idx, 1.0).tobytes() == loop.tobytes() and km.globalInfo()["form"] == "one-shot"
    km.close()


# ---- 5. the sign-bit key -------------------------------------------------------------------------------------------------------------------------------------------

def test_cell_index_that_wraps_the_int_streamed():
    """a handful of points at the corners of a box of leaf 1 whose extents' product (1290^3) stays below INT32_MAX while div_b's (1291^3) passes it: the far
    corners' indices wrap negative and sort first, as the int does (the flipped sign bit); streamed at batch 2"""
    lo, hi = 0.5, 1290.4
    corners = np.array([[x, y, z] for z in (lo, hi) for y in (lo, hi) for x in (lo, hi)], f32)
    rng = np.random.default_rng(505)
    pts = np.concatenate([corners, corners[[7, 0, 5, 7, 2]] + f32(0.03), corners[[6, 7]] - np.array([0.0, 0.02, 0.01], f32)]).astype(f32)
    pts = np.concatenate([pts, rng.uniform(0, 1, (len(pts), 1)).astype(f32)], axis=1)[rng.permutation(len(pts))]
    frames = [(pts[:4], pts[4:9], ZERO_POSE), (pts[9:10], pts[10:], ZERO_POSE)]
    cat = concat(frames, [ZERO_POSE] * 2, [0, 1])
    key, ext, div = cell_keys(cat, 1.0)
    assert ext <= 2 ** 31 - 1 < div and (key < 0).any() and (key > 0).any()
    want = oracle(cat, 1.0)
    assert len(want) == 8 and want[0, 2] > 1000                           # a wrapped (negative) index comes first
    km = keymap_of(frames)
    assert same(run(km, [0, 1], 1.0, 2, len(cat)), want)
    assert same(run(km, [0, 1], 1.0, 64, len(cat)), want)
    km.close()


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_key_map_working(small):
    frames, cats, wants = small
    rng = np.random.default_rng(606)
    bad = cloud(rng, 200, [-5, -5, -1], [5, 5, 2]); bad[137, 1] = np.inf
    wide = np.array([[0, 0, 0, 1], [3000, 3000, 3000, 2], [1, 1, 1, 3], [2, 2, 2, 4]], f32)   # at leaf 0.4: more than INT32_MAX cells
    km = keymap_of(frames[:12] + [(E4, bad, ZERO_POSE), (wide[:1], wide[1:], ZERO_POSE)])
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    h = km._h
    out = np.zeros((8, 4), f32)
    assert lib().rolo_keymap_get_global_map(h, out.ctypes.data_as(fp), 8) == ESTATE          # get before the first map
    before = km.extractCloud(list(range(12))); sub_before = km.submap()

    def code(fn):
        with pytest.raises(RoloError) as ei:
            fn()
        return ei.value.code, str(ei.value)
    for batch in (2 ** 20, 64):                                                               # one-shot, streamed
        km.setGlobalBatch(batch)
        assert code(lambda: km.globalMap([0, 12, 1], 0.4))[0] == ENONFINITE
    km.setGlobalBatch(3)
    c, msg = code(lambda: km.globalMap([13], 0.4))
    assert c == EINVAL and "leaf size is too small" in msg                                    # the streamed form refuses PCL's copy-through ...
    km.setGlobalBatch(4)
    assert same(km.globalMap([13], 0.4), wide) and km.globalInfo()["form"] == "one-shot"      # ... the one-shot form keeps it
    assert code(lambda: km.globalMap([0, 14], 1.0))[0] == EINVAL                              # index outside the store
    assert code(lambda: km.globalMap([-1], 1.0))[0] == EINVAL
    assert code(lambda: km.globalCloud([0, 14]))[0] == EINVAL
    assert code(lambda: km.globalMap([0], 0.0))[0] == EINVAL and code(lambda: km.globalMap([0], -1.0))[0] == EINVAL
    for b in (-1, 2 ** 26 + 1):
        assert code(lambda: km.setGlobalBatch(b))[0] == EINVAL
    assert lib().rolo_keymap_get_global_map(h, out.ctypes.data_as(fp), 8) == ESTATE          # the failed call left no map
    km.setGlobalBatch(2 ** 26); km.setGlobalBatch(100)
    got = km.globalMap([0, 1], 10.0)
    assert len(got) > 1 and same(got, oracle(concat(frames, [f[2] for f in frames], [0, 1]), 10.0))
    small_out = np.zeros((len(got) - 1, 4), f32)
    assert lib().rolo_keymap_get_global_map(h, small_out.ctypes.data_as(fp), len(got) - 1) == EINVAL   # cap too small
    assert km.extractCloud(list(range(12))) == before
    sub_after = km.submap()
    assert sub_after[0].tobytes() == sub_before[0].tobytes() and sub_after[1].tobytes() == sub_before[1].tobytes() and len(sub_after[1]) > 0
    km.close()


# ---- 7. poses ----------------------------------------------------------------------------------------------------------------------------------------------------

def test_corrected_poses_change_the_map(small):
    frames, cats, wants = small
    frames = frames[:10]
    km = keymap_of(frames)
    idx = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 4]
    poses = [fr[2].copy() for fr in frames]
    total = len(concat(frames, poses, idx))
    first = run(km, idx, 0.4, 500, total)
    assert same(first, oracle(concat(frames, poses, idx), 0.4))
    poses[4] = (poses[4] + np.array([0.001, -0.002, 0.01, 0.3, -0.2, 0.05], f32)).astype(f32)
    km.setPose(4, poses[4])
    second = run(km, idx, 0.4, 500, total)
    assert second.tobytes() != first.tobytes() and same(second, oracle(concat(frames, poses, idx), 0.4))
    # PoseGraph.correctPoses: the odometry chain of these poses and one loop factor that disagrees with it
    g = PoseGraph()
    for p in poses:
        g.addOdomFactor(p)
    T = np.eye(4); T[:3, 3] = [-5.0, -0.3, 0.1]
    g.addBetween(9, 0, T, [1e-4] * 6)
    g.optimize()
    g.correctPoses(km)
    moved = [np.array(p, f32) for p in km.poses]
    assert max(np.abs(a - b).max() for a, b in zip(moved, poses)) > 1e-3
    third = run(km, idx, 0.4, 500, total)
    assert third.tobytes() != second.tobytes() and same(third, oracle(concat(frames, moved, idx), 0.4))
    g.close(); km.close()


# ---- 8. globalCloud ----------------------------------------------------------------------------------------------------------------------------------------------

def test_global_cloud_is_the_transformed_concatenation(small):
    frames, cats, wants = small
    km = keymap_of(frames)
    km.setGlobalBatch(257)
    for name in ("forty_frames", "repeated_unordered", "frames_empty_in_both", "only_empty_frames", "empty_list"):
        assert same(km.globalCloud(SMALL_LISTS[name]), cats[name]), name
    assert max(len(fr[0]) + len(fr[1]) for fr in frames[:40]) > 257                          # a frame larger than the batch
    idx = np.array(SMALL_LISTS["repeated_unordered"], np.int32)
    n = len(cats["repeated_unordered"])
    out = np.zeros((n, 4), f32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    assert lib().rolo_keymap_global_cloud(km._h, idx.ctypes.data_as(ip), len(idx), out.ctypes.data_as(fp), n - 1) == EINVAL
    assert not out.any()
    assert lib().rolo_keymap_global_cloud(km._h, idx.ctypes.data_as(ip), len(idx), out.ctypes.data_as(fp), n) == n and same(out, cats["repeated_unordered"])
    km.close()


# ---- 9. past 2^26 points, with a closed-form answer ---------------------------------------------------------------------------------------------------------------

def test_map_of_more_than_2_pow_26_points_in_closed_form():
    """One lattice frame of 2^16 points, 8 per cell of leaf 1 in a block of 32 x 16 x 16 cells, coordinates (cell + 1/4 or + 3/4) and intensities small dyadic
    values: every sum is exact in float in any order, so the answer follows from the set of tiles alone. 1 025 key frames hold it (the pose belongs to the key
    frame, so each translation is a key frame of its own: 1 GiB resident) under integer translations that tile a 32 x 32 grid, the last one an exact repeat;
    listed shuffled, 67 174 400 points at the default batch. Pins the size arithmetic past 2^26 (offsets, counts, batch cuts); the order is the small tests'."""
    gx, gy, gz = 32, 16, 16
    c = np.stack(np.meshgrid(np.arange(gx), np.arange(gy), np.arange(gz), indexing="ij"), -1).reshape(-1, 3)
    sub = np.array([[a, b, d] for a in (0.25, 0.75) for b in (0.25, 0.75) for d in (0.25, 0.75)])
    xyz = (c[:, None, :] + sub[None, :, :]).reshape(-1, 3)
    inten = (np.arange(len(xyz)) % 8).astype(np.float64) * 0.5                                # per cell 0, .5, .. 3.5: mean 1.75
    lattice = np.concatenate([xyz, inten[:, None]], axis=1).astype(f32)
    rng = np.random.default_rng(909)
    lattice = lattice[rng.permutation(len(lattice))]
    assert len(lattice) == 2 ** 16
    tiles = [(i, j) for j in range(32) for i in range(32)] + [(5, 9)]
    km = KeyFrameMap()
    for i, j in tiles:
        km.addKeyFrame(lattice[:1000], lattice[1000:], np.array([0, 0, 0, gx * i, gy * j, 0], f32), 0.0)
    order = rng.permutation(len(tiles))
    total = len(tiles) * 2 ** 16
    assert total > 2 ** 26
    km.setGlobalBatch(0)
    got = km.globalMap(order, 1.0)
    info = km.globalInfo()
    print("past 2^26:", info, "ms", km.globalLastMs())
    assert info["points"] == total and info["form"] == "streamed" and info["batches"] == -(-total // 2 ** 24)
    # expected: every cell of the 1024 x 512 x 16 block, x fastest; centroid = cell + 1/2, intensity 1.75 (16 points in tile (5, 9)'s cells: the same means)
    nx, ny = 32 * gx, 32 * gy
    assert info["cells"] == nx * ny * gz == len(got)
    want = np.empty((gz, ny, nx, 4), f32)
    want[..., 0] = (np.arange(nx) + 0.5)[None, None, :]
    want[..., 1] = (np.arange(ny) + 0.5)[None, :, None]
    want[..., 2] = (np.arange(gz) + 0.5)[:, None, None]
    want[..., 3] = 1.75
    assert same(got, want.reshape(-1, 4))
    km.close()
