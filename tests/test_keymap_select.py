"""CPU: rolo_keyposes_select_nearby (extractNearby, reference src/backMapping.cpp:575-614, with extractCloud's range filter :626) against a numpy twin
written here, which uses the oracle's pcl::VoxelGrid (pyorc.voxelgrid) for the key-pose filter. The entry point is pure host code: no device needed.
FLANN's strict "<" on the radius and its tie order are unpinned, so every case keeps distances away from exactly r."""
import numpy as np
import pytest

from oracle import pyorc
from rolo_amd.backend import select_nearby

f32 = np.float32


def d2_f32(a, b):
    """dx*dx + dy*dy + dz*dz in float, left to right"""
    d = (np.asarray(a, f32) - np.asarray(b, f32)).astype(f32)
    return ((d[..., 0] * d[..., 0]).astype(f32) + (d[..., 1] * d[..., 1]).astype(f32)).astype(f32) + (d[..., 2] * d[..., 2]).astype(f32)


def twin(xyz, times, time_cur, radius, density, recent):
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    n = xyz.shape[0]
    last = xyz[-1]
    d2 = d2_f32(xyz, last)
    hit = np.nonzero(d2 < f32(radius) * f32(radius))[0]
    hit = hit[np.lexsort((hit, d2[hit]))]                      # (distance, index)
    cloud = np.concatenate([xyz[hit], hit.astype(f32)[:, None]], axis=1).astype(f32)
    ds = pyorc.voxelgrid(cloud, density) if len(hit) else np.zeros((0, 4), f32)
    listed = []                                                # (position, key-frame index)
    for p in ds:
        listed.append((p[:3], int(np.argmin(d2_f32(xyz, p[:3])))))   # argmin: the first of equals
    for i in range(n - 1, -1, -1):
        if time_cur - times[i] < recent:
            listed.append((xyz[i], i))
        else:
            break
    out = [k for pos, k in listed if not np.sqrt(d2_f32(pos, last)) > f32(radius)]
    return np.array(out, np.int32)


def trajectory_with_loop(n=400):
    """a rounded rectangle driven once and a bit: the end comes back to within the radius of the start"""
    s = np.linspace(0.0, 1.07, n)
    ang = 2 * np.pi * s
    xyz = np.stack([120.0 * np.cos(ang) + 0.013 * np.arange(n) % 0.7, 60.0 * np.sin(ang), 0.5 * np.sin(3 * ang)], axis=1).astype(f32)
    times = 0.5 * np.arange(n)
    return xyz, times


CASES = {}
_xyz, _t = trajectory_with_loop()
CASES["loop_400"] = (_xyz, _t, _t[-1] + 0.1, 50.0, 2.0, 10.0)
_rng = np.random.default_rng(7)
_spot = (_rng.uniform(-0.25, 0.25, (30, 3)) * np.array([1, 1, 0.1])).astype(f32)
CASES["turning_on_the_spot"] = (_spot, 0.2 * np.arange(30), 0.2 * 29 + 0.05, 50.0, 2.0, 10.0)
CASES["single_pose"] = (np.array([[3.0, -2.0, 0.5]], f32), np.array([12.0]), 12.1, 50.0, 2.0, 10.0)
CASES["no_recent_pose"] = (_xyz[:150], _t[:150], _t[149] + 60.0, 50.0, 2.0, 10.0)
_line = np.stack([7.3 * np.arange(40), np.zeros(40), np.zeros(40)], axis=1).astype(f32)
CASES["radius_excludes_all_but_last"] = (_line, 1.0 * np.arange(40), 39.0 + 20.0, 3.0, 2.0, 10.0)
CASES["radius_excludes_recent_ones"] = (_line, 1.0 * np.arange(40), 39.5, 10.0, 2.0, 10.0)


@pytest.mark.parametrize("name", list(CASES))
def test_select_nearby_matches_the_numpy_twin(name):
    xyz, times, time_cur, radius, density, recent = CASES[name]
    want = twin(xyz, times, time_cur, radius, density, recent)
    got = select_nearby(xyz, times, time_cur, radius, density, recent)
    print(name, "entries", len(got), "distinct", len(set(got.tolist())))
    assert got.dtype == np.int32 and np.array_equal(got, want)
    # what each case is there for
    if name == "loop_400":
        assert (got < 40).any() and (got > 360).any()            # the loop's other end is in the list
    if name == "turning_on_the_spot":
        assert len(got) > len(set(got.tolist()))                 # duplicates, as in the reference
    if name == "single_pose":
        assert got.tolist() == [0, 0]
    if name == "no_recent_pose":
        assert len(got) == len(pyorc.voxelgrid(np.concatenate([xyz, np.zeros((len(xyz), 1), f32)], 1)[d2_f32(xyz, xyz[-1]) < f32(radius) ** 2], density))
    if name == "radius_excludes_all_but_last":
        assert got.tolist() == [39]


def test_empty_and_capacity():
    import ctypes as C
    from rolo_amd._lib import lib
    fp, dp, ip = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert lib().rolo_keyposes_select_nearby(None, None, 0, 50.0, 2.0, 0.0, 10.0, None, 0) == 0
    xyz, times, time_cur, radius, density, recent = CASES["turning_on_the_spot"]
    want = twin(xyz, times, time_cur, radius, density, recent)
    t = np.ascontiguousarray(times, np.float64)
    small = np.full(3, -1, np.int32)
    m = lib().rolo_keyposes_select_nearby(xyz.ctypes.data_as(fp), t.ctypes.data_as(dp), len(xyz), radius, density, time_cur, recent, small.ctypes.data_as(ip), 3)
    assert m == len(want) and np.array_equal(small, want[:3])    # the count is the whole list's, only `cap` entries are written
    assert lib().rolo_keyposes_select_nearby(xyz.ctypes.data_as(fp), t.ctypes.data_as(dp), len(xyz), radius, 0.0, time_cur, recent, small.ctypes.data_as(ip), 3) == -1
