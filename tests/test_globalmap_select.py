"""CPU: KeyFrameMap.selectGlobal's rule (backend.select_global; publishGlobalMap's selection, reference src/backMapping.cpp:1619-1654) against a numpy twin
written here: tests/test_keymap_select.py::twin without its time clause, with the oracle's pcl::VoxelGrid (pyorc.voxelgrid) for the key-pose filter. Pure host
code: no device needed. FLANN's strict "<" on the radius and its tie order are unpinned, so every case keeps distances away from exactly r, and
the test checks that it does."""
import numpy as np
import pytest

from oracle import pyorc
from rolo_amd.backend import select_global, select_nearby

f32 = np.float32


def d2_f32(a, b):
    """dx*dx + dy*dy + dz*dz in float, left to right"""
    d = (np.asarray(a, f32) - np.asarray(b, f32)).astype(f32)
    return ((d[..., 0] * d[..., 0]).astype(f32) + (d[..., 1] * d[..., 1]).astype(f32)).astype(f32) + (d[..., 2] * d[..., 2]).astype(f32)


def twin(xyz, radius, density):
    """-> (indices, smallest |distance - r| over every distance the rule compares with r)"""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    last = xyz[-1]
    d2 = d2_f32(xyz, last)
    hit = np.nonzero(d2 < f32(radius) * f32(radius))[0]
    hit = hit[np.lexsort((hit, d2[hit]))]                      # (distance, index)
    cloud = np.concatenate([xyz[hit], hit.astype(f32)[:, None]], axis=1).astype(f32)
    ds = pyorc.voxelgrid(cloud, density) if len(hit) else np.zeros((0, 4), f32)
    listed = [(p[:3], int(np.argmin(d2_f32(xyz, p[:3])))) for p in ds]   # argmin: the first of equals
    out = [k for pos, k in listed if not np.sqrt(d2_f32(pos, last)) > f32(radius)]
    dist = np.concatenate([np.sqrt(d2.astype(np.float64)), [np.sqrt(float(d2_f32(pos, last))) for pos, _ in listed]])
    return np.array(out, np.int32), float(np.abs(dist - radius).min())


def trajectory_with_loop(n=400):
    """tests/test_keymap_select.py's rounded rectangle driven once and a bit: the end comes back to the start"""
    s = np.linspace(0.0, 1.07, n)
    ang = 2 * np.pi * s
    return np.stack([120.0 * np.cos(ang) + 0.013 * np.arange(n) % 0.7, 60.0 * np.sin(ang), 0.5 * np.sin(3 * ang)], axis=1).astype(f32)


_loop = trajectory_with_loop()
_rng = np.random.default_rng(17)
_spot = (_rng.uniform(-0.25, 0.25, (30, 3)) * np.array([1, 1, 0.1])).astype(f32)
CASES = {
    "loop_400_defaults": (_loop, None, None),                   # globalMapVisualizationSearchRadius 1000, ...PoseDensity 10: the whole loop
    "loop_400_r1000_d10": (_loop, 1000.0, 10.0),
    "loop_400_radius_clips": (_loop, 90.0, 10.0),               # the far side of the loop is out
    "loop_400_dense_filter": (_loop, 1000.0, 1.5),
    "single_pose": (np.array([[3.0, -2.0, 0.5]], f32), 1000.0, 10.0),
    "duplicates_among_filtered_poses": (_spot, 1000.0, 0.2),    # cells' centroids whose nearest key pose is the same one
}


@pytest.mark.parametrize("name", list(CASES))
def test_select_global_matches_the_numpy_twin(name):
    xyz, radius, density = CASES[name]
    got = select_global(xyz) if radius is None else select_global(xyz, radius, density)
    radius, density = (1000.0, 10.0) if radius is None else (radius, density)
    want, margin = twin(xyz, radius, density)
    print(name, "entries", len(got), "distinct", len(set(got.tolist())), "margin to r", margin)
    assert margin > 1e-3                                           # no compared distance sits at the radius
    assert got.dtype == np.int32 and np.array_equal(got, want)
    # what each case is there for
    if name.startswith("loop_400_r1000") or name == "loop_400_defaults":
        assert got.min() < 40 and got.max() > 360 and 150 < np.median(got) < 250 and len(got) < 400   # all round the loop, thinned
    if name == "loop_400_radius_clips":
        assert len(got) and not ((got > 120) & (got < 260)).any()
    if name == "single_pose":
        assert got.tolist() == [0]
    if name == "duplicates_among_filtered_poses":
        assert len(got) > len(set(got.tolist()))


def test_nothing_is_admitted_by_time():
    """select_nearby's recent clause lists the newest poses whatever the filter did; the global selection is exactly its list without them"""
    times = 0.5 * np.arange(len(_loop))
    with_recent = select_nearby(_loop, times, times[-1] + 0.1, 1000.0, 10.0, 10.0)
    got = select_global(_loop, 1000.0, 10.0)
    assert len(with_recent) > len(got) and np.array_equal(with_recent[:len(got)], got)
    assert select_global(np.zeros((0, 3), f32)).tolist() == []
