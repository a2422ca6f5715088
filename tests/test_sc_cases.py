"""CPU: the constructed Scan Context clouds of tests/sc_cases.py are what they claim — no planted point can hide, every sector and ring edge has both outcomes
among its points under the correctly rounded statement, every guard point lies inside or outside the device's guard as labelled — and sc_twin on the platform
libm is compared with that statement over all of them. What test_gpu_scancontext_cases.py holds the device to is pinned here before any GPU sees it."""
import math

import numpy as np
import pytest

import sc_cases as sc
import sc_twin as T

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def built():
    return sc.build()


def by_cloud(suite):
    out = [[] for _ in suite.clouds]
    for p in suite.points:
        out[p.cloud].append(p)
    return out


def test_placement_no_planted_point_can_hide(built):
    """(d): within a cloud the reserved bins — a point's bin under either outcome — are disjoint, the bin the statement gives is one of the reserved ones, and
    every z' is its own, above NO_POINT and not 0. The statement's descriptor then holds every kept point's z' in its own bin and nothing else."""
    for suite in sc.all_suites(built):
        P = suite.P
        for cloud, members in zip(suite.clouds, by_cloud(suite)):
            assert len(cloud) == len(members) > 0
            seen = set()
            for p in members:
                assert not (p.bins & seen), (suite.name, p.meta)
                seen |= p.bins
            keep, ring, sector = sc.point_bins(cloud, P)
            zp = (cloud[:, 2].astype(f64) + f64(P["lidar_height"])).astype(f32)
            assert len(set(zp.tolist())) == len(zp) and (zp >= 1.0).all()
            desc = T.make_scancontext(cloud, P, sc.atan_cr)
            assert np.count_nonzero(desc) == int(keep.sum())
            for i, p in enumerate(members):
                assert p.index == i and (cloud[i, 0], cloud[i, 1]) == (p.x, p.y)
                if keep[i]:
                    assert (int(ring[i]), int(sector[i])) in p.bins, (suite.name, p.meta)
                    assert desc[ring[i] - 1, sector[i] - 1] == zp[i]
                else:
                    assert p.meta["kind"] == "ring" and p.meta["ring"] == 0 and all(desc[r - 1, s - 1] == 0 for r, s in p.bins)


def test_every_sector_edge_has_both_sectors(built):
    """(a): under the correctly rounded statement the points of edge k fall into sectors k and k + 1, at least two quotient floats on either side, adjacent floats
    across the edge; the four branches occur; the float whose angle is the edge itself is planted for all of the first 14 edges at S = 60"""
    for suite in built["sectors"]:
        P = suite.P; S = P["num_sector"]
        _, _, sector = (np.concatenate(v) for v in zip(*[sc.point_bins(c, P) for c in suite.clouds]))
        order = [p for m in by_cloud(suite) for p in m]
        got = {}
        for p, s in zip(order, sector.tolist()):
            assert s == p.meta["sector"]
            q = f32(abs(p.y)) / f32(abs(p.x))
            assert q == p.meta["q"]                                  # the division is exact: the planted quotient comes back
            got.setdefault(p.meta["edge"], []).append((p.meta["off"], s))
        assert sorted(got) == list(range(1, S))
        for k, v in got.items():
            near = dict(v)
            assert [near[o] for o in range(-2, 4)] in ([k] * 3 + [k + 1] * 3, [k + 1] * 3 + [k] * 3), (suite.name, k, sorted(v))
        assert {p.meta["branch"] for p in suite.points} == {1, 2, 3, 4}
        on_edge = {p.meta["edge"] for p in suite.points if p.meta["on_edge"]}
        print("SECTORS %s: %d points, %d clouds, %d edges with a float angle equal to the edge" % (suite.name, len(suite.points), len(suite.clouds), len(on_edge)))
        if S == 60:
            assert set(range(1, 15)) <= on_edge


def test_every_ring_edge_has_both_rings(built):
    """(c): at every ring edge, on an axis and off it, both rings occur among adjacent floats; at max_radius the largest kept float and the dropped one above it.
    At 25 / 7 and 79.9 / 20 no edge k * max_radius / R is a float, and 79.9 is not a float itself; at 50 / 16 and 70 / 64 the edges are floats and the fp64
    quotient r / max_radius is what rounds"""
    for suite in built["rings"]:
        P = suite.P; R = P["num_ring"]
        inexact = sum(float(f32(k * P["max_radius"] / R)) != k * P["max_radius"] / R for k in range(1, R))
        assert inexact == {(50.0, 16): 0, (25.0, 7): 6, (70.0, 64): 0, (79.9, 20): 19}[(P["max_radius"], R)]   # 3.125 k and 1.09375 k are floats, r / 50 and r / 70 are not exact
        keep, ring, _ = (np.concatenate(v) for v in zip(*[sc.point_bins(c, P) for c in suite.clouds]))
        order = [p for m in by_cloud(suite) for p in m]
        got = {}
        for p, kp, rg in zip(order, keep.tolist(), ring.tolist()):
            assert (rg if kp else 0) == p.meta["ring"]
            got.setdefault((p.meta["edge"], p.meta["on_axis"]), {})[p.meta["off"]] = p.meta["ring"]
            if p.meta["on_axis"]:
                assert p.x == 0 or p.y == 0
            else:
                assert p.x != 0 and p.y != 0
        assert sorted(got) == [(k, ax) for k in range(1, R + 1) for ax in (False, True)]
        for (k, _), v in got.items():
            if k == R:
                assert v == {0: R, 1: 0}
            else:
                assert v == {-1: k, 0: k, 1: k + 1, 2: k + 1}
        print("RINGS %s: %d points, %d clouds" % (suite.name, len(suite.points), len(suite.clouds)))
    assert float(f32(79.9)) > 79.9


def test_guard_points_are_inside_or_outside_as_labelled(built):
    """(b): the closest points and the spread lie inside M -+ 1e-10, of every rim pair one point lies inside and one outside; both float outcomes occur at each
    axis; the zone next to 0 is inside the guard throughout; the closest approach to M equals the recorded one"""
    for suite in built["guard"]:
        S = suite.P["num_sector"]
        for A, br in sc.AXES:
            k = int(A / 360.0 * S)
            pts = [p for p in suite.points if p.meta["axis"] == A and p.meta["M"] is not None]
            for p in pts:
                t = sc.angle64(p.meta["branch"], f32(abs(p.y)) / f32(abs(p.x)))
                assert t == p.meta["t"] and p.meta["inside"] == sc.in_guard(t)
                assert p.meta["inside"] or abs(t - p.meta["M"]) > 0.999 * sc.GUARD
                assert p.meta["sector"] == (k + 1 if t > p.meta["M"] else k)
            assert all(p.meta["inside"] for p in pts if p.meta["role"] in ("closest", "spread"))
            rim = [p.meta["inside"] for p in pts if p.meta["role"] == "rim"]
            assert rim == [False, True, True, False]                # in quotient order: outside, inside ... inside, outside
            assert {p.meta["sector"] for p in pts if p.meta["role"] == "closest"} == {k, k + 1}
            assert sum(p.meta["role"] == "spread" for p in pts) >= 8
        for p in suite.points:                                      # every point of (b), the zones beside 0 and 360 and the far quotients included: as labelled
            assert p.meta["inside"] == sc.in_guard(p.meta["t"]), p.meta
        zero = [p for p in suite.points if p.meta["role"] == "zero"]
        assert len(zero) == 18 and all(p.meta["t"] == sc.angle64(p.meta["branch"], p.meta["q"]) for p in zero)
        assert all(p.meta["inside"] and p.meta["sector"] == 1 for p in zero if p.meta["branch"] == 1)
        assert all(not p.meta["inside"] and p.meta["sector"] == S and 360.0 - 1e-10 < p.meta["t"] <= 360.0 for p in zero if p.meta["branch"] == 4)   # within 1e-10 below 360, whose nearest midpoint is 1.5e-5 away
        assert any(float(p.meta["q"]) == 2.0 ** -149 for p in zero)
        far = [p for p in suite.points if p.meta["role"] == "far"]
        assert sorted(float(p.meta["q"]) for p in far) == [-math.inf, float(f32(3.0) / f32(1e-38)), math.inf]
        assert [p.meta["sector"] for p in far] == [3 * S // 4, 3 * S // 4, S]
        assert [(p.meta["t"], p.meta["inside"]) for p in far] == [(270.0, False), (270.0, False), (450.0, False)]   # floats themselves: outside the guard
        assert far[0].meta["t"] == sc.angle64(4, far[0].meta["q"]) and sc.angle64(4, f32(np.inf)) == 270.0 and sc.angle64(4, f32(-np.inf)) == 450.0
        got = sc.closest_ulps(suite)
        print("GUARD %s: %d points, %d inside the guard; closest approach to M in fp64 ulps of the angle (below, above): %s"
              % (suite.name, len(suite.points), sum(p.meta["inside"] for p in suite.points), got))
        assert got == sc.CLOSEST_ULPS


def test_libm_against_the_correctly_rounded_statement(built):
    """sc_twin on the platform libm against the statement over every planted point: the count of differing atan values and of differing bins is printed (and
    recorded in sc_cases' docstring for the machine it was written on). Nothing is asserted about the count and no point leaves the GPU assertion: the device is
    held to the correctly rounded value whatever the host libm does"""
    for suite in sc.all_suites(built):
        P = suite.P
        n_atan = n_bins = n_guard = 0
        for cloud in suite.clouds:
            with np.errstate(all="ignore"):
                q = np.abs(cloud[:, 1]) / np.abs(cloud[:, 0])
            fin = np.isfinite(q)
            n_atan += int((T._atan(q[fin]) != sc.atan_cr(q[fin])).sum())
            a, b = sc.point_bins(cloud, P, T._atan), sc.point_bins(cloud, P)
            n_bins += int(((a[1] != b[1]) | (a[2] != b[2]) | (a[0] != b[0])).sum())
            x, y = cloud[:, 0], cloud[:, 1]
            for xi, yi, qi in zip(x, y, q):
                br = 1 if xi >= 0 and yi >= 0 else 2 if xi < 0 and yi >= 0 else 3 if xi < 0 else 4
                qq = qi if br != 4 or xi != 0 or not np.signbit(xi) else -qi
                n_guard += qq == qq and sc.in_guard(sc.angle64(br, qq))
        print("LIBM %s: %d points, %d inside the guard, libm atan differs from the correctly rounded on %d, another bin on %d" % (suite.name, len(suite.points), n_guard, n_atan, n_bins))
        assert sum(len(c) for c in suite.clouds) == len(suite.points)


def test_case_module_is_deterministic(built):
    """nothing is drawn at random: a second construction gives the same clouds byte for byte, and the counts are the recorded ones"""
    for kind, geoms in (("sectors", sc.SECTOR_GEOMS), ("guard", [P for P in sc.SECTOR_GEOMS if P["num_sector"] % 4 == 0]), ("rings", sc.RING_GEOMS)):
        assert tuple((len(s.points), len(s.clouds)) for s in built[kind]) == sc.COUNTS[kind]
        assert [s.P for s in built[kind]] == [dict(P) for P in geoms]
    P = sc.SECTOR_GEOMS[2]
    again = sc.Suite("sectors", P, sc.sector_points(P))
    first = built["sectors"][2]
    assert len(again.clouds) == len(first.clouds) and all(a.tobytes() == b.tobytes() for a, b in zip(again.clouds, first.clouds))
    P = sc.RING_GEOMS[1]
    again = sc.Suite("rings", P, sc.ring_points(P))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again.clouds, built["rings"][1].clouds))
    P = sc.SECTOR_GEOMS[1]
    again = sc.Suite("guard", P, sc.guard_points(P))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again.clouds, built["guard"][1].clouds))
