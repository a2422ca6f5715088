"""CPU: the constructed projection clouds of tests/projection_cases.py (planted column edges, axes and signed zeros, range gates, ring values) through the C++ oracle
and the numpy twin — the expectation the device's K1 is held to in test_gpu_projection_cases.py, pinned before any GPU sees it. Everything is exact: columns,
verdicts, pixel owners, n."""
import numpy as np
import pytest

import projection_cases as pc
from oracle import pyorc, twin_front as tw


@pytest.fixture(scope="module")
def built():
    return pc.build()


def oracle_projection(case):
    return pyorc.project(pyorc.front_params(**case.cfg), case.xyz, case.ring)


def check_against_builder(case, proj):
    col, row = pc.read_back(case, proj)
    want = pc.expected_columns(case)
    assert np.array_equal(col, want), pc.describe(case, col, want)
    assert np.array_equal(row[case.owner], case.ring[case.owner].astype(np.int32))
    assert proj["n"] == case.n                                    # with the columns: exactly the accepted first points, nothing else
    o = np.nonzero(case.owner)[0]
    o = o[np.lexsort((case.col[o], case.ring[o]))]                 # the output is row-major
    assert np.array_equal(proj["point_range"], case.range[o])


def test_builder_conditions(built):
    """at least half of the planted points of every H are ones the host libm rounds correctly, in every octant of azimuth; the special edges are there; a third
    point lies more than 256 indices behind the pair point that keeps the pixel; the gates have their exact, stepped and contraction points"""
    for H in pc.EDGE_H:
        e = built["edges"][H]; k = e["kept"]; d = e["dropped"]
        print("EDGES H=%d planted %d kept %d (%.1f %%) dropped %d third points %d; libm atan2f not correctly rounded on %.1f %% of the planted points"
              % (H, e["planted"], e["planted"] - len(d.ring), 100 * e["share"], len(d.ring), e["thirds"], 100 * (1 - e["share"])))
        assert e["no_pair"] == 0 and e["planted"] >= 2 * H // pc.THIN[H]
        assert e["share"] >= 0.5
        assert np.array_equal(np.unique(pc.octant(k)), np.arange(8))
        assert k.same_bits.all() and np.array_equal(k.col, k.col_cr) and k.accept.all()
        assert not d.same_bits.any()
        planted_edges = set(k.meta["edge"].tolist()) | set(d.meta["edge"].tolist())
        assert pc.special_edges(H) <= planted_edges
        pair = ~k.meta["is_third"]
        assert (k.margin[pair] <= 1).mean() > 0.9                  # one ulp of atan2f moves nearly every one of them into the neighbouring column
        # a pair: two floats one ulp apart in one coordinate, in the two columns beside edge e, on ring e % 16
        ed, sd = k.meta["edge"][pair], k.meta["side"][pair]
        assert np.array_equal(k.col[pair], (ed - 1 + sd) % H) and np.array_equal(k.ring[pair], ed % 16)
        third = np.nonzero(k.meta["is_third"])[0]
        assert e["thirds"] == third.size >= H // 40
        for i in third:
            first = np.nonzero(pair & (k.meta["edge"] == k.meta["edge"][i]) & (k.meta["side"] == k.meta["side"][i]))[0]
            assert first.size == 1 and i - first[0] > 256 and k.col[first[0]] == k.col[i] and k.range[first[0]] != k.range[i]
        assert len(k.ring) <= 2 * 4096 + 300
    for H in pc.EDGE_H:
        a = built["axes"][H]
        assert np.array_equal(a.col, a.col_cr) and a.accept.all() and a.owner.all()
        # +pi and -pi are one column: (+0, -r) and (-0, -r), the denormals beside them, and atan2f(+-0, -0)
        assert set(a.col[[1, 2, 8, 9, 14, 15]].tolist()) == {H // 4} and set(a.col[-5:].tolist()) == {3 * H // 4, H // 4}
        assert a.col[4] == H // 2 and a.col[5] == 0 and a.col[0] == 3 * H // 4
    for g in built["gates"]:
        assert np.array_equal(g.col[g.accept], g.col_cr[g.accept])
        kind = g.meta["kind"]
        lo, hi = pc.F(g.cfg["lidar_min_range"]), pc.F(g.cfg["lidar_max_range"])
        at_gate = kind == 0
        assert at_gate.sum() >= 12 and g.accept[at_gate].all() and np.all((g.range[at_gate] == lo) | (g.range[at_gate] == hi))
        stepped = np.nonzero(kind == 1)[0]; half = stepped.size // 2
        assert half == 12 and np.all(g.accept[stepped[:half]] != g.accept[stepped[half:]])
        assert (kind == 2).sum() >= 2                               # the points that notice a contracted x*x + y*y + z*z, at either gate
    r1, r3 = built["rings"]
    assert set(r1.ring[r1.accept].tolist()) == set(range(16)) and set(r3.ring[r3.accept].tolist()) == {0, 3, 6, 9, 12, 15}
    assert {16, 17, 32768, 65520, 65535} <= set(r1.ring[~r1.accept].tolist())


def test_oracle_gives_the_builders_columns(built):
    """pyorc.project on every built cloud: the builder's column for every point (read through point_col_ind, the points found by their coordinates in `extracted`),
    its accept / reject verdicts and n"""
    for case in pc.all_cases(built):
        check_against_builder(case, oracle_projection(case))


def test_contraction_points_see_a_contracted_sum(built):
    """the gate points of kind 2 change their verdict when the sum of squares is evaluated with fused multiply-adds: they are what notices front.hip (or the
    oracle) being compiled without -ffp-contract=off"""
    for g in built["gates"]:
        lo, hi = pc.F(g.cfg["lidar_min_range"]), pc.F(g.cfg["lidar_max_range"])
        for i in np.nonzero(g.meta["kind"] == 2)[0]:
            plain, f1, f2 = pc._sum_sq_forms(*g.xyz[i])
            ok = [not (np.sqrt(s) < lo or np.sqrt(s) > hi) for s in (plain, f1, f2)]
            assert ok[0] == bool(g.accept[i]) and ok[1] != ok[0] and ok[2] != ok[0]


def test_dropped_points_are_reported(built):
    """the planted points where the host libm's atan2f is not the correctly rounded value: through the oracle for the record. Nothing to assert about their columns —
    the two statements differ on them by construction — beyond that the oracle follows ITS libm on them too."""
    for H in pc.EDGE_H:
        d = built["edges"][H]["dropped"]
        col, _ = pc.read_back(d, oracle_projection(d))
        assert np.array_equal(col, pc.expected_columns(d))
        print("DROPPED H=%d: %d points, the correctly rounded atan2f gives another column than the host libm's on %d" % (H, len(d.ring), int((d.col != d.col_cr).sum())))


def test_twin_agrees_on_axes_gates_and_rings(built):
    """oracle/twin_front.py's projection on the axes, gates and rings clouds. Its float32 numpy arctan2 is numpy's own kernel, not glibc's atan2f, so it is NOT asserted on
    the planted edges (an ulp there is a column); on these clouds every point is far from an edge of its column."""
    for case in [built["axes"][H] for H in pc.EDGE_H] + built["gates"] + built["rings"]:
        assert (case.margin[case.accept] > 4).all()
        c = case.cfg
        pt = tw.project(case.xyz, case.ring, c["n_scan"], c["horizon_scan"], c.get("downsample_rate", 1), c.get("lidar_min_range", pc.DEFAULT_GATES[0]),
                        c.get("lidar_max_range", pc.DEFAULT_GATES[1]))
        po = oracle_projection(case)
        assert pt["n"] == po["n"] == case.n
        assert np.array_equal(np.sort(pt["owner"]), np.nonzero(case.owner)[0])
        for k in ("extracted", "point_col_ind", "point_range", "start_ring", "end_ring"):
            assert np.array_equal(pt[k], po[k]), (case.name, k)
