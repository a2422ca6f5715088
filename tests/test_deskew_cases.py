"""CPU: the constructed de-skew clouds of tests/deskew_cases.py through the C++ oracle and the numpy twin — the expectation the device's azimuth and de-skew kernels
are held to in test_gpu_deskew_cases.py, pinned before any GPU sees it. The serial statement on the host libm's atan2f IS the oracle, bit for bit; on the correctly
rounded atan2 it is what the device must compute, and the oracle agrees with it wherever libm is correctly rounded."""
import numpy as np
import pytest

import deskew_cases as dc
from deskew_cases import F, bits
from oracle import pyorc, twin_front as tw


@pytest.fixture(scope="module")
def built():
    return dc.build()


def test_statement_is_the_oracle_bit_for_bit(built):
    """azimuth_statement on the host libm's atan2f against orc_azimuth_times, on every cloud"""
    for c in dc.all_clouds(built):
        to = pyorc.azimuth_times(c.xyz, c.scan_period)
        assert np.array_equal(bits(to), bits(c.libm["times"])), dc.describe(c, to, None)


def test_statement_is_the_twin(built):
    """oracle/twin_front.azimuth_times takes numpy's float32 arctan2 where the oracle takes glibc's atan2f: the statement ON numpy's values is the twin bit for bit —
    the prefix form of the flag against the serial one — and where the two functions lead every point through the same rules the times differ by the ulp of the
    angle that test_oracle_front_golden.py allows (1e-7 s)"""
    other_rules = 0
    for c in dc.all_clouds(built):
        a = np.arctan2(c.xyz[:, 1], c.xyz[:, 0])
        assert a.dtype == F
        st = dc.azimuth_statement(a, c.scan_period)
        tt = tw.azimuth_times(c.xyz, c.scan_period)
        assert np.array_equal(bits(tt), bits(st["times"])), dc.describe(c, tt, None)
        if st["tags"] == c.libm["tags"] and st["end_tag"] == c.libm["end_tag"]:
            assert np.abs(tt - c.libm["times"]).max() <= 1e-7, c.title()
        else:
            other_rules += 1
    print("TWIN: numpy's arctan2 leads a point through another rule than glibc's atan2f in %d of %d clouds" % (other_rules, len(dc.all_clouds(built))))


def test_every_rule_is_taken(built):
    seen = {t: 0 for t in dc.ALL_TAGS}
    for c in dc.all_clouds(built):
        for t in c.exact["tags"] + [c.exact["end_tag"]]:
            seen[t] += 1
    print("RULES taken (points; e*: clouds):", seen)
    assert all(v > 0 for v in seen.values()), seen
    never = [c for c in dc.all_clouds(built) if c.exact["flag"] is None and c.n > 2]
    assert never, "a cloud that never passes half a turn"
    for n, k in dc.SIZES:
        assert any(c.n == n and c.exact["flag"] == k for c in built["sizes"]), (n, k)


def test_planted_pairs(built):
    """the two clouds of a pair differ by one ulp in one coordinate of the planted point, the exact statement puts them on the two sides of the pair's threshold, and
    libm keeps more than half of the pairs of every threshold"""
    for thr, pairs in built["planted"].items():
        assert len(pairs) == dc.STARTS_PER_THRESHOLD
        kept = 0
        for lo, hi in pairs:
            k = lo.planted
            assert k == hi.planted and lo.n == hi.n
            d = np.abs(dc._ordinal(lo.xyz) - dc._ordinal(hi.xyz))
            assert d.sum() == 1 and d[k, :2].sum() == 1, lo.title()
            want = dc.SIDES[thr]
            got = tuple(dc._decision(thr, c.exact, k) for c in (lo, hi))
            assert got == want and (lo.side, hi.side) == want, (lo.title(), got)
            if thr == 5:                                                   # the witnesses: near 0 by the first rule, near one period by the second
                w = slice(k + 1, k + 4)
                assert np.abs(hi.exact["times"][w]).max() < 0.03 and np.abs(lo.exact["times"][w] - hi.exact["times"][w]).min() > 0.07, lo.title()
            kept += lo.kept and hi.kept
        print("PLANTED threshold %d [%s]: %d pairs, the host libm is correctly rounded on both planted points of %d (%.0f %%)"
              % (thr, dc.THRESHOLDS[thr], len(pairs), kept, 100.0 * kept / len(pairs)))
        assert 2 * kept >= len(pairs), thr
        starts = np.array([p[0].start for p in pairs])
        assert np.ptp(starts) > 1.0, "start azimuths spread over the range from which threshold %d can be reached" % thr
    specials = sum(1 for pairs in built["planted"].values() for p in pairs if min(abs(abs(p[0].start) - np.pi), abs(abs(p[0].start) - np.pi / 2), abs(p[0].start)) < 1e-5)
    print("PLANTED pairs whose start azimuth is at, or a few ulps from, +-pi or an axis: %d" % specials)
    assert specials >= 20


def test_oracle_against_the_exact_statement(built):
    """where libm is correctly rounded on the first, the last and the planted point (the kept clouds), the oracle's time is the exact statement's on every point on
    which libm is correctly rounded too"""
    points = same = 0
    for c in dc.all_clouds(built):
        if not c.kept:
            continue
        assert c.libm["end_tag"] == c.exact["end_tag"] and c.libm["flag"] == c.exact["flag"], c.title()
        to = pyorc.azimuth_times(c.xyz, c.scan_period)
        m = c.same_bits
        points += m.size; same += int(m.sum())
        assert np.array_equal(bits(to)[m], bits(c.exact["times"])[m]), dc.describe(c, np.where(m, to, c.exact["times"]), c.libm["flag"])
    print("ORACLE compared with the exact statement on %d of %d points of the kept clouds" % (same, points))


def oracle_deskewed(c, times, rot):
    fo = pyorc.front_params(**c.cfg)
    po = pyorc.project(fo, c.xyz, c.ring, times, pyorc.deskew(list(rot["incre_rpy"]), c.scan_period, rot["odom_time_diff"]))
    o = c.order
    assert po["n"] == len(o) and np.array_equal(po["point_range"], dc.float_range(c.xyz)[o]), c.name
    assert np.array_equal(bits(po["extracted"][:, 3]), bits(c.ring[o].astype(F) * c.xyz[o, 2])), c.name
    return po["extracted"][:, :3]


def test_oracle_rotation_within_the_derived_bound(built):
    """the oracle's de-skewed coordinates against the float64 statement at the oracle's own times, bound at E = 1 (glibc's sinf / cosf); a point at time 0 keeps
    the raw point's bits"""
    worst = 0.0; zeros = 0
    cases = list(built["rotation"])
    for j, rot in enumerate(dc.ROTATIONS):
        for c in dc.all_clouds(built)[j::3] + built["sizes"]:
            cases.append(dc.as_rotation_case(c, rot, pyorc.azimuth_times(c.xyz, c.scan_period)))
    for c in cases:
        rot = dict(incre_rpy=c.incre_rpy, odom_time_diff=c.odom_time_diff)
        got = oracle_deskewed(c, c.times, rot)
        o = c.order
        err = dc.rotation_error(got, c.stated[o], c.xyz[o])
        worst = max(worst, float(err.max()))
        assert (err <= 5 * dc.HOST_TRIG_ULPS + 5).all(), (c.name, float(err.max()))
        z = c.times[o] == 0
        zeros += int(z.sum())
        raw = c.xyz[o][z]
        assert np.array_equal(got[z], raw) and np.array_equal(bits(got[z])[raw != 0], bits(raw)[raw != 0]), c.name
    print("ROTATION oracle: largest error %.2f x 2^-24 L1 (allowed %d) over %d clouds; %d points at time 0 keep the raw bits" % (worst, 5 * dc.HOST_TRIG_ULPS + 5, len(cases), zeros))
    assert zeros >= len(cases)
