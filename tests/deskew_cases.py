"""Constructed raw clouds for the de-skew step of the front end (azimuth_flag_kernel, azimuth_time_kernel, deskew_point in ring_scatter_kernel: rolo_amd/csrc/front.hip;
oracle/rolo_oracle_front.cpp:27-63), with the expected time, rule and de-skewed coordinates of every point. CPU only: numpy, mpmath and the host libm (through
tests/projection_cases.py); neither rolo_amd nor HIP is imported.

The times of a cloud without a time field are interpolated from the azimuth (deskewCloudInfo, timeFlag == -1, imageProjection.cpp:270-327) by a rule that makes seven
comparisons of a float angle against a threshold. azimuth_statement() is that rule, serially, on the float atan2 values it is GIVEN:

  the float statement   on atan2f of the host libm — the C++ oracle's orc_azimuth_times, bit for bit;
  the exact statement   on the correctly rounded float atan2 (projection_cases.atan2_exact) — what the device computes, and the only value two machines agree on.

Besides the times it returns the index of the point that set halfPassed (None: no point did) and per point the rule it took:
  end rule     e0 (end kept), e- (end - start > 3 pi: 2 pi subtracted), e+ (end - start < pi: 2 pi added);
  first half   a0 / a+ / a- (no adjustment, + 2 pi, - 2 pi), with a trailing * on the point that set the flag;
  second half  b0 / b+ / b- (after the unconditional + 2 pi: nothing more, + 2 pi, - 2 pi).
a- never sets the flag: the rule applies to ori > start + 3 pi / 2, and ori <= pi, so the adjusted angle ori - 2 pi is <= -pi <= start: angle - start <= 0, never > pi.

deskew_statement() is deskewPoint (:368-396, rotation only): ratio, s1 and the three angles in float32 exactly where the reference rounds (front.hip, deskew_point:
exact float operations, the same on every machine), the sines, cosines, the nine entries and the three sums in float64.

The bound on the rotation (rotation_bound), in units of u = 2^-24, the spacing of the floats below 1. Let the float sinf / cosf be within E ulps: each of A .. F
(|.| <= 1) is within E u of the float64 value. The worst entry is A * DF - B * E with DF = fl(D * F): five trig values enter it, each with cofactors <= 1, so their
errors add up to at most 5 E u to first order; DF, A * DF, B * E and the difference round once each, values below 1, half a spacing each: two more u. The entry is
within (5 E + 2) u, the other entries closer, so the three entries of a row put the sum off by at most (5 E + 2) u (|x| + |y| + |z|) = (5 E + 2) u L1. The row's three
products round to within u of themselves, together u L1 at most (the entries are <= 1); its two real additions (the third adds 0.f) to within u of a partial sum
<= L1 each. So a float result differs from the float64 statement by at most (5 E + 5) 2^-24 L1 per coordinate. E = 1 for the host libm (glibc documents sinf / cosf
at 1 ulp); for the device E = 2: the 1 ulp that HIP's math API reference lists — a largest OBSERVED error — plus one, as front.hip takes it for atan2f (COLUMN_GUARD_DEG).

Clouds. Tens of points each (1 025 at most), ranges 3 .. 60 m, z small and never zero (the gates at 2 m and 1000 m are never in play), H = 1800 and every point on a
pixel of its own with two free columns on either side (own_pixels), so the stored coordinates of every point can be read: the output is the points in (ring, column)
order. For EVERY point the exact angle (mpmath, 256 bits) lies at least 2^-20 of a float ulp from the midpoint of two floats — a point that does not is re-drawn — so
that a double-precision atan2 rounded to float is the correctly rounded float. The first and the last point of a cloud, whose angles move every time of the cloud,
are re-drawn until the host libm is correctly rounded on them (unless they are the planted point), and every point that is not planted keeps its rule when its
angle moves by three ulps: the oracle can then be compared point by point wherever libm is correctly rounded on the point itself.

  planted    for each of the seven thresholds (THRESHOLDS) and about 40 start azimuths over (-pi, pi] where the threshold can be reached — among them starts at, and a
             few ulps from, +-pi (the negative x axis with y = +0 / -0) and the axes — a PAIR of clouds that differ in one coordinate of one point by one ulp, which
             the exact statement puts on either side. 1, 2: end - start against 3 pi / pi, planted on the last point; 3, 4: ori against start - pi / 2 /
             start + 3 pi / 2, planted at index 1; 5: the flip, adjusted ori - start against pi, followed by witnesses within +-pi / 2 of the start (the first rule
             leaves them near 0, the second near one period); 6, 7: ori + 2 pi against end - 3 pi / 2 / end + pi / 2, planted behind a point that set the flag.
             A cloud is KEPT where libm is correctly rounded on its planted point; a pair where both clouds are. Two adjacent coordinates with different
             angle floats have the midpoint of those floats between their exact angles, so they are hard cases for any atan2f: libm loses many of them, by
             bands of the angle. A random start is therefore drawn up to four times, with the rest of its cloud, for a pair that libm keeps (the device is
             held to the exact statement on every pair, kept or not). A special start whose threshold falls where the coordinates resolve the angle 2^20 times
             finer than the float does (a threshold on an axis) has no pair that meets the midpoint condition and is given up for that threshold.
  orders     one clockwise sweep, the same reversed, ring-major (four sweeps one after another), a random permutation, less than half a turn clockwise (the flag
             is never set) and anticlockwise (it is: + 2 pi takes every point past it), 1.02 turns, the first / last point on the negative x axis with y = +0 / -0, points with x = y = +-0.
  sizes      n = 1, 2, 255, 256, 257, 1025 with the flipping point at index 1, 255, 256, n - 1 or nowhere; further candidates (points that the first rule would let
             flip) behind it in every block, or the only candidate in the last block.
  rotation   three increment sets — (0.7, -0.9, 2.5), (0.004, -0.006, 0.035) and (3.0, 1.5, -3.1) rad, the last with odom_time_diff = -0.05 so that s1 is negative and
             the arguments of sinf / cosf reach 8 rad — with handed-over times 0, denormals, up to 1.3 periods and a ramp.

build() makes everything once per process."""
import math

import mpmath as mp
import numpy as np

from projection_cases import F, _adjacent_flip, _from_ordinal, _ordinal, atan2_exact, atan2f, bits, column_of_angle, flip_margin, float_range  # noqa: F401

PI = math.pi
TWO_PI = 2 * math.pi
H = 1800
SEED = 20261020
SCAN_PERIOD = 0.1
INT_MAX = 2 ** 31 - 1
THRESHOLDS = {1: "end - start > 3 pi (last point)", 2: "end - start < pi (last point)", 3: "ori < start - pi / 2", 4: "ori > start + 3 pi / 2",
              5: "the flip: adjusted ori - start > pi", 6: "ori + 2 pi < end - 3 pi / 2", 7: "ori + 2 pi > end + pi / 2"}
SIDES = {1: ("e-", "e0"), 2: ("e+", "e0"), 3: ("a+*", "a0"), 4: ("a-", "a0*"), 5: ("flips", "stays"), 6: ("b+", "b0"), 7: ("b-", "b0")}
ALL_TAGS = ("e0", "e-", "e+", "a0", "a+", "a-", "a0*", "a+*", "b0", "b+", "b-")
STARTS_PER_THRESHOLD = 40
START_RANGE = {1: (-PI, 0.0), 2: (0.0, PI), 3: (-PI / 2, PI), 4: (-PI, -PI / 2)}   # where a threshold can be reached at all (thresholds 5 - 7: everywhere)
DEVICE_TRIG_ULPS = 2         # HIP's math API reference lists sinf / cosf at 1 ulp (observed); plus one
HOST_TRIG_ULPS = 1


# ---- the serial statement of deskewCloudInfo's timeFlag == -1 branch -----------------------------------------------------------------------
def azimuth_statement(ang, scan_period=SCAN_PERIOD):
    """ang[i] = the float atan2(y, x) of raw point i -> dict(times float32, flag int or None, tags [str], end_tag, start, end). Float and double steps as the
    reference's C++ takes them: a float compared with or added to a double expression is widened, a sum stored into a float is rounded once."""
    ang = np.asarray(ang, F).reshape(-1)
    n = ang.size
    neg = -ang
    start = neg[0]                                                                                      # :272
    end = F(float(neg[n - 1]) + TWO_PI)                                                                  # :273
    if float(F(end - start)) > 3 * PI:                                                                   # :274-277
        end = F(float(end) - TWO_PI); end_tag = "e-"
    elif float(F(end - start)) < PI:
        end = F(float(end) + TWO_PI); end_tag = "e+"
    else:
        end_tag = "e0"
    diff = F(end - start)
    sp = F(scan_period)
    s64, e64 = float(start), float(end)
    times = np.empty(n, F); tags = []; flag = None
    for i in range(n):
        ori = neg[i]                                                                                     # :307
        if flag is None:
            if float(ori) < s64 - PI / 2:
                ori = F(float(ori) + TWO_PI); t = "a+"
            elif float(ori) > s64 + PI * 3 / 2:
                ori = F(float(ori) - TWO_PI); t = "a-"
            else:
                t = "a0"
            if float(F(ori - start)) > PI:
                flag = i; t += "*"
        else:                                                                                            # :316-322
            ori = F(float(ori) + TWO_PI)
            if float(ori) < e64 - PI * 3 / 2:
                ori = F(float(ori) + TWO_PI); t = "b+"
            elif float(ori) > e64 + PI / 2:
                ori = F(float(ori) - TWO_PI); t = "b-"
            else:
                t = "b0"
        times[i] = sp * F(F(ori - start) / diff)                                                         # :324-325
        tags.append(t)
    return dict(times=times, flag=flag, tags=tags, end_tag=end_tag, start=start, end=end)


def azimuth_times(xyz, scan_period=SCAN_PERIOD, atan2=atan2f):
    """the statement on a cloud; atan2(a, b) -> float32 array is the float atan2: the host libm's by default, cr_angles for the correctly rounded one"""
    xyz = np.asarray(xyz, F)
    return azimuth_statement(atan2(xyz[:, 1], xyz[:, 0]), scan_period)


# ---- the float64 statement of deskewPoint ---------------------------------------------------------------------------------------------
def deskew_statement(xyz, times, incre_rpy, scan_period=SCAN_PERIOD, odom_time_diff=0.1):
    """-> (n, 3) float64"""
    xyz = np.asarray(xyz, F); t = np.asarray(times, F)
    sp = F(scan_period)
    ratio = (t.astype(np.float64) / np.float64(sp)).astype(F)                                             # :380 double / float, stored float
    s1 = F(np.float64(sp) / np.float64(odom_time_diff))                                                    # :383
    roll, pitch, yaw = (-((F(incre_rpy[k]) * s1) * ratio).astype(F).astype(np.float64) for k in range(3))   # float products, rounded one by one
    A, B, C, D, E, Fs = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    x, y, z = (xyz[:, k].astype(np.float64) for k in range(3))
    return np.stack([(A * C) * x + (A * D * Fs - B * E) * y + (B * Fs + A * D * E) * z,
                     (B * C) * x + (A * E + B * D * Fs) * y + (B * D * E - A * Fs) * z,
                     (-D) * x + (C * Fs) * y + (C * E) * z], 1)


def l1(xyz):
    return np.abs(np.asarray(xyz, F).astype(np.float64)).sum(1)


def rotation_bound(xyz, trig_ulps):
    """the largest |float result - float64 statement| per coordinate (module docstring): (5 E + 5) 2^-24 (|x| + |y| + |z|), one value per point"""
    return (5 * trig_ulps + 5) * 2.0 ** -24 * l1(xyz)


def rotation_error(stored, stated, xyz):
    """-> per point the largest coordinate error as a multiple of 2^-24 L1"""
    return np.abs(np.asarray(stored, np.float64) - stated).max(1) / (2.0 ** -24 * l1(xyz))


# ---- exact angles -------------------------------------------------------------------------------------------------------------------------
class Redraw(Exception):
    """a drawn cloud misses one of the generator's own conditions: draw again"""


_EXACT = {}


def _cr_angle(y, x):
    """the correctly rounded float atan2(y, x) and whether the exact value keeps 2^-20 ulp from the midpoints beside it (cached by the bits of the arguments)"""
    key = (float(y).hex(), float(x).hex())
    if key not in _EXACT:
        c, v = atan2_exact(y, x)
        ok = True
        if v is not None:
            with mp.workprec(256):
                lo, hi = np.nextafter(c, F(-np.inf)), np.nextafter(c, F(np.inf))
                ulp = mp.mpf(float(hi)) - mp.mpf(float(c))
                d = min(abs(v - (mp.mpf(float(c)) + mp.mpf(float(lo))) / 2), abs(v - (mp.mpf(float(c)) + mp.mpf(float(hi))) / 2))
                ok = bool(d >= ulp * mp.mpf(2) ** -20)
        _EXACT[key] = (F(c), ok)
    return _EXACT[key]


def cr_angles(a, b, margin=None):
    """the correctly rounded float atan2(a, b), element by element; margin: a list that receives the midpoint verdict of every element"""
    out = np.empty(len(a), F)
    for i, (p, q) in enumerate(zip(np.asarray(a, F).tolist(), np.asarray(b, F).tolist())):
        out[i], ok = _cr_angle(p, q)
        if margin is not None:
            margin.append(ok)
    return out


def fast_angles(xyz):
    """float(atan2 in double) of (y, x): the generator's working value, confirmed against cr_angles once a cloud is drawn"""
    xyz = np.asarray(xyz, F)
    return np.arctan2(xyz[:, 1].astype(np.float64), xyz[:, 0].astype(np.float64)).astype(F)


def shifted(ang, k, skip):
    """every angle moved by k float ulps, except the indices in skip"""
    o = _ordinal(ang) + k
    o[list(skip)] = _ordinal(ang)[list(skip)]
    return _from_ordinal(o)


# ---- pixels ---------------------------------------------------------------------------------------------------------------------------
def own_pixels(xyz):
    """-> (ring, column) per point: the k-th point that comes within two columns of an earlier one goes on the next free ring. The column is K1's (the expression
    on the correctly rounded atan2f(x, y)); a point within two ulps of a column edge is refused (Redraw), so that any atan2f gives this column."""
    xyz = np.asarray(xyz, F)
    a = np.arctan2(xyz[:, 0].astype(np.float64), xyz[:, 1].astype(np.float64)).astype(F)
    col = column_of_angle(a, H)
    if (col < 0).any() or (flip_margin(a, H, most=2) <= 2).any():
        raise Redraw("a point at a column edge")
    taken = []
    ring = np.zeros(len(col), np.uint16)
    for i, c in enumerate(col.tolist()):
        near = {(c + d) % H for d in (-2, -1, 0, 1, 2)}
        r = 0
        while r < len(taken) and taken[r] & near:
            r += 1
        if r == len(taken):
            taken.append(set())
        taken[r].add(c); ring[i] = r
    if len(taken) > 128:
        raise Redraw("more than 128 rings")
    return ring, col.astype(np.int32)


# ---- a cloud --------------------------------------------------------------------------------------------------------------------------
class Cloud:
    """xyz (n, 3) float32 and ring uint16 of a raw cloud, cfg = the keyword arguments of front_params; ang_cr / ang_libm: the two float atan2(y, x) of every point,
    same_bits where they agree; exact / libm: azimuth_statement on either; col: K1's column of every point, order: the raw indices in output order; thr / side /
    pair / planted: the threshold, the side the exact statement takes, the number of the pair within the threshold and the index of the planted point (0 / "" / -1 /
    -1 for a cloud without one); kept: libm is correctly rounded on the first, the last and the planted point."""

    def __init__(self, name, xyz, thr=0, side="", pair=-1, planted=-1, scan_period=SCAN_PERIOD):
        self.name = name; self.xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
        self.thr, self.side, self.pair, self.planted, self.scan_period = thr, side, pair, planted, scan_period
        n = len(self.xyz)
        rg = float_range(self.xyz)
        assert (rg >= 3).all() and (rg <= 60.5).all() and (self.xyz[:, 2] != 0).all(), name
        self.ring, self.col = own_pixels(self.xyz)
        margin = []
        self.ang_cr = cr_angles(self.xyz[:, 1], self.xyz[:, 0], margin)
        if not all(margin):
            raise Redraw("an angle too close to the midpoint of two floats")
        assert np.array_equal(bits(self.ang_cr), bits(fast_angles(self.xyz))), name + ": a double atan2 rounded to float is the correctly rounded float"
        self.ang_libm = atan2f(self.xyz[:, 1], self.xyz[:, 0])
        self.same_bits = bits(self.ang_cr) == bits(self.ang_libm)
        ends = [i for i in (0, n - 1) if i != planted]
        if not self.same_bits[ends].all():
            raise Redraw("libm is not correctly rounded on the first / last point")
        self.kept = bool(planted < 0 or self.same_bits[planted])
        self.exact = azimuth_statement(self.ang_cr, scan_period)
        self.libm = azimuth_statement(self.ang_libm, scan_period)
        skip = set(ends) | ({planted} if planted >= 0 else set())
        for k in (3, -3):
            s = azimuth_statement(shifted(self.ang_cr, k, skip), scan_period)
            if s["tags"] != self.exact["tags"] or s["end_tag"] != self.exact["end_tag"]:
                raise Redraw("a point that is not planted within three ulps of a threshold")
        self.cfg = dict(n_scan=16 if int(self.ring.max()) < 16 else 128, horizon_scan=H)
        self.order = np.lexsort((self.col, self.ring))
        self.start = float(self.exact["start"])

    @property
    def n(self):
        return len(self.xyz)

    @property
    def flag(self):
        return INT_MAX if self.exact["flag"] is None else self.exact["flag"]

    def title(self):
        if not self.thr:
            return "%s (start azimuth %r)" % (self.name, self.start)
        return "%s: threshold %d [%s], side %s, start azimuth %r (%s), planted point #%d" % (
            self.name, self.thr, THRESHOLDS[self.thr], self.side, self.start, float(self.start).hex(), self.planted)


def describe(cloud, dev_times, dev_flag, most=8):
    """the points whose time differs from the exact statement's, for an assertion message"""
    ex = cloud.exact
    bad = np.nonzero(bits(dev_times) != bits(ex["times"]))[0]
    lines = ["%s: %d of %d times differ; flag index %s, expected %s; end rule %s" % (cloud.title(), bad.size, cloud.n, dev_flag, cloud.flag, ex["end_tag"])]
    for i in bad[:most]:
        lines.append("  #%d x=%r (%s) y=%r (%s): time %r, expected %r by rule %s; correctly rounded atan2f %r (libm %r)"
                     % (i, float(cloud.xyz[i, 0]), float(cloud.xyz[i, 0]).hex(), float(cloud.xyz[i, 1]), float(cloud.xyz[i, 1]).hex(), float(dev_times[i]),
                        float(ex["times"][i]), ex["tags"][i], float(cloud.ang_cr[i]), float(cloud.ang_libm[i])))
    return "\n".join(lines)


# ---- drawing points -------------------------------------------------------------------------------------------------------------------
def wrap(o):
    """an angle into (-pi, pi]"""
    return o - TWO_PI * math.ceil((o - PI) / TWO_PI)


def point(ori, rng, r=None):
    """a point whose azimuth -atan2(y, x) is ori (up to the rounding of its coordinates), range 3 .. 60, a small z"""
    r = rng.uniform(3.0, 58.0) if r is None else r
    return np.array([r * math.cos(ori), -r * math.sin(ori), r * rng.uniform(0.01, 0.05) * rng.choice([-1.0, 1.0])], F)


def anchor(ori, rng):
    """a point at azimuth ori on which the host libm's atan2f is correctly rounded: a first or a last point"""
    for _ in range(200):
        p = point(ori + rng.uniform(-1e-4, 1e-4), rng)
        if bits(atan2f(p[1:2], p[0:1]))[0] == bits(fast_angles(p[None]))[0]:
            return p
    raise Redraw("no anchor")


def special_starts(rng):
    """first points at, and a few ulps from, the negative x axis (start = -+pi) and the axes"""
    out = []
    r = 7.25
    for ysign in (0.0, -0.0):
        out.append((-r, ysign)); out.append((r, ysign))                       # start = -+pi, -+0
    for xsign in (0.0, -0.0):
        out.append((xsign, r)); out.append((xsign, -r))                       # start = -+pi / 2
    for k in (1, 3):
        for sg in (1.0, -1.0):
            out.append((-r, sg * r * k * 2.0 ** -22))                         # k ulps of pi from the negative x axis
            out.append((sg * r * k * 2.0 ** -23, r)); out.append((sg * r * k * 2.0 ** -23, -r))   # ... of pi / 2 from the y axis
            out.append((r, sg * r * 2.0 ** -100 * k))                         # beside the positive x axis: a tiny angle
    pts = [np.array([x, y, 0.3 * (1 + 0.1 * i)], F) for i, (x, y) in enumerate(out)]
    return [p for p in pts if bits(atan2f(p[1:2], p[0:1]))[0] == bits(fast_angles(p[None]))[0]]


def ori_of(p):
    return -float(fast_angles(np.asarray(p, F)[None])[0])


# ---- planted pairs ------------------------------------------------------------------------------------------------------------------------
def _decision(thr, st, k):
    if thr in (1, 2):
        return st["end_tag"]
    if thr == 5:
        return "flips" if st["flag"] == k else "stays"
    return st["tags"][k]


def _target(thr, s, end):
    """the raw azimuth (before any adjustment) at which threshold thr lies, or None where it cannot be reached with a margin from the branch cut at +-pi"""
    if thr in (6, 7):
        t = end - 3 * PI / 2 - TWO_PI if thr == 6 else end + PI / 2 - TWO_PI
    else:
        t = {1: s + PI, 2: s - PI, 3: s - PI / 2, 4: s + 3 * PI / 2, 5: wrap(s + PI)}[thr]
    return t if -PI + 0.12 < t < PI - 0.12 else None


def _layout(thr, first, rng):
    """-> (points, index of the planted point) with the planted point exactly at its threshold in double; Redraw where thr cannot be reached from this start"""
    s = ori_of(first)
    first_half = lambda: point(wrap(s + rng.uniform(-1.2, 2.8)), rng)          # noqa: E731 — the first rule leaves it alone or adjusts it; it never flips
    flipper = lambda: point(wrap(s + PI + rng.uniform(0.25, 1.2)), rng)        # noqa: E731
    witness = lambda: point(wrap(s + rng.uniform(-1.3, 1.3)), rng)             # noqa: E731
    anyp = lambda: point(rng.uniform(-PI, PI), rng)                            # noqa: E731
    if thr in (1, 2):
        t = _target(thr, s, None)
        if t is None:
            raise Redraw("unreachable")
        pts = [first, first_half(), first_half(), flipper(), anyp(), anyp(), witness(), point(t, rng)]
        return pts, len(pts) - 1
    # the last point: a little less than a full turn, a little more, or far from it — whatever lets the second-half thresholds be reached
    # (the flip's witnesses tell the two rules apart only where the turn is about full)
    for delta in rng.permutation([-0.2, 0.13] if thr == 5 else [-0.2, 0.13, -2.0, 2.0, -0.9, 0.9]):
        last = anchor(wrap(s + delta), rng)
        end = float(azimuth_statement(fast_angles(np.stack([first, last])))["end"])
        t = _target(thr, s, end)
        if t is not None:
            break
    else:
        raise Redraw("unreachable")
    if thr in (3, 4):
        pts = [first, point(t, rng), first_half(), anyp(), witness(), anyp(), anyp(), last]
        return pts, 1
    if thr == 5:
        pts = [first, first_half(), first_half(), point(t, rng), witness(), witness(), witness(), anyp(), last]
        return pts, 3
    pts = [first, first_half(), flipper(), anyp(), point(t, rng), witness(), anyp(), last]
    return pts, 4


def plant(thr, first, pair, rng):
    """-> the two clouds of a pair (side order of SIDES[thr])"""
    pts, k = _layout(thr, first, rng)
    xyz = np.stack(pts).astype(F)
    step_x = abs(xyz[k, 0]) <= abs(xyz[k, 1])                                  # step the smaller coordinate: the finer one in angle
    c = 0 if step_x else 1
    base = fast_angles(xyz)

    def variant(o):
        v = xyz.copy(); v[k, c] = _from_ordinal(np.array([o]))[0]
        return v

    def verdict(o):
        out = []
        for oo in np.asarray(o).tolist():
            a = base.copy(); a[k] = fast_angles(variant(oo)[k:k + 1])[0]
            d = _decision(thr, azimuth_statement(a), k)
            out.append(SIDES[thr].index(d) if d in SIDES[thr] else 2)
        return np.array(out, np.int64)

    a, b, found = _adjacent_flip(np.array([_ordinal(xyz[k, c])]), verdict, reach=1 << 30)
    if not found[0] or sorted((int(verdict(a)[0]), int(verdict(b)[0]))) != [0, 1]:
        raise Redraw("no adjacent pair on the two sides")
    o = (a[0], b[0]) if verdict(a)[0] == 0 else (b[0], a[0])
    out = []
    for side, oo in zip(SIDES[thr], o):
        cl = Cloud("planted/%d/%d/%s" % (thr, pair, side), variant(oo), thr, side, pair, k)
        if _decision(thr, cl.exact, k) != side:
            raise Redraw("the exact statement disagrees with the working angle")
        out.append(cl)
    return out


def planted_clouds(seed=SEED):
    """-> {thr: [(cloud of side 0, cloud of side 1), ...]}"""
    out = {}
    for thr in THRESHOLDS:
        rng = np.random.default_rng(seed + thr)
        firsts = special_starts(rng)
        pairs = []; tries = 0
        while len(pairs) < STARTS_PER_THRESHOLD:
            tries += 1
            assert tries < 4000, "threshold %d: cannot plant %d pairs" % (thr, STARTS_PER_THRESHOLD)
            # the first pair that the oracle can be held to as well (libm correctly rounded on both planted points), or else the last one drawn. Whether libm is
            # depends on the angle far more than on the range, so a random start is drawn again with the rest of its cloud; a special start keeps what it gets
            special = firsts.pop(0) if firsts else None
            best = None
            for _ in range(3 if special is not None else 4):
                try:
                    first = special if special is not None else anchor(rng.uniform(*START_RANGE.get(thr, (-PI, PI))), rng)
                    best = tuple(plant(thr, first, len(pairs), rng))
                    if best[0].kept and best[1].kept:
                        break
                except Redraw as e:
                    if special is not None and str(e) == "unreachable":
                        break
            if best is not None:
                pairs.append(best)
        out[thr] = pairs
    return out


# ---- orders -----------------------------------------------------------------------------------------------------------------------------
def _draw(name, make, rng, tries=200, **kw):
    for _ in range(tries):
        try:
            return Cloud(name, make(), **kw)
        except Redraw:
            pass
    raise AssertionError(name + ": no draw meets the generator's conditions")


def _sweep(s, extent, n, rng, jitter=0.4):
    """n azimuths from s over `extent` radians (negative: anticlockwise), jittered inside their steps"""
    step = extent / n
    return [wrap(s + step * (i + (rng.uniform(-jitter, jitter) if 0 < i else 0.0))) for i in range(n)]


def order_clouds(seed=SEED):
    rng = np.random.default_rng(seed + 100)
    out = []
    for s in (0.7, -2.6, 2.9):
        def of(oris, first=None, last=None):
            pts = [point(o, rng) for o in oris]
            pts[0] = anchor(oris[0], rng) if first is None else first
            pts[-1] = anchor(oris[-1], rng) if last is None else last
            return np.stack(pts)
        full = TWO_PI - 0.2
        out.append(_draw("order/clockwise sweep/%g" % s, lambda: of(_sweep(s, full, 40, rng)), rng))
        out.append(_draw("order/reversed sweep/%g" % s, lambda: of(_sweep(s, full, 40, rng)[::-1]), rng))
        out.append(_draw("order/ring-major/%g" % s, lambda: of(sum((_sweep(s, full, 16, rng) for _ in range(4)), [])), rng))
        out.append(_draw("order/random/%g" % s, lambda: of(list(rng.permutation(_sweep(s, full, 48, rng)))), rng))
        out.append(_draw("order/less than half a turn/%g" % s, lambda: of(_sweep(s, 2.9, 24, rng)), rng))
        out.append(_draw("order/anticlockwise, less than half a turn/%g" % s, lambda: of(_sweep(s, -2.9, 24, rng)), rng))
        out.append(_draw("order/1.02 turns/%g" % s, lambda: of(_sweep(s, 1.02 * TWO_PI, 51, rng)), rng))
        zeros = lambda: np.array([[0.0, 0.0, 5.0], [-0.0, 0.0, 5.5], [0.0, -0.0, 6.0], [-0.0, -0.0, 6.5]], F)   # noqa: E731 — atan2f(+-0, +-0) = +-0 / +-pi
        out.append(_draw("order/x = y = +-0 inside a sweep/%g" % s,
                         lambda: np.concatenate([of(_sweep(s, 2.0, 8, rng)), zeros()[:2], of(_sweep(s + 2.2, 2.0, 8, rng)), zeros()[2:], of(_sweep(s + 4.4, 1.6, 8, rng))]), rng))
    for ys in (0.0, -0.0):
        axis = np.array([-9.5, ys, 0.4], F)                                     # atan2f(+-0, x < 0) = +-pi: start or end = -+pi
        tag = "y = %s0" % ("-" if math.copysign(1.0, ys) < 0 else "+")
        out.append(_draw("order/first point on the negative x axis, " + tag,
                         lambda: np.stack([axis] + [point(o, rng) for o in _sweep(-PI, TWO_PI - 0.2, 32, rng)[1:-1]] + [anchor(wrap(PI - 0.2), rng)]), rng))
        out.append(_draw("order/last point on the negative x axis, " + tag,
                         lambda: np.stack([anchor(wrap(PI + 0.2), rng)] + [point(o, rng) for o in _sweep(PI + 0.2, TWO_PI - 0.2, 32, rng)[1:-1]] + [axis]), rng))
    return out


# ---- sizes and the flag's place ---------------------------------------------------------------------------------------------------------------
SIZES = ((1, None), (2, None), (2, 1), (255, 1), (255, 254), (256, 1), (256, 255), (257, 255), (257, 256), (1025, 1), (1025, 255), (1025, 256), (1025, 600),
         (1025, 1024), (1025, None))


def size_clouds(seed=SEED):
    """n points, the flipping point at index k (None: nowhere): points before it that the first rule never lets flip, behind it points from the whole turn — candidates
    of azimuth_flag_kernel's atomicMin in every later block; k = n - 1: the only candidate is the last thread of the last block"""
    rng = np.random.default_rng(seed + 200)
    out = []
    for n, k in SIZES:
        def make():
            s = rng.uniform(-PI, PI)
            oris = [s]
            for i in range(1, n):
                if k is None or i < k:
                    oris.append(wrap(s + rng.uniform(-1.2, 2.8)))
                elif i == k:
                    oris.append(wrap(s + PI + rng.uniform(0.25, 1.2)))
                else:
                    oris.append(rng.uniform(-PI, PI))
            pts = [point(o, rng) for o in oris]
            pts[0] = anchor(oris[0], rng)
            if n > 1:
                pts[-1] = anchor(oris[-1], rng)
            return np.stack(pts)
        c = _draw("size/n = %d, flag at %s" % (n, k), make, rng, tries=400)
        assert c.exact["flag"] == k, c.name
        out.append(c)
    return out


# ---- rotation -------------------------------------------------------------------------------------------------------------------------
ROTATIONS = (dict(incre_rpy=(0.7, -0.9, 2.5), odom_time_diff=0.1), dict(incre_rpy=(0.004, -0.006, 0.035), odom_time_diff=0.0987),
             dict(incre_rpy=(3.0, 1.5, -3.1), odom_time_diff=-0.05))


class RotationCase:
    """a cloud with handed-over times (what rolo_front_set_deskew / orc_project_deskew take: fabs(point.time)) and a de-skew; stated: the float64 statement"""

    def __init__(self, name, xyz, times, incre_rpy, odom_time_diff, scan_period=SCAN_PERIOD):
        self.name, self.xyz, self.times = name, np.ascontiguousarray(xyz, F), np.ascontiguousarray(times, F)
        self.incre_rpy, self.odom_time_diff, self.scan_period = incre_rpy, odom_time_diff, scan_period
        self.ring, self.col = own_pixels(self.xyz)
        self.cfg = dict(n_scan=16 if int(self.ring.max()) < 16 else 128, horizon_scan=H)
        self.order = np.lexsort((self.col, self.ring))
        self.stated = deskew_statement(self.xyz, self.times, incre_rpy, scan_period, odom_time_diff)


def rotation_cases(seed=SEED, n=96):
    rng = np.random.default_rng(seed + 300)
    sp = SCAN_PERIOD
    fixed = [0.0, 0.0, 0.0, 0.0, 1e-45, 1e-40, float(np.finfo(F).tiny), 1.3 * sp, sp, float(np.nextafter(F(sp), F(0))), 0.5 * sp, 1e-3 * sp]
    times = np.array(fixed + list(np.linspace(0.0, 1.3 * sp, n - len(fixed))), F)
    out = []
    for j, rot in enumerate(ROTATIONS):
        while True:
            try:
                az = rng.uniform(-PI, PI, n); el = rng.uniform(-0.3, 0.3, n); r = rng.uniform(3.0, 58.0, n)
                el = np.where(np.abs(el) < 0.01, 0.01, el)
                xyz = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1).astype(F)
                out.append(RotationCase("rotation/%d %r" % (j, rot["incre_rpy"]), xyz, times, **rot))
                break
            except Redraw:
                pass
    return out


def as_rotation_case(cloud, rot, times):
    """an azimuth cloud with the de-skew `rot` at the given times (the exact statement's for the device, the oracle's own for the oracle)"""
    c = RotationCase.__new__(RotationCase)
    c.name, c.xyz, c.times = cloud.name, cloud.xyz, np.ascontiguousarray(times, F)
    c.incre_rpy, c.odom_time_diff, c.scan_period = rot["incre_rpy"], rot["odom_time_diff"], cloud.scan_period
    c.ring, c.col, c.cfg, c.order = cloud.ring, cloud.col, cloud.cfg, cloud.order
    c.stated = deskew_statement(c.xyz, c.times, c.incre_rpy, c.scan_period, c.odom_time_diff)
    return c


_BUILT = None


def build():
    """-> dict(planted={thr: [(Cloud, Cloud)]}, orders=[Cloud], sizes=[Cloud], rotation=[RotationCase]); built once"""
    global _BUILT
    if _BUILT is None:
        _BUILT = dict(planted=planted_clouds(), orders=order_clouds(), sizes=size_clouds(), rotation=rotation_cases())
    return _BUILT


def all_clouds(b=None):
    b = b or build()
    return [c for thr in THRESHOLDS for pair in b["planted"][thr] for c in pair] + b["orders"] + b["sizes"]


if __name__ == "__main__":
    import time
    t0 = time.time()
    b = build()
    for thr in THRESHOLDS:
        pairs = b["planted"][thr]
        kept = sum(1 for p in pairs if p[0].kept and p[1].kept)
        print("threshold %d [%s]: %d pairs, libm correctly rounded on both planted points of %d" % (thr, THRESHOLDS[thr], len(pairs), kept))
    seen = {}
    for c in all_clouds(b):
        for t in c.exact["tags"] + [c.exact["end_tag"]]:
            seen[t] = seen.get(t, 0) + 1
    print("rules taken:", seen)
    print("%d clouds, %d points, built in %.1f s" % (len(all_clouds(b)), sum(c.n for c in all_clouds(b)), time.time() - t0))
