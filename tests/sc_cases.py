"""Constructed clouds for the Scan Context descriptor (sc_make_kernel in rolo_amd/csrc/scancontext.hip) with points planted where the sector or the ring is decided
by one rounding. CPU only: numpy, mpmath and tests/sc_twin.py; neither rolo_amd nor HIP is imported.

The judge is the CORRECTLY ROUNDED statement of xy2theta: sc_twin's own expression (float quotient, fp64 atan, K * a, the branch's 180 - / 180 + / 360 - in fp64,
one rounding to float) run on atan_cr — mpmath's atan at 200 bits rounded once to fp64 — in place of the platform libm, which is not correctly rounded everywhere.
`expected(cloud)` is sc_twin.make_scancontext and sc_twin.keys on that atan; the device is held to it bit for bit.

  (a) sectors[g]  (R, S) = (20, 60), (16, 40), (7, 13), (4, 1024): for every sector edge 360 k / S, k = 1 .. S - 1, the two ADJACENT quotient floats between which
                  the statement's sector goes from k to k + 1 (found by bisection over float ordinals from the float nearest tan of the edge's branch angle), two
                  more floats on either side of the pair, and that nearest float itself. Where the edge is a float, the quotients whose angle is exactly that float
                  are among them: their sector rests on the fp64 theta / 360 * S alone. An edge lies in its own quadrant, so all four branches occur; the axis
                  edges 90 / 180 / 270 are approached from the branch above them (below them the angle never exceeds the edge).
  (b) guard[g]    the geometries of (a) with S divisible by 4. At 90, 180 and 270 degrees the edge E is a float and the sector is decided at M, the midpoint of E
                  and the next float above it. From the branch above the axis (2, 3, 4; the branch below never exceeds E, so it cannot reach M): the two quotient
                  floats on either side of M, the two floats at either rim of the device's guard M -+ 1e-10 (one inside, one outside), and a spread at
                  4, 8, 16 ... floats from M in between. Then the zone next to 0 degrees (branch 1, quotients from 1e-12 down to the smallest denormal float:
                  the guard always fires) and next to 360 (branch 4 with the same quotients, the largest finite quotient y = -3, x = 1e-38, and x = +-0).
                  CLOSEST_ULPS records how close the planted angles come to M, in fp64 ulps of the angle.
  (c) rings[g]    max_radius / R = 50 / 16, 25 / 7, 70 / 64, 79.9 / 20: at every ring edge k * max_radius / R the two adjacent floats r between which the ring
                  goes from k to k + 1 and one more on either side, on an axis (r = |x| exactly) and off it (sqrtf(x * x + y * y) rounds; the stepped coordinate
                  is chosen from the float statement so that both rings occur); the largest float with double(r) <= max_radius and the next one up, which is
                  dropped, on an axis and off it.
  (d) placement   a planted point reserves, in its cloud, its bin under EITHER outcome (both sectors beside its edge, or both rings) and no two points of a cloud
                  share a reserved bin; every point of a cloud has its own z'. A misplaced point therefore always shows as one bin filled that should be empty and
                  one empty that should be filled. A quotient q is realised as x = +-2^e, y = +-q 2^e (the division is exact), e chosen among those that put the
                  radius into the middle 70 % of a ring; a greedy pass opens another cloud where no choice is free.

COUNTS (planted points and clouds per geometry) and CLOSEST_ULPS follow from the construction and mpmath alone and are ASSERTED by tests/test_sc_cases.py.
That test also PRINTS, without asserting them, how many points lie inside the guard and on how many the platform libm's atan is not the correctly rounded
one. With glibc 2.35 these were: planted points / of them inside the guard / libm atan differs —
  sectors (20, 60) 394 / 18 / 4, (16, 40) 261 / 18 / 4, (7, 13) 74 / 0 / 0, (4, 1024) 6819 / 18 / 11; guard 79 / 61 / 0 at each of (20, 60), (16, 40), (4, 1024);
  rings 50 / 16: 124 / 16 / 0, 25 / 7: 52 / 7 / 0, 70 / 64: 508 / 64 / 0, 79.9 / 20: 156 / 20 / 0 (a ring-edge point's angle is mid-sector or on an axis).
On none of those 19 points does sc_twin on libm reach another bin than the statement. Whatever a libm gives, every point stays in the GPU assertion: the
device is held to the correctly rounded value.

build() makes everything once per process (about 2 s)."""
import math

import mpmath as mp
import numpy as np

import sc_twin as T

f32, f64 = np.float32, np.float64
K = 180.0 / math.pi
GUARD = 1e-10                                   # SC_THETA_GUARD of scancontext.hip
SECTOR_GEOMS = (dict(num_ring=20, num_sector=60, max_radius=80.0, lidar_height=2.0), dict(num_ring=16, num_sector=40, max_radius=50.0, lidar_height=0.0),
                dict(num_ring=7, num_sector=13, max_radius=25.0, lidar_height=-1.5), dict(num_ring=4, num_sector=1024, max_radius=80.0, lidar_height=2.0))
RING_GEOMS = (dict(num_ring=16, num_sector=40, max_radius=50.0, lidar_height=0.0), dict(num_ring=7, num_sector=13, max_radius=25.0, lidar_height=-1.5),
              dict(num_ring=64, num_sector=60, max_radius=70.0, lidar_height=1.0), dict(num_ring=20, num_sector=60, max_radius=79.9, lidar_height=2.0))
AXES = ((90.0, 2), (180.0, 3), (270.0, 4))      # the axis edge and the branch above it
# the closest approach of a planted fp64 angle to the midpoint M that decides the sector, in fp64 ulps of the angle: (below M, above M) per axis
CLOSEST_ULPS = {90.0: (3, 15), 180.0: (2, 27), 270.0: (3, 15)}
# planted points, clouds: asserted by tests/test_sc_cases.py (the module is deterministic: nothing is drawn at random)
COUNTS = {"sectors": ((394, 14), (261, 7), (74, 8), (6819, 14)), "guard": ((79, 18), (79, 6), (79, 11)), "rings": ((124, 2), (52, 2), (508, 2), (156, 2))}

_ATAN = {}


def atan_cr(q):
    """the correctly rounded fp64 atan of every element: mpmath at 200 bits, rounded once"""
    out = []
    for v in np.asarray(q, f64).reshape(-1).tolist():
        a = _ATAN.get(v)
        if a is None:
            with mp.workprec(200):
                a = math.nan if v != v else float(mp.atan(mp.mpf(v)))
            _ATAN[v] = a
        out.append(a)
    return np.array(out, f64).reshape(np.shape(q))


def geom_name(P):
    return "R%d_S%d_r%g" % (P["num_ring"], P["num_sector"], P["max_radius"])


# ---- the statement on one point --------------------------------------------------------------------------------------------------------------
def angle64(branch, q, atan=atan_cr):
    """xy2theta's fp64 angle of quotient q (a float32) in `branch` 1 .. 4, before the rounding to float"""
    ka = K * float(atan(np.array([float(q)], f64))[0])
    return (ka, 180.0 - ka, 180.0 + ka, 360.0 - ka)[branch - 1]


def sector_of(theta, S):
    return int(T._clamp_ceil(np.array([(f64(f32(theta)) / f64(360.0)) * f64(S)]), S)[0])


def in_guard(t):
    """the device's test: the angle -+ GUARD rounds to two different floats"""
    return bool(f32(f64(t) - f64(GUARD)) != f32(f64(t) + f64(GUARD)))


def point_bins(pts, P, atan=atan_cr):
    """-> kept, ring, sector (1-based) of every point under sc_twin's expressions on `atan`"""
    pts = np.asarray(pts, f32).reshape(-1, 4)
    x, y = pts[:, 0].copy(), pts[:, 1].copy()
    with np.errstate(all="ignore"):
        r = np.sqrt(x * x + y * y)
        th = T.xy2theta(x, y, atan)
        keep = ~(r.astype(f64) > f64(P["max_radius"]))
        ring = T._clamp_ceil((r.astype(f64) / f64(P["max_radius"])) * f64(P["num_ring"]), P["num_ring"])
        sector = T._clamp_ceil((th.astype(f64) / f64(360.0)) * f64(P["num_sector"]), P["num_sector"])
    return keep, ring, sector


def expected(cloud, P, atan=atan_cr):
    """(desc, ring key, sector key, column norms) of the correctly rounded statement"""
    d = T.make_scancontext(cloud, P, atan)
    return (d,) + T.keys(d)


# ---- float ordinals: consecutive integers for consecutive positive floats ------------------------------------------------------------------------
def ordinal(f):
    return int(np.array([f], f32).view(np.int32)[0])


def from_ordinal(o):
    return np.array([o], np.int32).view(f32)[0]


O_MAX = ordinal(np.finfo(f32).max)


def flip(start, pred):
    """pred: a monotonic predicate on float ordinals 1 .. O_MAX. -> the ordinal a with pred(a) != pred(a + 1), searched outward from `start` in doubling steps,
    then by bisection"""
    p0 = pred(start)
    step, lo, hi = 1, None, None
    while lo is None:
        for cand in (start + step, start - step):
            c = min(max(cand, 1), O_MAX)
            if pred(c) != p0:
                lo, hi = (start, c) if c > start else (c, start)
                break
        else:
            assert step <= 2 * O_MAX, "the predicate never changes"
            step *= 2
    plo = pred(lo)
    while hi - lo > 1:
        m = (lo + hi) // 2
        if pred(m) == plo: lo = m
        else: hi = m
    return lo


# ---- a planted point -------------------------------------------------------------------------------------------------------------------------
class Point:
    """options: [(x, y, bins)], the realisations the placement may choose from, bins = the (ring, sector) pairs the point may land in under either outcome;
    x, y, z, cloud, index: set by the placement. meta: kind, edge, role, branch, q ..."""

    def __init__(self, options, **meta):
        self.options = options; self.meta = meta
        self.x = self.y = self.z = None; self.cloud = self.index = -1; self.bins = None


SIGNS = {1: (1, 1), 2: (-1, 1), 3: (-1, -1), 4: (1, -1)}


def realise(q, branch, P, sectors):
    """quotient q (float32, finite, > 0) as x = +-2^e, y = +-q 2^e in `branch` — the float division gives q back exactly — for every e that puts the radius
    into the middle 70 % of a ring; bins: that ring in each of `sectors`"""
    R, maxr = P["num_ring"], P["max_radius"]
    sx, sy = SIGNS[branch]
    out = []
    e0 = int(math.floor(math.log2(maxr / math.hypot(1.0, float(q))))) + 1
    for e in range(e0, e0 - 12, -1):
        if not -120 < e < 120:
            continue
        x = f32(2.0 ** e)
        y = f32(q * x)
        if not (np.isfinite(y) and float(y) == float(q) * 2.0 ** e and f32(y / x) == q):
            continue
        r = np.sqrt(x * x + y * y)
        pos = float(r) / maxr * R
        ring = math.ceil(pos)
        if ring < 1 or ring > R or not 0.15 <= pos - (ring - 1) <= 0.85:
            continue
        out.append((f32(sx) * x, f32(sy) * y, frozenset((ring, s) for s in sectors)))
    return out


def place(points, P):
    """(d): every point into the first cloud in which one of its options reserves only free bins. -> [cloud (n, 4) float32]; the points get x, y, z, cloud, index"""
    used, members = [], []
    for p in points:
        assert p.options, p.meta
        done = False
        for c in range(len(used) + 1):
            if c == len(used):
                used.append(set()); members.append([])
            for x, y, bins in p.options:
                if not (bins & used[c]):
                    used[c] |= bins
                    p.x, p.y, p.bins, p.cloud, p.index = x, y, bins, c, len(members[c])
                    p.z = f32(1.0 + p.index / 64.0) - f32(P["lidar_height"])     # z' = 1 + index / 64: exact, its own in the cloud, never NO_POINT or 0
                    members[c].append(p)
                    done = True
                    break
            if done:
                break
    return [np.array([[p.x, p.y, p.z, 0.0] for p in m], f32) for m in members]


def single_cloud(p):
    return np.array([[p.x, p.y, p.z, 0.0]], f32)


# ---- (a) sector edges ----------------------------------------------------------------------------------------------------------------------------
def edge_branch(E):
    """-> branch, the branch angle of the edge (degrees)"""
    if E < 90.0: return 1, E
    if E < 180.0: return 2, 180.0 - E
    if E < 270.0: return 3, E - 180.0
    return 4, 360.0 - E


def sector_points(P):
    S = P["num_sector"]
    pts = []
    for k in range(1, S):
        E = 360.0 * k / S
        br, phi = edge_branch(E)
        with mp.workprec(200):
            q0 = f32(1e-7) if phi == 0.0 else f32(1e7) if phi == 90.0 else f32(float(mp.tan(mp.mpf(phi) * mp.pi / 180)))
        sec = lambda o: sector_of(angle64(br, from_ordinal(o)), S)   # noqa: E731
        a = flip(ordinal(q0), lambda o: sec(o) > k)
        assert {sec(a), sec(a + 1)} == {k, k + 1}
        for o in sorted(set(range(a - 2, a + 4)) | {ordinal(q0)}):
            q = from_ordinal(o)
            th = f32(angle64(br, q))
            pts.append(Point(realise(q, br, P, (k, k + 1)), kind="sector", edge=k, branch=br, q=q, off=o - a, nearest=o == ordinal(q0),
                             on_edge=bool(f64(th) == E), sector=sector_of(th, S)))
    return pts


# ---- (b) the guard zone ------------------------------------------------------------------------------------------------------------------------------
def midpoint_above(A):
    return (float(f32(A)) + float(np.nextafter(f32(A), f32(np.inf)))) / 2.0


def guard_points(P):
    S = P["num_sector"]
    assert S % 4 == 0
    pts = []
    for A, br in AXES:
        k = int(A / 360.0 * S)
        M = midpoint_above(A)
        t = lambda o: angle64(br, from_ordinal(o))   # noqa: E731
        start = ordinal(f32(1e-7) if br == 3 else f32(1e7))
        m = flip(start, lambda o: t(o) > M)                       # m, m + 1 lie either side of M
        lo = flip(m, lambda o: o <= m and not in_guard(t(o)))       # the rims by the device's own test: lo + 1 .. hi lie inside the guard
        hi = flip(m, lambda o: o > m and not in_guard(t(o)))
        chosen = {m - 1: "closest", m: "closest", m + 1: "closest", m + 2: "closest", lo: "rim", lo + 1: "rim", hi: "rim", hi + 1: "rim"}
        step = 4
        while m - step > lo + 1 or m + 1 + step < hi:
            for o in (m - step, m + 1 + step):
                if lo + 1 < o < hi:
                    chosen.setdefault(o, "spread")
            step *= 2
        for o in sorted(chosen):
            q = from_ordinal(o)
            pts.append(Point(realise(q, br, P, (k, k + 1)), kind="guard", axis=A, branch=br, q=q, role=chosen[o], t=t(o), M=M, inside=in_guard(t(o)),
                             sector=sector_of(t(o), S)))
    tiny = [f32(v) for v in (1e-12, 1e-15, 1e-20, 1e-30, 1e-37)] + [np.finfo(f32).tiny, f32(1e-40), f32(1e-44), from_ordinal(1)]
    for br, axis in ((1, 0.0), (4, 360.0)):
        for q in tiny:
            tq = angle64(br, q)
            pts.append(Point(realise(q, br, P, (1, S)), kind="guard", axis=axis, branch=br, q=q, role="zero", t=tq, M=None, inside=br == 1, sector=sector_of(tq, S)))   # labelled: below 1e-10 degrees the guard fires, 360 - ka does not reach a midpoint
    # branch 4 at its far end: the largest finite quotient, and x = +-0 — +0 gives q = +inf and 270 degrees, -0 passes x >= 0 and gives q = -inf: 360 + 90 = 450
    k = 3 * S // 4
    w = P["max_radius"] / P["num_ring"]
    ring3 = min(max(math.ceil(3.0 / w), 1), P["num_ring"])
    pts.append(Point([(f32(1e-38), f32(-3.0), frozenset({(ring3, k), (ring3, k + 1)}))], kind="guard", axis=270.0, branch=4, q=f32(3.0) / f32(1e-38), role="far",
                     t=angle64(4, f32(3.0) / f32(1e-38)), M=None, inside=False, sector=k))
    for x0, sec in ((0.0, k), (-0.0, S)):
        opts = [(f32(x0), f32(-(ring - 0.5) * w), frozenset({(ring, k), (ring, k + 1), (ring, S), (ring, 1)})) for ring in range(1, P["num_ring"] + 1)]
        pts.append(Point(opts, kind="guard", axis=270.0, branch=4, q=f32(np.inf) if x0 == 0.0 and not np.signbit(x0) else f32(-np.inf), role="far", t=270.0 if sec == k else 450.0,
                         M=None, inside=False, sector=sec))
    return pts                                                      # the far points are labelled outside: 270 and 450 are floats


# ---- (c) ring edges ------------------------------------------------------------------------------------------------------------------------------------
def ring_of(r, P):
    """-> the ring of float radius r, 0 where the point is dropped"""
    if float(r) > P["max_radius"]:
        return 0
    return int(T._clamp_ceil(np.array([(f64(r) / f64(P["max_radius"])) * f64(P["num_ring"])]), P["num_ring"])[0])


def _root(x, y):
    x, y = f32(x), f32(y)
    return np.sqrt(x * x + y * y)


def ring_points(P):
    R, S, maxr = P["num_ring"], P["num_sector"], P["max_radius"]
    pts = []
    axis_dirs = ((1, 0), (0, 1), (-1, 0), (0, -1))

    def axis_sector(d):
        th = T.xy2theta(f32(d[0]), f32(d[1]), atan_cr)[0]
        return sector_of(th, S)

    for k in range(1, R + 1):
        last = k == R
        ek = k * maxr / R
        lower, upper = (k, 0) if last else (k, k + 1)             # the rings (0: dropped) either side of the edge
        verdict = (lambda r: ring_of(r, P) == 0) if last else (lambda r: ring_of(r, P) > k)
        # on an axis: r = |x| exactly
        a = flip(ordinal(f32(ek)), lambda o: verdict(from_ordinal(o)))
        offs = (0, 1) if last else (-1, 0, 1, 2)
        for j, off in enumerate(offs):
            r = from_ordinal(a + off)
            opts = []
            for d in axis_dirs[j % 4:] + axis_dirs[:j % 4]:
                s = axis_sector(d)
                opts.append((f32(d[0]) * r, f32(d[1]) * r, frozenset({(lower, s), (upper or R, s)})))
            pts.append(Point(opts, kind="ring", edge=k, on_axis=True, off=off, ring=ring_of(r, P)))
        # off the axes: the larger coordinate is stepped, the root rounds; one candidate direction per few sectors, mid-sector
        cands = [((k * 7 + 3 * i) % S) + 1 for i in range(8)]
        per_off = {off: [] for off in offs}
        for s in dict.fromkeys(cands):
            with mp.workprec(200):                                   # not the platform libm: the clouds are the same on every machine
                al = mp.mpf(2 * s - 1) * mp.pi / S
                cx, cy = float(ek * mp.cos(al)), float(ek * mp.sin(al))
            if min(abs(cx), abs(cy)) < 0.05 * ek:                   # a sector whose middle is an axis (sector 7 of 13): not off the axes
                continue
            step_x = abs(cx) >= abs(cy)
            fixed = f32(cy if step_x else cx)
            sign = f32(math.copysign(1.0, cx if step_x else cy))
            xy = (lambda o: (sign * from_ordinal(o), fixed)) if step_x else (lambda o: (fixed, sign * from_ordinal(o)))
            a = flip(ordinal(f32(abs(cx if step_x else cy))), lambda o: verdict(_root(*xy(o))))
            for off in offs:
                x, y = xy(a + off)
                keep, ring, sec = point_bins(np.array([[x, y, 0, 0]], f32), P)
                if int(sec[0]) != s:
                    continue
                per_off[off].append((x, y, frozenset({(lower, s), (upper or R, s)})))
        for off in offs:
            ring0 = ring_of(_root(per_off[off][0][0], per_off[off][0][1]), P)
            pts.append(Point(per_off[off], kind="ring", edge=k, on_axis=False, off=off, ring=ring0))
    return pts


# ---- everything ---------------------------------------------------------------------------------------------------------------------------------------
class Suite:
    """one geometry's planted points and the clouds they were placed into"""

    def __init__(self, kind, P, points):
        self.kind, self.P, self.points = kind, dict(P), points
        self.clouds = place(points, P)
        self.name = "%s/%s" % (kind, geom_name(P))


_BUILT = None


def build():
    """-> dict(sectors=[Suite per SECTOR_GEOMS], guard=[Suite per geometry with S % 4 == 0], rings=[Suite per RING_GEOMS]); built once"""
    global _BUILT
    if _BUILT is None:
        _BUILT = dict(sectors=[Suite("sectors", P, sector_points(P)) for P in SECTOR_GEOMS],
                      guard=[Suite("guard", P, guard_points(P)) for P in SECTOR_GEOMS if P["num_sector"] % 4 == 0],
                      rings=[Suite("rings", P, ring_points(P)) for P in RING_GEOMS])
    return _BUILT


def all_suites(b=None):
    b = b or build()
    return b["sectors"] + b["guard"] + b["rings"]


def closest_ulps(suite):
    """per axis the closest approach of a planted fp64 angle to M from below and from above, in ulps of the angle (M and the angle share a binade)"""
    out = {}
    for A, _ in AXES:
        M = midpoint_above(A)
        d = [(p.meta["t"] - M) / math.ulp(M) for p in suite.points if p.meta["axis"] == A and p.meta["M"] is not None]
        out[A] = (int(round(min(-v for v in d if v <= 0))), int(round(min(v for v in d if v > 0))))
    return out


if __name__ == "__main__":
    import time
    t0 = time.time()
    b = build()
    for s in all_suites(b):
        print("%s: %d points in %d clouds (largest %d)" % (s.name, len(s.points), len(s.clouds), max(len(c) for c in s.clouds)))
    for s in b["guard"]:
        print(s.name, "closest approach to M in fp64 ulps (below, above):", closest_ulps(s))
    print("built in %.1f s" % (time.time() - t0))
