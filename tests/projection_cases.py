"""Constructed raw clouds for K1, the projection (project_kernel in rolo_amd/csrc/front.hip; oracle/rolo_oracle_front.cpp:80-98), with the expected column, verdict
and pixel owner of every point. CPU only: numpy, mpmath and the host libm; neither rolo_amd nor HIP is imported.

The column of a point is decided by two statements that share nothing but the float steps behind the angle:

  the float statement   atan2f of the host libm (through ctypes), then the oracle's expression step by step in numpy float32 / float64:
                        horizonAngle = float(double(atan2f(x, y) * 180.f) / M_PI), ang_res_x = float(360.0 / float(H)),
                        column = -round((horizonAngle - 90.0) / ang_res_x) + H / 2, one wrap at >= H;
  the exact statement   mpmath.atan2 at 256 bits rounded ONCE to float32 (the nearest of the candidate and its two neighbours, compared in mpmath, so that
                        no rounding through a double can slip in; signed zeros by the rules of C99 F.9.1.4, which mpmath does not know), then the same steps.

A planted point is KEPT where the two give the same atan2f bits: the target is the correctly rounded value (as in tests/golden/make_golden_edges.py), and a point
where this machine's libm misses it is dropped, because no device answer could match both. The dropped points are kept apart (Case `dropped[H]`): reported, never
asserted.

  edges[H]   H in 1024, 1800, 2048, 4096 on 16 rings: for every column edge a pair of ADJACENT floats (one coordinate differs by one ulp) that the float statement
             puts into the two columns beside the edge; edge e on ring e % 16, so the pairs of one ring sit 16 columns apart. Every tenth kept pair gets a third
             point two ulps further from the edge, at another range, more than 256 indices after the pair: it must lose the pixel to the earlier point.
  axes[H]    the axes, signed zeros, denormals, FLT_MIN, the diagonals, |x| / |y| = 2^+-24 and the four signed (0, 0, z).
  gates      ranges exactly at, and one float beside, lidar_min_range / lidar_max_range (defaults and 0.7 / 50.3), and points whose x*x + y*y + z*z gives another
             verdict when a product is contracted into an FMA.
  rings      ring values n_scan - 1, n_scan, 32768, 65520, 65535, with downsample_rate 1 and 3.

build() makes everything once per process (about 4 s)."""
import ctypes
import ctypes.util
import math

import mpmath as mp
import numpy as np

F = np.float32
N_SCAN = 16
EDGE_H = (1024, 1800, 2048, 4096)
THIN = {1024: 1, 1800: 1, 2048: 1, 4096: 1}    # every edge; the special edges survive any thinning (plant_edges)
SEED = 20261020
DEFAULT_GATES = (2.0, 1000.0)                  # config/params.yaml lidarMinRange / lidarMaxRange = front_params' defaults
CONFIGURED_GATES = (0.7, 50.3)                 # neither is representable in few bits

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]
_libm.atan2f.restype = ctypes.c_float


# ---- the float statement ------------------------------------------------------------------------------------------------------------
def atan2f(x, y):
    """the host libm's atan2f(x, y), element by element"""
    x = np.asarray(x, F).reshape(-1); y = np.asarray(y, F).reshape(-1)
    f = _libm.atan2f
    return np.array([f(a, b) for a, b in zip(x.tolist(), y.tolist())], F)


def c_round(v):
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def column_of_angle(a, H):
    """imageProjection.cpp:437-444 from the float atan2 value on: -> column, or -1 where the reference drops the point"""
    t = np.asarray(a, F) * F(180)                                        # float * int: a float product
    ha = (t.astype(np.float64) / math.pi).astype(F)                      # / M_PI in double, stored in a float
    res = np.float64(F(360.0 / float(F(H))))                             # :438
    col = (-c_round((ha.astype(np.float64) - 90.0) / res) + H // 2).astype(np.int64)
    col = np.where(col >= H, col - H, col)
    return np.where((col < 0) | (col >= H), -1, col)


def float_range(xyz):
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return np.sqrt(x * x + y * y + z * z)                                # float32 throughout, nothing contracted


# ---- the exact statement ------------------------------------------------------------------------------------------------------------
def _neg(v):
    return math.copysign(1.0, v) < 0


def atan2_exact(x, y):
    """-> (the correctly rounded float32 atan2(x, y), the unrounded value as an mpf or None for the signed-zero cases)"""
    x = float(x); y = float(y)
    if x == 0.0:                                                          # atan2(+-0, y): +-0 for y > 0 or y = +0, +-pi for y < 0 or y = -0
        v = F(0.0) if (y > 0 or (y == 0 and not _neg(y))) else F(math.pi)
        return (F(-v) if _neg(x) else v), None
    with mp.workprec(256):
        v = mp.atan2(mp.mpf(x), mp.mpf(y))
        c = F(float(v))
        cands = (np.nextafter(c, F(-np.inf)), c, np.nextafter(c, F(np.inf)))
        err = [abs(mp.mpf(float(k)) - v) for k in cands]
        assert sorted(err)[0] != sorted(err)[1]                           # atan of a rational is no midpoint of two floats
        return cands[err.index(min(err))], v


def atan2_exact_array(x, y):
    return np.array([atan2_exact(a, b)[0] for a, b in zip(np.asarray(x, F).tolist(), np.asarray(y, F).tolist())], F)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def flip_margin(a, H, most=4):
    """the smallest k <= most for which atan2 value a moved by k float ulps (either way) changes the column; most + 1 if none does"""
    a = np.asarray(a, F); c0 = column_of_angle(a, H)
    out = np.full(a.shape, most + 1, np.int32)
    up = a.copy(); dn = a.copy()
    for k in range(1, most + 1):
        up = np.nextafter(up, F(np.inf)); dn = np.nextafter(dn, F(-np.inf))
        hit = (out > most) & ((column_of_angle(up, H) != c0) | (column_of_angle(dn, H) != c0))
        out[hit] = k
    return out


# ---- a case -------------------------------------------------------------------------------------------------------------------------
class Case:
    """xyz (n, 3) float32, ring uint16, cfg = the keyword arguments of front_params; per point: angle / angle_cr (atan2f bits of the two statements), col (the
    float statement's column, -1 where the point is refused), col_cr (the exact statement's), accept, owner (the point is the first of its pixel, so it is in the
    output), same_bits. `meta` holds per-point arrays of the builder (edge number, side ...)."""

    def __init__(self, name, cfg, xyz, ring, **meta):
        self.name = name; self.cfg = dict(cfg)
        self.xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3); self.ring = np.ascontiguousarray(ring, np.uint16)
        self.meta = meta
        H = cfg["horizon_scan"]; ns = cfg["n_scan"]; ds = cfg.get("downsample_rate", 1)
        lo, hi = F(cfg.get("lidar_min_range", DEFAULT_GATES[0])), F(cfg.get("lidar_max_range", DEFAULT_GATES[1]))
        self.range = float_range(self.xyz)
        self.angle = atan2f(self.xyz[:, 0], self.xyz[:, 1])
        self.angle_cr = atan2_exact_array(self.xyz[:, 0], self.xyz[:, 1])
        self.same_bits = bits(self.angle) == bits(self.angle_cr)
        r = self.ring.astype(np.int64)
        gate = ~((self.range < lo) | (self.range > hi)) & (r < ns) & (r % ds == 0)
        col, col_cr = column_of_angle(self.angle, H), column_of_angle(self.angle_cr, H)
        self.accept = gate & (col >= 0)
        self.col = np.where(self.accept, col, -1).astype(np.int32)
        self.col_cr = np.where(gate & (col_cr >= 0), col_cr, -1).astype(np.int32)
        self.margin = flip_margin(self.angle_cr, H)
        self.owner = np.zeros(len(r), bool)                                # "first point to claim a pixel wins" (:451)
        idx = np.nonzero(self.accept)[0]
        _, first = np.unique(r[idx] * H + col[idx], return_index=True)
        self.owner[idx[first]] = True
        key = np.ascontiguousarray(self.xyz).view(np.uint32).reshape(-1, 3)
        assert len({tuple(k) for k in key.tolist()}) == len(key), name + ": two points with the same coordinates cannot be told apart in the output"

    @property
    def n(self):
        return int(self.owner.sum())

    def subset(self, name, mask, **meta):
        m = {k: v[mask] for k, v in self.meta.items()}; m.update(meta)
        return Case(name, self.cfg, self.xyz[mask], self.ring[mask], **m)


def read_back(case, proj):
    """where the points of `case` went in a projection (the dict of pyorc.project / FrontEnd.project): -> (column, row) per raw point, -1 for a point that is not in
    `extracted`; the points are found by the bits of their coordinates, the row from start_ring / end_ring"""
    where = {tuple(k): i for i, k in enumerate(np.ascontiguousarray(case.xyz).view(np.uint32).reshape(-1, 3).tolist())}
    col = np.full(len(case.ring), -1, np.int32); row = np.full(len(case.ring), -1, np.int32)
    ext = np.ascontiguousarray(proj["extracted"][:, :3], F).view(np.uint32).reshape(-1, 3).tolist()
    first = np.asarray(proj["start_ring"]).astype(np.int64) - 4           # start = first - 1 + 5, end = last - 5 (:485, :503)
    rows = np.searchsorted(first, np.arange(len(ext)), side="right") - 1
    for j, k in enumerate(ext):
        i = where.get(tuple(k))
        if i is not None:
            col[i] = proj["point_col_ind"][j]; row[i] = rows[j]
    return col, row


def expected_columns(case):
    return np.where(case.owner, case.col, -1).astype(np.int32)


def describe(case, dev_col, ref_col, most=12):
    """the points whose column differs, for an assertion message"""
    bad = np.nonzero(np.asarray(dev_col) != np.asarray(ref_col))[0]
    lines = ["%s: %d of %d points differ (column -1: not in the output)" % (case.name, bad.size, len(case.ring))]
    for i in bad[:most]:
        lines.append("  #%d x=%r (%s) y=%r (%s) ring %d: device column %d, oracle column %d, correctly rounded atan2f %r (libm %r), column flips at %s ulp of it"
                     % (i, float(case.xyz[i, 0]), float(case.xyz[i, 0]).hex(), float(case.xyz[i, 1]), float(case.xyz[i, 1]).hex(), case.ring[i], dev_col[i], ref_col[i],
                        float(case.angle_cr[i]), float(case.angle[i]), case.margin[i] if case.margin[i] <= 4 else "> 4"))
    return "\n".join(lines)


# ---- float ordinals: consecutive integers for consecutive floats ----------------------------------------------------------------------------
def _ordinal(f):
    i = np.asarray(f, F).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def _from_ordinal(o):
    o = np.asarray(o, np.int64)
    return np.where(o < 0, (-o) | 0x80000000, o).astype(np.uint32).view(F)


def _adjacent_flip(start, verdict, reach=1 << 22):
    """Arrays of float ordinals `start`; verdict(ordinals) -> an integer per element. Finds for every element two ADJACENT ordinals (a, b) with
    verdict(a) == verdict(start) != verdict(b): doubling steps to either side until the verdict changes, then bisection. -> a, b, found"""
    start = np.asarray(start, np.int64)
    v0 = verdict(start)
    a = start.copy(); b = start.copy(); found = np.zeros(start.shape, bool)
    k = 1
    while not found.all() and k <= reach:
        for s in (k, -k):
            cand = start + s
            new = ~found & (verdict(cand) != v0)
            b[new] = cand[new]; found |= new
        k *= 2
    while True:
        open_ = found & (np.abs(b - a) > 1)
        if not open_.any():
            return a, b, found
        m = np.where(open_, (a + b) // 2, a)
        same = verdict(m) == v0
        a = np.where(open_ & same, m, a); b = np.where(open_ & ~same, m, b)


# ---- edges --------------------------------------------------------------------------------------------------------------------------
def special_edges(H):
    """edge e lies between column e - 1 (mod H) and column e: the wrap edge (H - 1 | 0), the edges beside column H / 4 (atan2f jumps from +pi to -pi inside
    it) and beside the other axis columns 0, H / 2, 3 H / 4"""
    s = set()
    for c in (0, H // 4, H // 2, 3 * H // 4):
        s.update((c, c + 1))
    return s


def plant_edges(H, thin=1, seed=SEED):
    """-> (all planted points as a Case in planting order with meta edge / side / pair, the number of edges that gave no pair)"""
    sp = special_edges(H)
    e = np.array([k for k in range(H) if k % thin == 0 or k in sp], np.int64)
    rng = np.random.default_rng(seed + H)
    r = rng.uniform(2.0, 80.0, e.size)
    ha = 90.0 + (H / 2 - e + 0.5) * (360.0 / H)                            # the angle of the edge in degrees, in (-180, 180]
    ha = np.where(ha > 180.0, ha - 360.0, ha)
    th = np.deg2rad(ha)
    x0 = (r * np.sin(th)).astype(F); y0 = (r * np.cos(th)).astype(F)
    z0 = (r * rng.uniform(0.01, 0.05, e.size) * rng.choice([-1.0, 1.0], e.size)).astype(F)   # small, never zero: the range stays above r
    step_x = np.abs(x0) <= np.abs(y0)                                      # step the smaller coordinate: the finer one in angle

    def at(o):
        v = _from_ordinal(o)
        return np.where(step_x, v, x0), np.where(step_x, y0, v)

    def verdict(o):
        return column_of_angle(atan2f(*at(o)), H)

    o0 = _ordinal(np.where(step_x, x0, y0))
    a, b, found = _adjacent_flip(o0, verdict)
    ca, cb = verdict(a), verdict(b)
    lo_col = (e - 1) % H
    good = found & (((ca == lo_col) & (cb == e)) | ((ca == e) & (cb == lo_col)))
    swap = ca == e                                                         # side 0: the point in column e - 1, side 1: the point in column e
    o_lo = np.where(swap, b, a); o_hi = np.where(swap, a, b)
    # the two points of a pair follow each other
    n = int(good.sum())
    xyz = np.empty((2 * n, 3), F)
    for s, o in ((0, o_lo), (1, o_hi)):
        x, y = at(o)
        xyz[s::2] = np.stack([x, y, z0], 1)[good]
    rg = np.repeat((e % N_SCAN)[good], 2); ed = np.repeat(e[good], 2); sd = np.tile(np.array([0, 1]), n)
    # the candidates for a third point: two ulps further from the edge than either point of the pair, at 1.5 times the height with the other sign
    far = np.stack([2 * o_lo - o_hi + (o_lo - o_hi), 2 * o_hi - o_lo + (o_hi - o_lo)], 1)[good]      # o + 2 (o - partner)
    third = np.empty((2 * n, 3), F)
    for s in (0, 1):
        full = np.zeros(e.size, np.int64); full[good] = far[:, s]
        x, y = at(full)
        third[s::2] = np.stack([x, y, (z0 * F(-1.5)).astype(F)], 1)[good]
    cfg = dict(n_scan=N_SCAN, horizon_scan=H)
    return Case("edges[%d] as planted" % H, cfg, xyz, rg, edge=ed, side=sd, third=third), int((~good).sum())


def edge_cases(H):
    """-> dict(kept=Case, dropped=Case, planted=int, share=float, thirds=int, no_pair=int)"""
    planted, no_pair = plant_edges(H, THIN[H])
    keep = planted.same_bits
    n = len(keep)
    pair_kept = keep[0::2] & keep[1::2]
    # every tenth kept pair gets a third point (sides alternate) — where the third point itself is one that both statements agree on and that stays in the column
    chosen = np.nonzero(pair_kept)[0][::10]
    cand = np.array([2 * p + (j % 2) for j, p in enumerate(chosen)], np.int64)
    t_xyz = planted.meta["third"][cand]
    t = Case("thirds", planted.cfg, t_xyz, planted.ring[cand])
    ok = t.same_bits & (t.col == planted.col[cand]) & t.accept
    cand = cand[ok]; t_xyz = t_xyz[ok]
    first = np.zeros(n, bool); first[cand] = True; first[cand ^ 1] = True   # the pairs with a third point go first, the third points last: > 256 indices apart
    order = np.concatenate([np.nonzero(keep & first)[0], np.nonzero(keep & ~first)[0]])
    assert (keep & ~first).sum() >= 256
    xyz = np.concatenate([planted.xyz[order], t_xyz]); ring = np.concatenate([planted.ring[order], planted.ring[cand]])
    edge = np.concatenate([planted.meta["edge"][order], planted.meta["edge"][cand]])
    side = np.concatenate([planted.meta["side"][order], planted.meta["side"][cand]])
    is_third = np.concatenate([np.zeros(order.size, bool), np.ones(cand.size, bool)])
    kept = Case("edges[%d]" % H, planted.cfg, xyz, ring, edge=edge, side=side, is_third=is_third)
    assert np.array_equal(kept.owner, ~is_third), "every pair point owns its pixel and every third point loses it"
    # the dropped points: the two sides of an edge on different rings (2 (e % 8) + side), so that no answer to one of them can hide another
    d = ~keep
    dropped = Case("dropped[%d]" % H, planted.cfg, planted.xyz[d], (2 * (planted.meta["edge"][d] % 8) + planted.meta["side"][d]), edge=planted.meta["edge"][d],
                   side=planted.meta["side"][d])
    return dict(kept=kept, dropped=dropped, planted=n, share=float(keep.mean()), thirds=int(cand.size), no_pair=no_pair)


# ---- axes ---------------------------------------------------------------------------------------------------------------------------
def _own_pixels(xyz, H):
    """rings for points that may share a column: the k-th point of a column goes on ring k"""
    col = column_of_angle(atan2f(xyz[:, 0], xyz[:, 1]), H)
    seen = {}
    ring = np.zeros(len(col), np.uint16)
    for i, c in enumerate(col.tolist()):
        ring[i] = seen.get(c, 0); seen[c] = ring[i] + 1
    assert ring.max() < N_SCAN
    return ring


def axes_case(H):
    r = F(7.25); den = F(1e-42); tiny = np.finfo(F).tiny; big = F(16.0); small = F(16.0 * 2.0 ** -24)
    z = F(0.375)
    p = [(0.0, r), (0.0, -r), (-0.0, -r), (-0.0, r), (r, 0.0), (-r, 0.0), (r, -0.0), (-r, -0.0),
         (den, -r), (-den, -r), (den, r), (-den, r), (tiny, r), (-tiny, r), (tiny, -r), (-tiny, -r),
         (r, r), (r, -r), (-r, r), (-r, -r)]
    for sx in (1, -1):
        for sy in (1, -1):
            p += [(sx * small, sy * big), (sx * big, sy * small)]           # |x| / |y| = 2^-24 and 2^24
    xyz = [(a, b, z * F(1 + 0.125 * k)) for k, (a, b) in enumerate(p)]
    xyz += [(0.0, 0.0, 5.0), (-0.0, 0.0, 5.5), (0.0, -0.0, 6.0), (-0.0, -0.0, 6.5), (0.0, 0.0, -7.0)]   # atan2f(+-0, +-0) = +-0 / +-pi; the range is |z|
    xyz = np.array(xyz, F)
    return Case("axes[%d]" % H, dict(n_scan=N_SCAN, horizon_scan=H), xyz, _own_pixels(xyz, H))


# ---- gates --------------------------------------------------------------------------------------------------------------------------
def _round_f32(num, den):
    """the positive rational num / den rounded once to float32 (nearest, ties to even); normal range only"""
    e = num.bit_length() - den.bit_length() - 24
    while True:                                                            # 2^23 <= num / (den 2^e) < 2^24
        n, d = (num, den << e) if e >= 0 else (num << -e, den)
        if n < (d << 23): e -= 1
        elif n >= (d << 24): e += 1
        else: break
    q, rem = divmod(n, d)
    if 2 * rem > d or (2 * rem == d and (q & 1)): q += 1
    return F(math.ldexp(q, e))


def _exact(f):
    return float(f).as_integer_ratio()


def _sum_sq_forms(x, y, z):
    """x*x + y*y + z*z as written (three rounded products, two rounded sums) and as a compiler that contracts may evaluate it — fma(z, z, fma(x, x, y*y)) and
    fma(z, z, fma(y, y, x*x)) — in exact rational arithmetic with one rounding per operation"""
    def fma(a, b, c):
        (an, ad), (bn, bd), (cn, cd) = _exact(a), _exact(b), _exact(c)
        return _round_f32(an * bn * cd + cn * ad * bd, ad * bd * cd)
    plain = F(F(F(x * x) + F(y * y)) + F(z * z))
    return plain, fma(z, z, fma(x, x, F(y * y))), fma(z, z, fma(y, y, F(x * x)))


def _contraction_points(gate, lo, hi, want, rng, tries=4000):
    """points beside `gate` whose verdict under [lo, hi] is another one once a product is contracted (both forms), found among `tries` seeded candidates: float64
    products against float32 steps first, then confirmed in exact arithmetic"""
    g = float(F(gate))
    az = rng.uniform(-np.pi, np.pi, tries); el = rng.uniform(0.3, 1.2, tries) * rng.choice([-1.0, 1.0], tries)
    x = (g * np.cos(el) * np.sin(az)).astype(F); y = (g * np.cos(el) * np.cos(az)).astype(F)
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    z = (np.sign(el) * np.sqrt(np.maximum(g * g - xd * xd - yd * yd, 0.0))).astype(F)
    out = []
    for k in (0, 1, -1, 2, -2):
        zz = _from_ordinal(_ordinal(z) + k); zd = zz.astype(np.float64)
        plain = (x * x + y * y) + zz * zz
        fused = ((xd * xd + (y * y).astype(np.float64)).astype(F).astype(np.float64) + zd * zd).astype(F)   # products exact in double, one rounding each (nearly)
        ok = lambda s: ~((np.sqrt(s) < F(lo)) | (np.sqrt(s) > F(hi)))   # noqa: E731
        for i in np.nonzero(ok(plain) != ok(fused))[0]:
            forms = _sum_sq_forms(x[i], y[i], zz[i])
            v = [bool(ok(np.array([s], F))[0]) for s in forms]
            if forms[0] == plain[i] and v[1] != v[0] and v[2] != v[0]:
                out.append((x[i], y[i], zz[i]))
            if len(out) >= want:
                return np.array(out, F)
    return np.array(out, F).reshape(-1, 3)


def gates_case(name, lo, hi, H=1800, seed=SEED):
    rng = np.random.default_rng(seed + int(1000 * lo))
    flo, fhi = F(lo), F(hi)
    pts = []
    for g in (flo, fhi):
        pts += [(g, 0, 0), (-g, 0, 0), (0, g, 0), (0, -g, 0), (0, 0, g), (0, 0, -g)]            # sqrtf(float(g * g)) == g: exactly at the gate, accepted
        for a, b, c, h in ((3, 4, 0, 5), (4, 3, 0, 5), (2, 3, 6, 7), (6, 2, 3, 7), (3, 6, 2, 7)):   # Pythagorean triples scaled to the gate, where that is exact
            s = float(g) / h
            q = np.array([[a * s, -b * s, c * s]], F)
            if float_range(q)[0] == g and np.all(q.astype(np.float64) == np.array([a * s, -b * s, c * s])):
                pts.append(tuple(q[0]))
    exact_n = len(pts)
    # one float beside the gate: step z until the verdict flips, keep the two adjacent floats
    m = 6
    az = rng.uniform(-np.pi, np.pi, 2 * m); el = rng.uniform(0.2, 1.0, 2 * m) * rng.choice([-1.0, 1.0], 2 * m)
    g = np.repeat(np.array([flo, fhi], np.float64), m)
    x = (g * np.cos(el) * np.sin(az)).astype(F); y = (g * np.cos(el) * np.cos(az)).astype(F); z = (g * np.sin(el)).astype(F)

    def verdict(o):
        rr = float_range(np.stack([x, y, _from_ordinal(o)], 1))
        return (~((rr < flo) | (rr > fhi))).astype(np.int64)
    a, b, found = _adjacent_flip(_ordinal(z), verdict)
    assert found.all()
    for o in (a, b):
        pts += [tuple(q) for q in np.stack([x, y, _from_ordinal(o)], 1)]
    step_n = len(pts) - exact_n
    contr = np.concatenate([_contraction_points(flo, lo, hi, 3, rng), _contraction_points(fhi, lo, hi, 3, rng)])
    xyz = np.concatenate([np.array(pts, F).reshape(-1, 3), contr])
    kind = np.array([0] * exact_n + [1] * step_n + [2] * len(contr))
    cfg = dict(n_scan=N_SCAN, horizon_scan=H, lidar_min_range=lo, lidar_max_range=hi)
    return Case(name, cfg, xyz, _own_pixels(xyz, H), kind=kind)


# ---- rings --------------------------------------------------------------------------------------------------------------------------
def rings_cases(H=1800):
    values = list(range(N_SCAN)) + [N_SCAN, N_SCAN + 1, 32768, 65520, 65535]
    ring = np.repeat(np.array(values, np.uint16), 3)
    col = (np.arange(ring.size) * 29 + 5) % H                               # every point its own column (centre azimuth), so no pixel hides a wrong verdict
    ha = np.deg2rad(90.0 + (H / 2 - col) * (360.0 / H))
    r = 4.0 + 0.25 * np.arange(ring.size)
    xyz = np.stack([r * np.sin(ha), r * np.cos(ha), 0.1 * r], 1).astype(F)
    return [Case("rings/downsample %d" % ds, dict(n_scan=N_SCAN, horizon_scan=H, downsample_rate=ds), xyz, ring) for ds in (1, 3)]


_BUILT = None


def build():
    """-> dict(edges={H: edge_cases(H)}, axes={H: Case}, gates=[Case, Case], rings=[Case, Case]); built once"""
    global _BUILT
    if _BUILT is None:
        _BUILT = dict(edges={H: edge_cases(H) for H in EDGE_H}, axes={H: axes_case(H) for H in EDGE_H},
                      gates=[gates_case("gates/default", *DEFAULT_GATES), gates_case("gates/configured", *CONFIGURED_GATES)], rings=rings_cases())
    return _BUILT


def all_cases(b=None):
    """every asserted cloud (the dropped points are not among them)"""
    b = b or build()
    return [b["edges"][H]["kept"] for H in EDGE_H] + [b["axes"][H] for H in EDGE_H] + b["gates"] + b["rings"]


def octant(case):
    return np.clip(np.floor((case.angle_cr.astype(np.float64) + math.pi) / (math.pi / 4)), 0, 7).astype(np.int64)


if __name__ == "__main__":
    import time
    t0 = time.time()
    b = build()
    for H in EDGE_H:
        c = b["edges"][H]
        k = c["kept"]
        m = k.margin[~k.meta["is_third"]]
        print("edges[%d]: planted %d, kept %.1f %% (%d + %d third points), dropped %d, edges without a pair %d; column flips at 1 ulp of atan2f for %.1f %% of the kept"
              % (H, c["planted"], 100 * c["share"], int((~k.meta["is_third"]).sum()), c["thirds"], len(c["dropped"].ring), c["no_pair"], 100 * float((m == 1).mean())))
    for c in all_cases(b)[len(EDGE_H):]:
        print("%s: %d points, %d accepted, n = %d, libm atan2f correctly rounded on %d" % (c.name, len(c.ring), int(c.accept.sum()), c.n, int(c.same_bits.sum())))
    print("built in %.1f s" % (time.time() - t0))
