"""The CPU statement of Scan Context (reference src/scancontext/Scancontext.cpp, include/scancontext/Scancontext.h), numpy scalars and serial Python loops only.

The reference itself cannot be built for the tests (it needs Eigen, PCL and OpenCV), so THIS twin is the parity target of tests/test_gpu_scancontext.py: the
same arithmetic as the HIP kernels, written independently of them from the reference's text. Expression types are the reference's: float32 where it computes
in float, float64 where an operand is a double (Python floats in the inner loops: the same IEEE doubles), every sum taken serially in index order in a Python
loop (Eigen's own order is not known: parity unpinned), atan through math.atan (the platform's libm, fp64) unless a caller passes another (tests/sc_cases.py: a correctly rounded one). Operations that are independent per point or per
searched key are written element-wise on arrays; nothing is ever summed by numpy."""
import math

import numpy as np

f32, f64 = np.float32, np.float64

DEFAULTS = dict(num_ring=20, num_sector=60, max_radius=80.0, lidar_height=2.0, num_exclude_recent=30, num_candidates=3, search_ratio=0.1, dist_thres=0.4)   # Scancontext.h:80-95
TREE_MAKING_PERIOD = 10   # :99
FAR = 10000000.0


def _atan(q):
    """fp64 atan of every element through math.atan (numpy's own array loop may take a vector routine with other rounding)"""
    return np.array([math.atan(v) if v == v else math.nan for v in np.asarray(q, f64).tolist()], f64)


def xy2theta(x, y, atan=None):
    """:23-36, element-wise on float32 arrays: the quotient is a float, atan and the rest fp64, the return value float. `atan` replaces the platform libm's
    (an fp64 array in, an fp64 array out): tests/sc_cases.py runs the same expression on a correctly rounded one"""
    at = atan or _atan
    x, y = np.atleast_1d(np.asarray(x, f32)), np.atleast_1d(np.asarray(y, f32))
    K = f64(180.0) / f64(math.pi)
    out = np.zeros(x.shape, f32)
    with np.errstate(all="ignore"):
        b1 = (x >= 0) & (y >= 0); b2 = (x < 0) & (y >= 0); b3 = (x < 0) & (y < 0); b4 = (x >= 0) & (y < 0)
        out[b1] = (K * at(y[b1] / x[b1])).astype(f32)
        out[b2] = (f64(180.0) - (K * at(y[b2] / (-x[b2])))).astype(f32)
        out[b3] = (f64(180.0) + (K * at(y[b3] / x[b3]))).astype(f32)
        out[b4] = (f64(360.0) - (K * at((-y[b4]) / x[b4]))).astype(f32)
    return out


def _clamp_ceil(v, hi):
    """max(min(hi, int(ceil(v))), 1) element-wise; int(NaN) is INT_MIN on x86, so 1"""
    with np.errstate(all="ignore"):
        c = np.ceil(v)
        return np.where(c != c, 1.0, np.clip(c, 1.0, float(hi))).astype(np.int64)


def make_scancontext(pts, P=DEFAULTS, atan=None):
    """:151-195. Returns the num_ring x num_sector float64 matrix (float32 values) or None for an empty cloud. The per-point arithmetic is element-wise on
    arrays (the same IEEE operations as on scalars); the maximum per bin is exact in any order. `atan`: see xy2theta"""
    pts = np.asarray(pts, f32).reshape(-1, 4)
    if len(pts) == 0:
        return None
    R, S = P["num_ring"], P["num_sector"]
    maxr, h = f64(P["max_radius"]), f64(P["lidar_height"])
    x, y, z = pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()
    with np.errstate(all="ignore"):
        zf = (z.astype(f64) + h).astype(f32)                 # :168
        r = np.sqrt(x * x + y * y)                            # :171, float
        assert r.dtype == f32
        th = xy2theta(x, y, atan)                             # :172
        keep = ~(r.astype(f64) > maxr)                        # :175
        ring = _clamp_ceil((r.astype(f64) / maxr) * f64(R), R)             # :178
        sector = _clamp_ceil((th.astype(f64) / f64(360.0)) * f64(S), S)    # :179
    desc = np.full((R, S), -1000.0, f64)
    np.maximum.at(desc, (ring[keep] - 1, sector[keep] - 1), zf[keep].astype(f64))   # :182-183: only a larger z' replaces the bin
    desc[desc == -1000.0] = 0.0
    desc[desc == 0.0] = 0.0   # a zero maximum is +0.0
    return desc


def keys(desc):
    """ring key (:198-211, rounded to float as eig2stdvec :62-66), sector key (:214-227), column norms: serial fp64 sums in index order
    (Python floats are IEEE doubles: the same additions as np.float64 scalars, one rounding each)"""
    R, S = desc.shape
    d = desc.tolist()
    ring = np.zeros(R, f32); sector = np.zeros(S, f64); norm = np.zeros(S, f64)
    for r in range(R):
        s = 0.0
        for c in range(S):
            s = s + d[r][c]
        ring[r] = f32(f64(s / float(S)))
    for c in range(S):
        s = 0.0; ss = 0.0
        for r in range(R):
            s = s + d[r][c]
            ss = ss + d[r][c] * d[r][c]
        sector[c] = s / float(R)
        norm[c] = math.sqrt(ss)
    return ring, sector, norm


def ringkey_dist(a, b):
    """nanoflann.hpp:383-408: float, groups of four left to right, then single terms. b: one key or an array of keys (one distance each, element-wise)"""
    a = np.asarray(a, f32); b = np.asarray(b, f32)
    n = len(a)
    res = np.zeros(b.shape[:-1], f32)
    d = 0
    with np.errstate(all="ignore"):
        while d + 3 < n:
            d0, d1, d2, d3 = a[d] - b[..., d], a[d + 1] - b[..., d + 1], a[d + 2] - b[..., d + 2], a[d + 3] - b[..., d + 3]
            res = res + (((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3)
            d += 4
        while d < n:
            d0 = a[d] - b[..., d]
            res = res + d0 * d0
            d += 1
    assert res.dtype == f32
    return res


def candidates(ringkeys, query, n_search, K):
    """the min(K, n_search) nearest of keys 0 .. n_search-1 by (distance, index); K = 0: all, in index order"""
    if K == 0:
        return list(range(n_search))
    dist = ringkey_dist(ringkeys[query], np.asarray(ringkeys[:n_search], f32).reshape(n_search, -1))
    d = sorted(zip(dist.tolist(), range(n_search)))
    return [i for _, i in d[:min(K, n_search)]]


def fast_align(vk1, vk2):
    """:93-113 with circshift :39-59: shifted[j] = vk2[(j - s) mod S]"""
    vk1 = np.asarray(vk1, f64).tolist(); vk2 = np.asarray(vk2, f64).tolist()
    S = len(vk1)
    arg, mn = 0, FAR
    for s in range(S):
        acc = 0.0
        for j in range(S):
            d = vk1[j] - vk2[(j - s) % S]
            acc = acc + d * d
        cur = math.sqrt(acc) if acc == acc and acc != math.inf else acc
        if cur < mn:
            arg, mn = s, cur
    return arg


def dist_direct(c1, n1, c2, n2, shift):
    """:69-90 on sc2 shifted right by `shift` columns. c1 / c2: the matrices as lists of columns, n1 / n2: the column norms"""
    S = len(c1)
    cnt = 0
    total = 0.0
    for j in range(S):
        jj = (j - shift) % S
        if n1[j] == 0 or n2[jj] == 0:
            continue
        dot = 0.0
        for u, v in zip(c1[j], c2[jj]):
            dot = dot + u * v
        total = total + dot / (n1[j] * n2[jj])
        cnt += 1
    return 1.0 - total / cnt if cnt else math.nan


def distance(e1, e2, search_ratio):
    """distanceBtnScanContext :116-148 on two stored entries (desc, ring, sector, norm) -> (distance, shift)"""
    S = e1[0].shape[1]
    a = fast_align(e1[2], e2[2])
    radius = int(math.floor(0.5 * search_ratio * S + 0.5))   # C round() of a non-negative value
    space = sorted({a} | {(a + i) % S for i in range(1, radius + 1)} | {(a - i) % S for i in range(1, radius + 1)})
    c1, c2 = e1[0].T.tolist(), e2[0].T.tolist()
    n1, n2 = e1[3].tolist(), e2[3].tolist()
    arg, mn = 0, FAR
    for s in space:
        cur = dist_direct(c1, n1, c2, n2, s)
        if cur < mn:
            arg, mn = s, cur
    return f64(mn), arg


def deg2rad(degrees):
    """:17-20: float parameter, double arithmetic, float result"""
    return f32(f64(f32(degrees)) * f64(math.pi) / f64(180.0))


class Store:
    """the descriptors and keys of makeAndSaveScancontextAndKeys (:236-250) with detection against the first n_search of them"""

    def __init__(self, **kw):
        self.P = dict(DEFAULTS); self.P.update(kw)
        self.entries = []
        self.atan = None   # the platform libm's; see xy2theta

    def add(self, pts):
        desc = make_scancontext(pts, self.P, self.atan)
        if desc is None:
            return -1
        self.entries.append((desc,) + keys(desc))
        return len(self.entries) - 1

    def detect(self, query, n_search):
        """:284-342 -> dict(loop_id, yaw, nn_idx, nn_align, min_dist, cand, cand_dist, cand_align)"""
        out = dict(loop_id=-1, yaw=f32(0.0), nn_idx=0, nn_align=0, min_dist=f64(FAR), cand=[], cand_dist=[], cand_align=[])
        if n_search <= 0:
            return out
        P = self.P
        cand = candidates([e[1] for e in self.entries], query, n_search, P["num_candidates"])
        for c in cand:
            d, al = distance(self.entries[query], self.entries[c], P["search_ratio"])
            out["cand_dist"].append(d); out["cand_align"].append(al)
            if d < out["min_dist"]:
                out["min_dist"], out["nn_align"], out["nn_idx"] = d, al, c
        out["cand"] = cand
        if out["min_dist"] < P["dist_thres"]:
            out["loop_id"] = out["nn_idx"]
        out["yaw"] = deg2rad(f64(out["nn_align"]) * (f64(360.0) / f64(P["num_sector"])))
        return out


class Manager:
    """SCManager's two user calls with the rebuild-period counter and the stale searched set of :263-282"""

    def __init__(self, **kw):
        self.store = Store(**kw)
        self.counter = 0
        self.n_search = 0
        self.searched = []   # the searched-set size of every detect call (the staircase)

    def makeAndSaveScancontextAndKeys(self, pts):
        return self.store.add(pts)

    def detectLoopClosureID(self):
        n = len(self.store.entries)
        if n < self.store.P["num_exclude_recent"] + 1:
            self.searched.append(None)
            return -1, f32(0.0)
        if self.counter % TREE_MAKING_PERIOD == 0:
            self.n_search = n - self.store.P["num_exclude_recent"]
        self.counter += 1
        self.searched.append(self.n_search)
        r = self.store.detect(n - 1, self.n_search)
        self.last = r
        return r["loop_id"], r["yaw"]
