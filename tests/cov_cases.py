"""Constructed neighbourhoods for the covariance stage (K5's second half), their exact classes and the exact statement of the six regularisations.

A cloud is made of CLUSTERS of exactly k points whose diameter is below a quarter of the distance to any other cluster: the k nearest neighbours of every point (itself
included) are its own cluster, so every member shares ONE covariance — and float32 coordinates are rationals, so that covariance is known exactly (fractions.Fraction).
Its spectrum and projectors are taken with mpmath at 60 digits, and the six rules of rot_vgicp_impl.hpp:458-491 are stated as functions of the exact matrix,
sum_k v(lambda_k) P_k; FROBENIUS is (C + 1e-3 I) ||(C + 1e-3 I)^-1||_F with 1e-3 the double it is.

Classes (derived here by Fraction elimination for the rank and exact equality of entries for the ties — never by a float eigen-solver):
  W   full rank, adjacent eigenvalue ratios in [3, 1e3]     T2  exact tie of the two largest (sets invariant under the quarter turn about z)
  T3  exact triple tie (octahedral sets)                     R2  exactly planar            R1  exactly collinear            R0  k coincident points
  N1  a float-rounded oblique line: rank 3, two eigenvalues ~1e-15 of the first

build_fixture() (mpmath, the oracle: tests/golden/make_golden_cov_cases.py) makes tests/golden/cov_cases.npz; everything else here — load(), check_covariances() — needs
numpy alone, so that the GPU test depends neither on mpmath nor on a numpy generator."""
import os
import zlib
from fractions import Fraction as F

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cov_cases.npz")

KS = (20, 7, 33, 100)   # knn_tail_kernel<20, true> / <20>, <32>, <64>, knn_tail_loop_kernel with its rounds of 64
CLOUDS = ("regular", "mixed")
RULES = ("NONE", "MIN_EIG", "NORMALIZED_MIN_EIG", "PLANE", "FROBENIUS", "PLANE_S")   # = RegularizationMethod's values
NONE, MIN_EIG, NORMALIZED_MIN_EIG, PLANE, FROBENIUS, PLANE_S = range(6)
SVD_RULES = (MIN_EIG, NORMALIZED_MIN_EIG, PLANE, PLANE_S)
CLASSES = ("W", "T2", "T3", "R2", "R1", "R0", "N1")
W, T2, T3, R2, R1, R0, N1 = range(7)
SIX = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
EPS = 1e-3             # the regularisations' constant, the double it is
FLOOR = 8 * 2.0 ** -53  # floor of a relative bar
MP_DIGITS = 60

# (clusters of the source, clusters of the target) per k: sizes that are no multiple of 256, unequal workgroup counts (256 queries each)
SIZES = {"regular": {20: (13, 27), 7: (19, 38), 33: (5, 13), 100: (2, 6)}, "mixed": {20: (13, 40), 7: (19, 38), 33: (5, 13), 100: (3, 10)}}

# W: half extents of the oblique box, the dyadic grid of its offsets (a translate by a lattice centre is then exact in float32), and where it may sit
W_KINDS = {
    "Wt": ((1e-3, 4e-4, 1.5e-4), 21, "tiny"),   # 1e-3 m: every eigenvalue below 1e-3
    "Wm": ((0.3, 0.12, 0.02), 14, "any"),       # 0.3 m: lambda_3 < 1e-3 < lambda_2; also at (900, -700, 30)
    "Wf": ((0.4, 0.05, 0.004), 17, "near"),     # flat: lambda_3 / lambda_1 below 1e-3
    "Wb": ((40.0, 12.0, 2.5), 10, "far"),       # 40 m: every eigenvalue above 1e-3
}


# ---------------------------------------------------------------- exact arithmetic ----------------------------------------------------------------
def exact_moments(p32):
    """(sums of the coordinates [3], centred product sums [3][3], covariance [3][3]) of float32 points, in Fractions"""
    k = len(p32)
    X = [[F(float(v)) for v in p] for p in np.asarray(p32, np.float32)]
    s1 = [sum(x[a] for x in X) for a in range(3)]
    m = [s / k for s in s1]
    D = [[x[a] - m[a] for a in range(3)] for x in X]
    s2 = [[sum(d[a] * d[b] for d in D) for b in range(3)] for a in range(3)]
    return s1, s2, [[v / k for v in r] for r in s2]


def exact_rank(C):
    A = [list(r) for r in C]
    rank = 0
    for col in range(3):
        piv = next((r for r in range(rank, 3) if A[r][col] != 0), None)
        if piv is None:
            continue
        A[rank], A[piv] = A[piv], A[rank]
        for r in range(rank + 1, 3):
            f = A[r][col] / A[rank][col]
            A[r] = [a - f * b for a, b in zip(A[r], A[rank])]
        rank += 1
    return rank


def exact_class(C):
    """the class from the exact matrix alone: rank by elimination, ties by equality of entries; N1 from the exact invariants (e2 / tr^2 ~ lambda_2 / lambda_1)"""
    rank = exact_rank(C)
    if rank < 3:
        return (R0, R1, R2)[rank]
    offdiag0 = C[0][1] == 0 and C[0][2] == 0 and C[1][2] == 0
    if offdiag0 and C[0][0] == C[1][1] == C[2][2]:
        return T3
    if offdiag0 and C[0][0] == C[1][1] and C[0][0] > C[2][2]:
        return T2
    tr = C[0][0] + C[1][1] + C[2][2]
    e2 = C[0][0] * C[1][1] - C[0][1] ** 2 + C[0][0] * C[2][2] - C[0][2] ** 2 + C[1][1] * C[2][2] - C[1][2] ** 2
    if e2 < tr * tr * F(1, 10 ** 8):
        return N1
    return W


def _spectrum(C, cls):
    """eigenvalues (descending) and unit eigenvectors with mpmath; the zeros of a rank-deficient class are set exactly"""
    import mpmath as mp
    mp.mp.dps = MP_DIGITS
    A = mp.matrix(3, 3)
    for a in range(3):
        for b in range(3):
            A[a, b] = mp.mpf(C[a][b].numerator) / mp.mpf(C[a][b].denominator)
    if cls == R0:
        return A, [mp.mpf(0)] * 3, [mp.matrix([1, 0, 0]), mp.matrix([0, 1, 0]), mp.matrix([0, 0, 1])]
    E, Q = mp.eigsy(A)
    lam = [E[2], E[1], E[0]]
    vec = [Q[:, 2], Q[:, 1], Q[:, 0]]
    for i in range({R2: 2, R1: 1}.get(cls, 3), 3):
        lam[i] = mp.mpf(0)
    return A, lam, vec


def _rule_values(rule, lam, s3=1):
    """v(lambda_k) of the SVD rules, rot_vgicp_impl.hpp:471-489 (lam descending; s3: the sign on a zero third singular value)"""
    import mpmath as mp
    eps = mp.mpf(EPS)
    if rule == MIN_EIG:
        v = [max(l, eps) for l in lam]
    elif rule == NORMALIZED_MIN_EIG:
        v = [max(l / lam[0], eps) for l in lam]
    elif rule == PLANE:
        v = [mp.mpf(1), mp.mpf(1), eps]
    else:
        s = lam[0] + lam[1] + lam[2]
        v = [lam[0] / s, lam[1] / s, eps]
    v[2] = s3 * v[2]
    return v


def exact_statement(p32):
    """class, expected six-entry matrices per rule (NaN where nothing is defined), the alternative of an R2 cluster (sign -1 on the zero singular value),
    the exact leading direction and v(lambda_1) per rule, and the eigenvalues (float64 roundings of the 60-digit values)"""
    import mpmath as mp
    s1, s2, C = exact_moments(p32)
    cls = exact_class(C)
    A, lam, vec = _spectrum(C, cls)
    exp = np.full((6, 6), np.nan); alt = np.full((6, 6), np.nan); vtop = np.full(6, np.nan)

    def six(M):
        return [float(M[a, b]) for a, b in SIX]

    exp[NONE] = [float(C[a][b]) for a, b in SIX]
    Mreg = A + mp.mpf(EPS) * mp.eye(3)
    Minv = mp.inverse(Mreg)
    exp[FROBENIUS] = six(Mreg * mp.sqrt(sum(Minv[a, b] ** 2 for a in range(3) for b in range(3))))
    P = [v * v.T for v in vec]
    for rule in SVD_RULES:
        defined = cls in (W, T2, R2) or (cls == T3 and rule in (MIN_EIG, NORMALIZED_MIN_EIG)) or (cls == R0 and rule in (MIN_EIG, PLANE))
        if cls != R0:
            vtop[rule] = float(_rule_values(rule, lam)[0])
        if not defined:
            continue
        for s3, out in ((1, exp), (-1, alt)):
            if s3 < 0 and cls != R2:
                continue
            v = _rule_values(rule, lam, s3)
            out[rule] = six(v[0] * P[0] + v[1] * P[1] + v[2] * P[2])
    d = np.array([float(x) for x in vec[0]])
    return dict(cls=cls, exp=exp, alt=alt, vtop=vtop, dvec=d, lam=np.array([float(l) for l in lam]), s1=s1, s2=s2, C=C)


# ---------------------------------------------------------------- shapes ----------------------------------------------------------------
def _rational_rotation(rng):
    """an oblique rotation with rational entries: from a quaternion of small integers, none zero and no two equal in magnitude"""
    while True:
        q = rng.integers(1, 9, 4) * rng.choice([-1, 1], 4)
        if len(set(abs(int(v)) for v in q)) == 4:
            break
    a, b, c, d = (float(v) for v in q)
    n = a * a + b * b + c * c + d * d
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]]) / n


def _dyadic(rng, k, lo, hi, bits):
    return rng.integers(lo, hi + 1, k).astype(np.float64) / 2.0 ** bits


def shape_offsets(kind, k, rng):
    """offsets (k, 3) float64 of one cluster about its centre; all on a dyadic grid but N1's"""
    if kind in W_KINDS:
        h, bits, _ = W_KINDS[kind]
        u = rng.random((k, 3)) * 2 - 1
        return np.round((u * np.array(h)) @ _rational_rotation(rng).T * 2.0 ** bits) / 2.0 ** bits
    if kind == "T2":     # orbits of the quarter turn about z: (x, y, z) -> (-y, x, z); k = 4 m + r with r points on the axis
        pts = []
        for _ in range(k // 4):
            x, y = _dyadic(rng, 1, 12, 24, 6)[0], _dyadic(rng, 1, 1, 11, 6)[0]
            z = _dyadic(rng, 1, -6, 6, 6)[0]
            pts += [(x, y, z), (-y, x, z), (-x, -y, z), (y, -x, z)]
        pts += [(0.0, 0.0, z / 64.0) for z in range(1, k % 4 + 1)]
        return np.array(pts)
    if kind == "T3":     # octahedral orbits: the 6 axis points, the 8 corners of a cube, the centre
        def axis(a):
            return [(a, 0, 0), (-a, 0, 0), (0, a, 0), (0, -a, 0), (0, 0, a), (0, 0, -a)]

        def cube(a):
            return [(sx * a, sy * a, sz * a) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
        sets = {20: axis(0.25) + axis(0.375) + cube(0.125), 7: axis(0.25) + [(0, 0, 0)]}[k]
        return np.array(sets, np.float64)
    if kind in ("R2z", "R2o"):   # z constant / the oblique dyadic plane spanned by (1, 0, 1/2) and (0, 1, -1/4)
        s, t = _dyadic(rng, k, -90, 90, 8), _dyadic(rng, k, -40, 40, 8)
        return np.stack([s, t, np.zeros(k) if kind == "R2z" else s / 2 - t / 4], 1)
    if kind in ("R1x", "R1o"):   # on the x axis / along (1, 1/2, -1/4), dyadic parameters
        t = _dyadic(rng, k, -24, 24, 6)
        return np.stack([t, np.zeros(k), np.zeros(k)], 1) if kind == "R1x" else np.stack([t, t / 2, -t / 4], 1)
    if kind == "R0":
        return np.zeros((k, 3))
    if kind == "N1":     # an oblique line, rounded to float32 when placed
        t = rng.random(k) * 0.8 - 0.4
        return np.stack([t, 0.3 * t, -0.7 * t], 1)
    raise ValueError(kind)


def place(off, centre, exact=True):
    p = np.asarray(centre, np.float64) + off
    p32 = p.astype(np.float32)
    assert not exact or np.array_equal(p32.astype(np.float64), p), "a translate that is not exact in float32"
    return p32


def _w_ok(kind, st):
    """the W shape is what its kind promises: adjacent ratios in [3, 1e3] and its side of each clamp"""
    l = st["lam"]
    if st["cls"] != W or not (3 <= l[0] / l[1] <= 1e3 and 3 <= l[1] / l[2] <= 1e3):
        return False
    return {"Wt": l[0] < EPS and l[2] / l[0] > EPS, "Wm": l[2] < EPS < l[1] and l[2] / l[0] > EPS, "Wf": l[2] / l[0] < EPS, "Wb": l[2] > EPS and l[2] / l[0] > EPS}[kind]


def sums_regular(st):
    """all nine sums of the moments epilogue are non-zero and inside [2^-500, 2^500]: the wavefront takes the shared-reciprocal path"""
    vals = list(st["s1"]) + [st["s2"][a][b] for a, b in SIX]
    return all(v != 0 and F(2) ** -500 <= abs(v) <= F(2) ** 500 for v in vals)


# ---------------------------------------------------------------- clouds ----------------------------------------------------------------
MIXED_KINDS = ("Wm", "Wt", "Wf", "Wb", "Wm@far", "R2z", "R2o", "R2z@far", "R2o@far", "R1x", "R1o", "R0", "N1", "T2", "T3")
SOURCE_ORDER = ("R0", "Wm", "N1", "R1o", "R2o", "T2", "Wt", "R1x", "R2z", "T3", "Wf", "Wm@far", "R2z@far", "Wb", "R2o@far")
REGULAR_KINDS = ("Wm", "Wt", "Wf", "Wb", "Wm@far")
FAR_W = (900.0, -700.0, 30.0)
FAR_R2 = (512.0, 256.0, 2.0)


def _slots(rng):
    """lattice centres: (16 i + 1/2) within +-48.5 m (each the middle of a 1 m voxel) without the origin's cell, whose eight neighbours (+-1/2) take the tiny clusters;
    the 40 m clusters sit on a 4 096 m lattice"""
    g = [(16.0 * i + 0.5, 16.0 * j + 0.5, 16.0 * l + 0.5) for i in range(-3, 4) for j in range(-3, 4) for l in range(-3, 4) if (i, j, l) != (0, 0, 0)]
    g = [g[i] for i in rng.permutation(len(g))]
    tiny = [(sx * 0.5, sy * 0.5, sz * 0.5) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    far = [(4096.0 * i, 4096.0 * j, 0.0) for i, j in ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1))]
    return dict(any=g, near=g, tiny=tiny, far=far)


KIND_CLASS = {"Wm": W, "Wt": W, "Wf": W, "Wb": W, "R2z": R2, "R2o": R2, "R1x": R1, "R1o": R1, "R0": R0, "N1": N1, "T2": T2, "T3": T3}


def _make_shape(kind, k, side):
    """the shape of a kind for one k and one side: ONE draw, used wherever the kind appears on that side (regular and mixed clouds alike), so that the expected matrices
    of its exact translates are one block of the fixture"""
    base = kind.split("@")[0]
    rng = np.random.default_rng(zlib.crc32(("cov-cases-shape-%s-%d-%s" % (base, k, side)).encode()))
    for _ in range(400):
        off = shape_offsets(base, k, rng)
        if base not in W_KINDS:
            return off
        st = exact_statement(place(off, (0.5, 0.5, 0.5) if base != "Wb" else (4096.0, 0.0, 0.0)))
        if _w_ok(base, st):
            return off
    raise AssertionError("no %s shape for k = %d" % (kind, k))


def build_cloud_pair(cloud, k):
    """{src, tgt: dict(pts (n, 3) float32 shuffled, owner (n,), centre (m, 3), kind [m])}. The target takes the kinds in turn; the source takes some of the target's
    centres with the same kind and the source's own draw of its shape (a registration of the pair has overlap and a non-zero residual), and the kinds the target had no room for"""
    rng = np.random.default_rng(zlib.crc32(("cov-cases-%s-%d" % (cloud, k)).encode()))
    kinds = [q for q in (MIXED_KINDS if cloud == "mixed" else REGULAR_KINDS) if k in (20, 7) or q not in ("T2", "T3")]
    n_src, n_tgt = SIZES[cloud][k]
    slots = _slots(rng)
    all_kinds = [kinds[i % len(kinds)] for i in range(n_tgt)] if n_tgt >= len(kinds) else list(kinds[len(kinds) - n_tgt:]) + list(kinds[:len(kinds) - n_tgt])
    n_extra = len(all_kinds) - n_tgt     # clusters of the source alone
    seen = {}
    centres = []
    for q in all_kinds:
        base = q.split("@")[0]
        j = seen.get(q, 0); seen[q] = j + 1
        if q == "Wm@far":
            c = (FAR_W[0] + 16.0 * j, FAR_W[1], FAR_W[2])
        elif q.endswith("@far"):
            c = (FAR_R2[0] + 32.0 * j + (16.0 if q == "R2o@far" else 0.0), FAR_R2[1], FAR_R2[2])
        else:
            c = slots[W_KINDS[base][2] if base in W_KINDS else "near"].pop(0)
        centres.append(c)
    # the target's clusters that the source shares: one of each kind in SOURCE_ORDER (degenerate and regular kinds in turn) before a second of any
    inst = [all_kinds[:i].count(q) for i, q in enumerate(all_kinds[:n_tgt])]
    shared = sorted(sorted(range(n_tgt), key=lambda i: (inst[i], SOURCE_ORDER.index(all_kinds[i])))[: n_src - n_extra])
    members = {"src": shared + list(range(n_tgt, n_tgt + n_extra)), "tgt": list(range(n_tgt))}
    out = {}
    for side in ("src", "tgt"):
        pts, owner, cc, kk = [], [], [], []
        for j, ci in enumerate(members[side]):
            q = all_kinds[ci]
            pts.append(place(_make_shape(q, k, side), centres[ci], exact=q != "N1"))
            owner += [j] * k; cc.append(centres[ci]); kk.append(q)
        pts = np.concatenate(pts); owner = np.array(owner, np.int16)
        perm = rng.permutation(pts.shape[0])   # shuffled: the gather is scattered
        out[side] = dict(pts=np.ascontiguousarray(pts[perm]), owner=owner[perm], centre=np.array(cc), kind=kk)
    return out


def separation_ok(pts, owner):
    """every cluster's diameter is below a quarter of its distance to any other cluster (float64 on float32 coordinates: exact enough by orders of magnitude)"""
    p = pts.astype(np.float64)
    d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
    same = owner[:, None] == owner[None, :]
    for c in np.unique(owner):
        m = owner == c
        diam = d[np.ix_(m, m)].max()
        if not diam < 0.25 * d[np.ix_(m, ~m)].min():
            return False
    return bool((d[~same] > 0).all())


def xyz1(p):
    return np.ascontiguousarray(np.concatenate([p.astype(np.float32), np.ones((p.shape[0], 1), np.float32)], 1))


def oracle_covariances(rule, k, src, tgt):
    from oracle import pyorc
    o = pyorc.Reg(pyorc.default_params(regularization=rule, k_correspondences=k, voxel_type=pyorc.VOXEL_UNIFORM, voxel_resolution=1.0))
    o.set_target(xyz1(tgt)); o.set_source(xyz1(src))
    assert o.compute_covariances() == 0
    return o.source_covs()[:, :3, :3], o.target_covs()[:, :3, :3]


def build_fixture():
    """every array of tests/golden/cov_cases.npz (mpmath and the oracle are needed)"""
    d = {}
    uniq, blocks = {}, []   # one expected block per distinct exact covariance (a shape translated by a lattice centre keeps its matrix exactly)
    for cloud in CLOUDS:
        for k in KS:
            pair = build_cloud_pair(cloud, k)
            for side in ("src", "tgt"):
                c = pair[side]
                key = "%s_k%d_%s" % (cloud, k, side)
                st = [exact_statement(c["pts"][c["owner"] == j]) for j in range(len(c["kind"]))]
                assert separation_ok(c["pts"], c["owner"]), key
                assert [s["cls"] for s in st] == [KIND_CLASS[q.split("@")[0]] for q in c["kind"]], key
                if cloud == "regular":   # (no vanishing cross sum: in particular no cluster is symmetric about a coordinate plane)
                    assert all(s["cls"] == W and sums_regular(s) for s in st), key
                idx = []
                for s in st:
                    ckey = tuple(tuple(r) for r in s["C"])
                    if ckey not in uniq:
                        uniq[ckey] = len(blocks); blocks.append(s)
                    idx.append(uniq[ckey])
                d[key + "_pts"] = c["pts"]; d[key + "_owner"] = c["owner"]
                d[key + "_cls"] = np.array([s["cls"] for s in st], np.int8); d[key + "_block"] = np.array(idx, np.int16)
                d[key + "_near"] = np.array([np.abs(cc).max() <= 60.0 for cc in c["centre"]])
    d["block_exp"] = np.stack([s["exp"] for s in blocks])
    r2 = [i for i, s in enumerate(blocks) if s["cls"] == R2]
    r1 = [i for i, s in enumerate(blocks) if s["cls"] in (R1, N1)]
    d["block_r2"] = np.array(r2, np.int16); d["block_alt"] = np.stack([blocks[i]["alt"][list(SVD_RULES)] for i in r2])
    d["block_r1"] = np.array(r1, np.int16); d["block_vtop"] = np.stack([blocks[i]["vtop"] for i in r1]); d["block_dvec"] = np.stack([blocks[i]["dvec"] for i in r1])
    # the bars: per rule the oracle's largest deviation from the exact matrix over the W and T2 clusters of all k, relative to the largest |entry|
    dev = np.zeros(6)
    for cloud in CLOUDS:
        for k in KS:
            src, tgt = d["%s_k%d_src_pts" % (cloud, k)], d["%s_k%d_tgt_pts" % (cloud, k)]
            for rule in range(6):
                for side, cov in zip(("src", "tgt"), oracle_covariances(rule, k, src, tgt)):
                    key = "%s_k%d_%s" % (cloud, k, side)
                    cls = d[key + "_cls"][d[key + "_owner"]]
                    E = unpack6(d["block_exp"][d[key + "_block"][d[key + "_owner"]], rule])
                    sel = (cls == W) | (cls == T2)
                    rel = np.abs(cov[sel] - E[sel]).max((1, 2)) / np.abs(E[sel]).max((1, 2))
                    dev[rule] = max(dev[rule], rel.max())
    d["oracle_dev"] = dev
    return d


# ---------------------------------------------------------------- the fixture and the assertions (numpy only) ----------------------------------------------------------------
def unpack6(c6):
    c6 = np.asarray(c6)
    M = np.empty(c6.shape[:-1] + (3, 3))
    for i, (a, b) in enumerate(SIX):
        M[..., a, b] = c6[..., i]; M[..., b, a] = c6[..., i]
    return M


class Case:
    """one cloud of the fixture"""

    def __init__(self, z, cloud, k, side):
        key = "%s_k%d_%s" % (cloud, k, side)
        self.key, self.k = key, k
        self.pts, self.owner, self.cls, self.block = z[key + "_pts"], z[key + "_owner"].astype(np.int64), z[key + "_cls"].astype(np.int64), z[key + "_block"].astype(np.int64)
        nb = z["block_exp"].shape[0]
        alt = np.full((nb, 6, 6), np.nan); alt[np.ix_(z["block_r2"], SVD_RULES)] = z["block_alt"]
        self.vtop = np.full((nb, 6), np.nan); self.vtop[z["block_r1"]] = z["block_vtop"]
        self.dvec = np.full((nb, 3), np.nan); self.dvec[z["block_r1"]] = z["block_dvec"]
        self.exp, self.alt, self.near = unpack6(z["block_exp"]), unpack6(alt), z[key + "_near"]
        self.xyz1 = xyz1(self.pts)
        self.pcls = self.cls[self.owner]


def load(path=GOLDEN):
    z = np.load(path)
    cases = {(cloud, k, side): Case(z, cloud, k, side) for cloud in CLOUDS for k in KS for side in ("src", "tgt")}
    return cases, np.array(z["oracle_dev"])


def bars(oracle_dev):
    """relative bar per rule: 10 x the oracle's recorded deviation from exact arithmetic, floored at 8 * 2^-53"""
    return np.maximum(10.0 * np.asarray(oracle_dev), FLOOR)


def knn_inside_clusters(case, idx):
    """the premise: every point's k nearest neighbours (itself included) are exactly its own cluster"""
    own = case.owner[np.asarray(idx)]
    return bool((own == case.owner[:, None]).all()) and all(len(set(r)) == case.k for r in np.asarray(idx))


def check_covariances(case, rule, cov, bar, ref=None):
    """Every assertion of the statement for one cloud and one rule. cov: (n, 3, 3) as computed; bar: the rule's relative bar; ref: the oracle's (n, 3, 3) for the same
    points (the R2 signs and R0's NaN pattern are compared with it). Returns (worst ratio to the bar over the well-defined comparisons, {+1: n, -1: n} R2 signs)."""
    cov = np.asarray(cov)
    worst = 0.0
    signs = {1: 0, -1: 0}
    name = "%s %s" % (case.key, RULES[rule])
    fails = []   # every comparison is made and printed before anything is raised

    def close(M, E, what, scale=None):
        nonlocal worst
        s = np.abs(E).max() if scale is None else scale
        r = float(np.abs(M - E).max() / (bar * s))
        worst = max(worst, r)
        if not (np.isfinite(M).all() and r <= 1.0):
            fails.append("%s: %s: %.3g x the bar (%.3g relative)" % (name, what, r, bar))

    for c in range(len(case.cls)):
        cl = int(case.cls[c]); blk = case.block[c]
        mem = np.nonzero(case.owner == c)[0]
        M = cov[mem]; E = case.exp[blk, rule]
        tag = "cluster %d (%s)" % (c, CLASSES[cl])
        if rule in (NONE, FROBENIUS) or cl in (W, T2) or (cl == T3 and rule in (MIN_EIG, NORMALIZED_MIN_EIG)) or (cl == R0 and rule in (MIN_EIG, PLANE)):
            if cl == R0 and rule == NONE:
                assert (M == 0).all(), "%s: %s: NONE of coincident points is not zero" % (name, tag)
            else:
                close(M, E[None], tag)
        elif cl == T3:      # PLANE, PLANE_S on a triple tie: any orthonormal frame serves; the eigenvalues are defined
            want = np.array([EPS, 1.0, 1.0]) if rule == PLANE else np.array([EPS, 1.0 / 3, 1.0 / 3])
            assert np.isfinite(M).all(), "%s: %s: not finite" % (name, tag)
            close(M, np.swapaxes(M, 1, 2), tag + " symmetry", scale=np.abs(M).max())
            close(np.linalg.eigvalsh(0.5 * (M + np.swapaxes(M, 1, 2))), want[None], tag + " eigenvalues", scale=want.max())
        elif cl == R2:      # the sign fix on a zero singular value: exact(+1) or exact(-1), the same one as the oracle's
            A = case.alt[blk, rule]
            for i, Mi in zip(mem, M):
                assert np.isfinite(Mi).all(), "%s: %s: not finite" % (name, tag)
                s = 1 if np.abs(Mi - E).max() <= np.abs(Mi - A).max() else -1
                close(Mi, E if s > 0 else A, tag + " sign %+d" % s)
                signs[s] += 1
                if ref is not None:
                    so = 1 if np.abs(ref[i] - E).max() <= np.abs(ref[i] - A).max() else -1
                    assert s == so, "%s: %s: point %d has sign %+d, the oracle %+d" % (name, tag, i, s, so)
        elif cl in (R1, N1):
            assert np.isfinite(M).all(), "%s: %s: not finite" % (name, tag)
            d = case.dvec[blk]
            close(M @ d, (case.vtop[blk, rule] * d)[None], tag + " C d = v(lambda_1) d", scale=max(np.abs(M).max(), abs(case.vtop[blk, rule])))
            if rule == PLANE:
                sv = np.linalg.svd(M, compute_uv=False)
                close(sv, np.where(sv > 0.5, 1.0, EPS), tag + " singular values", scale=1.0)
        else:               # R0 under NORMALIZED_MIN_EIG, PLANE_S: 0 / 0 — NaN exactly where the oracle has it
            assert cl == R0
            if ref is not None:
                assert np.array_equal(np.isnan(M), np.isnan(ref[mem])), "%s: %s: NaN pattern differs from the oracle's:\n%s\n%s" % (name, tag, M[0], ref[mem][0])
    assert not fails, "\n".join(fails[:12] + ["(%d comparisons over the bar)" % len(fails)])
    return worst, signs
