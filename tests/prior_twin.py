"""The ground prior stated in numpy: the ground model's x-y queries and patch cut, FitLocalSurface, AverageHeightAt and the terrain pose solver, as
include/rolo_hip.h ("the ground prior") words them after the reference's src/prior_pose/pose_solver.cpp and prior_pose_node.cpp:164-233. The device kernels
(rolo_amd/csrc/groundprior.hip) are judged against this file; tests/test_prior_twin.py holds this file to closed forms and to its own second routes.

Searches are brute force over all points. Float work is numpy float32, double work plain Python floats (IEEE doubles with correctly rounded sqrt and division),
and every sum over neighbours or wheels is serial in the stated order (np.cumsum's last element; np.sum adds pairwise and gives other bits).

Two steps have two routes each, so that the spread between routes measures what a third implementation may differ by:
  eig   'jacobi' (the cyclic Jacobi the device runs, restated operation by operation) or 'eigh' (numpy.linalg.eigh)
  lin   'lu' (the full-pivot LU with Eigen's rank rule, restated) or 'solve' (numpy.linalg.solve; singular when it raises or returns a non-finite value)
"""
import math

import numpy as np

F = np.float32
MAX_NEIGHBOURS = 4096
FIT_OK, FIT_FEW_HITS, FIT_FEW_INLIERS, FIT_NO_PLANE, FIT_VERTICAL, FIT_OVERFLOW = range(6)
STATUS_OVERFLOW, STATUS_NONFINITE = 1, 2
END_CONVERGED, END_MAX_ITERS = 0, 1
EPS = 2.220446049250313e-16


class Params:
    """rolo_priorpose_params with the values of config/prior_pose_params.yaml"""

    def __init__(self, **kw):
        self.wheel_xy = [(-3.0046, 0.7836), (0.8942, 0.7836), (0.8942, -0.7836), (-3.0046, -0.7836)]
        self.vehicle_com_z = 1.0
        self.body_to_lidar_t = [0.0, 0.0, 1.04]
        self.body_to_lidar_R = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
        self.k_spring, self.g, self.max_iters, self.lm_lambda, self.tol_cost, self.tol_step = 20.0, 1.0, 50, 0.01, 1.0e-12, 1.0e-10
        self.ground_avg_radius, self.ground_min_neighbors = 0.3, 5
        self.fit_radius, self.fit_outlier_factor, self.fit_min_points = 0.6, 3.0, 15
        self.z_min, self.z_max, self.roll_max, self.pitch_max, self.wheel_distance_max = -8.0, 8.0, 0.5, 0.5, 0.1
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)

    @staticmethod
    def square(size_xy, **kw):
        """VehicleModel::FromSquare"""
        h = size_xy / 2.0
        return Params(wheel_xy=[(-h, h), (h, h), (h, -h), (-h, -h)], **kw)


def serial_sum(a):
    a = np.asarray(a, np.float64)
    return float(np.cumsum(a)[-1]) if a.size else 0.0


# ---- the queries ---------------------------------------------------------------------------------------------------------------------------------------------
def d2_xy(cloud, qx, qy):
    """(dx dx + dy dy) + 0 in float, per point"""
    c = np.asarray(cloud, np.float32)
    dx = F(qx) - c[:, 0]
    dy = F(qy) - c[:, 1]
    return dx * dx + dy * dy


def nearest_xy(cloud, qx, qy):
    """the smallest (d2, index)"""
    d2 = d2_xy(cloud, qx, qy)
    i = int(np.argmin(d2))   # the first of equal minima
    return i, d2[i]


def radius_xy(cloud, qx, qy, radius):
    """indices and d2 of { d2 < (float)(r r) } in ascending (d2, index)"""
    d2 = d2_xy(cloud, qx, qy)
    r2 = F(float(radius) * float(radius))
    idx = np.nonzero(d2 < r2)[0]
    order = np.lexsort((idx, d2[idx]))
    return idx[order].astype(np.int32), d2[idx][order]


def extract_patch(cloud, cx, cy, size, T=None):
    """ExtractPatch (two PassThrough passes), then pcl::transformPointCloud in float with T (4 x 4)"""
    c = np.asarray(cloud, np.float32)
    half = float(size) * 0.5
    xlo, xhi, ylo, yhi = F(float(cx) - half), F(float(cx) + half), F(float(cy) - half), F(float(cy) + half)
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(c[:, 0]) & np.isfinite(c[:, 1]) & np.isfinite(c[:, 2]) & ~((c[:, 0] < xlo) | (c[:, 0] > xhi)) & ~((c[:, 1] < ylo) | (c[:, 1] > yhi))
    out = c[keep].copy()
    if T is not None and out.shape[0]:
        T = np.asarray(T, np.float32)
        x, y, z = out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy()
        for r in range(3):
            out[:, r] = T[r, 0] * x + (T[r, 1] * y + (T[r, 2] * z + T[r, 3]))
    return out


# ---- the fit -------------------------------------------------------------------------------------------------------------------------------------------------
def _jacobi_rot(a, v, p, q, r):
    apq = a[p][q]
    if apq == 0.0:
        return
    app, aqq, g = a[p][p], a[q][q], abs(apq)
    if abs(app) + g == abs(app) and abs(aqq) + g == abs(aqq):
        a[p][q] = a[q][p] = 0.0
        return
    theta = (aqq - app) / (2.0 * apq)
    t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    a[p][p] = app - t * apq
    a[q][q] = aqq + t * apq
    a[p][q] = a[q][p] = 0.0
    arp, arq = a[r][p], a[r][q]
    a[r][p] = a[p][r] = c * arp - s * arq
    a[r][q] = a[q][r] = s * arp + c * arq
    for k in range(3):
        vp, vq = v[k][p], v[k][q]
        v[k][p] = c * vp - s * vq
        v[k][q] = s * vp + c * vq


def smallest_eigenvector_jacobi(m6):
    """xx xy xz yy yz zz -> the eigenvector of the smallest eigenvalue, the first of equal ones"""
    a = [[m6[0], m6[1], m6[2]], [m6[1], m6[3], m6[4]], [m6[2], m6[4], m6[5]]]
    v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(30):
        if a[0][1] == 0.0 and a[0][2] == 0.0 and a[1][2] == 0.0:
            break
        _jacobi_rot(a, v, 0, 1, 2)
        _jacobi_rot(a, v, 0, 2, 1)
        _jacobi_rot(a, v, 1, 2, 0)
    c1 = a[1][1] < a[0][0]
    lo = a[1][1] if c1 else a[0][0]
    col = 2 if a[2][2] < lo else (1 if c1 else 0)
    return [v[0][col], v[1][col], v[2][col]]


def smallest_eigenvector_eigh(m6):
    M = np.array([[m6[0], m6[1], m6[2]], [m6[1], m6[3], m6[4]], [m6[2], m6[4], m6[5]]])
    _, vec = np.linalg.eigh(M)
    return [float(vec[0, 0]), float(vec[1, 0]), float(vec[2, 0])]


def fit_points(pts, qx, qy, thr, min_pts, eig="jacobi"):
    """FitLocalSurface after its search, on the neighbours in list order (n x 3 floats, n >= 1) -> (fallback, inliers, z)"""
    x, y, z = (np.asarray(pts[:, k], np.float64) for k in range(3))
    n = z.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        mean = serial_sum(z) / float(n)
        sd = math.sqrt(serial_sum((z - mean) * (z - mean)) / float(n)) if n else 0.0
        lo, hi = mean - thr * sd, mean + thr * sd
        inl = (z >= lo) & (z <= hi)
    m = int(inl.sum())
    if m < min_pts:
        return FIT_FEW_INLIERS, m, 0.0
    if m < 3:
        return FIT_NO_PLANE, m, 0.0
    x, y, z = x[inl], y[inl], z[inl]
    cx, cy, cz = serial_sum(x) / float(m), serial_sum(y) / float(m), serial_sum(z) / float(m)
    dx, dy, dz = x - cx, y - cy, z - cz
    m6 = [serial_sum(dx * dx), serial_sum(dx * dy), serial_sum(dx * dz), serial_sum(dy * dy), serial_sum(dy * dz), serial_sum(dz * dz)]
    nrm = smallest_eigenvector_jacobi(m6) if eig == "jacobi" else smallest_eigenvector_eigh(m6)
    d = -((nrm[0] * cx + nrm[1] * cy) + nrm[2] * cz)
    if abs(nrm[2]) < 1e-6:
        return FIT_VERTICAL, m, 0.0
    return FIT_OK, m, -((nrm[0] * qx + nrm[1] * qy) + d) / nrm[2]


def ground_point(cloud, P, qx, qy, eig="jacobi", cap=MAX_NEIGHBOURS):
    """the ground point under a double query as ComputeResidualAndJacobian takes it -> dict(hits, inliers, fallback, nearest, point)"""
    c = np.asarray(cloud, np.float32)
    idx, _ = radius_xy(c, qx, qy, P.fit_radius)
    hits, inliers, z = int(idx.shape[0]), 0, 0.0
    if hits > cap:
        fb = FIT_OVERFLOW
    elif hits < P.fit_min_points:
        fb = FIT_FEW_HITS
    elif hits == 0:
        fb = FIT_NO_PLANE
    else:
        fb, inliers, z = fit_points(c[idx, :3], float(qx), float(qy), P.fit_outlier_factor, P.fit_min_points, eig)
    if fb == FIT_OK:
        return dict(hits=hits, inliers=inliers, fallback=fb, nearest=-1, point=[float(qx), float(qy), z])
    i, _ = nearest_xy(c, qx, qy)
    return dict(hits=hits, inliers=inliers, fallback=fb, nearest=i, point=[float(c[i, 0]), float(c[i, 1]), float(c[i, 2])])


def average_height_at(cloud, P, qx, qy, cap=MAX_NEIGHBOURS):
    """AverageHeightAt -> (height, status bits)"""
    c = np.asarray(cloud, np.float32)
    i, _ = nearest_xy(c, qx, qy)
    if not P.ground_avg_radius > 0.0:
        return float(c[i, 2]), 0
    idx, _ = radius_xy(c, c[i, 0], c[i, 1], P.ground_avg_radius)
    hits = idx.shape[0]
    if hits <= 0 or hits < P.ground_min_neighbors or hits > cap:
        return float(c[i, 2]), (STATUS_OVERFLOW if hits > cap else 0)
    return serial_sum(c[idx, 2]) / float(hits), 0


# ---- the solver ----------------------------------------------------------------------------------------------------------------------------------------------
def mul33(a, b):
    return [[(a[i][0] * b[0][j] + a[i][1] * b[1][j]) + a[i][2] * b[2][j] for j in range(3)] for i in range(3)]


def rotx(a):
    c, s = math.cos(a), math.sin(a)
    return [[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]]


def roty(a):
    c, s = math.cos(a), math.sin(a)
    return [[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]


def rotz(a):
    c, s = math.cos(a), math.sin(a)
    return [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]


def mulv(R, b):
    return [(R[i][0] * b[0] + R[i][1] * b[1]) + R[i][2] * b[2] for i in range(3)]


def lu3_solve(A, b):
    """Eigen::FullPivLU<Matrix3d>(A).solve(b), None when A is not invertible by its rank rule (a pivot counts if |p| > 3 eps |p_max|)"""
    a = [list(r) for r in A]
    c = list(b)
    col = [0, 1, 2]
    maxpivot = 0.0
    for k in range(3):
        big, pr, pc = -1.0, k, k
        for j in range(k, 3):        # column by column, the first of equals
            for i in range(k, 3):
                if abs(a[i][j]) > big:
                    big, pr, pc = abs(a[i][j]), i, j
        if big == 0.0 or not big >= 0.0:
            return None
        maxpivot = max(maxpivot, big)
        a[k], a[pr] = a[pr], a[k]
        c[k], c[pr] = c[pr], c[k]
        for i in range(3):
            a[i][k], a[i][pc] = a[i][pc], a[i][k]
        col[k], col[pc] = col[pc], col[k]
        for i in range(k + 1, 3):
            l = a[i][k] / a[k][k]
            a[i][k] = l
            for j in range(k + 1, 3):
                a[i][j] -= l * a[k][j]
            c[i] -= l * c[k]
    thr = 3.0 * EPS * maxpivot
    if not (abs(a[0][0]) > thr and abs(a[1][1]) > thr and abs(a[2][2]) > thr):
        return None
    y2 = c[2] / a[2][2]
    y1 = (c[1] - a[1][2] * y2) / a[1][1]
    y0 = ((c[0] - a[0][1] * y1) - a[0][2] * y2) / a[0][0]
    x = [0.0, 0.0, 0.0]
    x[col[0]], x[col[1]], x[col[2]] = y0, y1, y2
    return x


def np_solve(A, b):
    try:
        x = np.linalg.solve(np.array(A), np.array(b))
    except np.linalg.LinAlgError:
        return None
    return [float(v) for v in x] if np.all(np.isfinite(x)) else None


def wheel_points(P, R, x, y, z):
    out = []
    for wx, wy in P.wheel_xy:
        r = mulv(R, [wx, wy, -P.vehicle_com_z])
        out.append([r[0] + x, r[1] + y, r[2] + z])
    return out


def residual_jacobian(P, R, pw, pn):
    """ComputeResidualAndJacobian given the wheels' world points and their ground points -> (residual[3], J[3][3])"""
    n = [R[0][2], R[1][2], R[2][2]]
    f, fz, fr, fp = [], [], [], []
    for (wx, wy), p, gpt in zip(P.wheel_xy, pw, pn):
        a = [p[0] - gpt[0], p[1] - gpt[1], p[2] - gpt[2]]
        d = (a[0] * n[0] + a[1] * n[1]) + a[2] * n[2]
        active = d < 0.0
        rp = mulv(R, [wx, wy, -P.vehicle_com_z])
        dd_dz = (0.0 * n[0] + 0.0 * n[1]) + 1.0 * n[2]
        dd_dr = ((0.0 * n[0] + (-rp[2]) * n[1]) + rp[1] * n[2]) + ((a[0] * 0.0 + a[1] * (-n[2])) + a[2] * n[1])
        dd_dp = ((rp[2] * n[0] + 0.0 * n[1]) + (-rp[0]) * n[2]) + ((a[0] * n[2] + a[1] * 0.0) + a[2] * (-n[0]))
        f.append(P.k_spring * d if active else 0.0)
        fz.append(P.k_spring * dd_dz if active else 0.0)
        fr.append(P.k_spring * dd_dr if active else 0.0)
        fp.append(P.k_spring * dd_dp if active else 0.0)
    rows = [[1.0 for _ in P.wheel_xy], [wy for _, wy in P.wheel_xy], [-wx for wx, _ in P.wheel_xy]]

    def through(v):
        return [serial_sum([rows[i][w] * v[w] for w in range(len(v))]) for i in range(3)]
    r = through(f)
    res = [r[0] + P.g * ((n[0] * 0.0 + n[1] * 0.0) + n[2] * 1.0), r[1] + P.g * 0.0, r[2] + P.g * 0.0]
    cols = [through(fz), through(fr), through(fp)]
    J = [[cols[c][i] for c in range(3)] for i in range(3)]
    J[0][1] += P.g * n[1]
    J[0][2] += P.g * (-n[0])
    return res, J


def get_rpy(m):
    """tf2::Matrix3x3::getRPY"""
    if abs(m[2][0]) >= 1.0:
        return [math.atan2(m[2][1], m[2][2]), 1.5707963267948966 if m[2][0] < 0.0 else -1.5707963267948966, 0.0]
    pitch = -math.asin(m[2][0])
    cp = math.cos(pitch)
    return [math.atan2(m[2][1] / cp, m[2][2] / cp), pitch, math.atan2(m[1][0] / cp, m[0][0] / cp)]


def _finite(vs):
    return all(math.isfinite(v) for p in vs for v in p)


def solve(cloud, P, x, y, yaw, eig="jacobi", lin="lu", cap=MAX_NEIGHBOURS):
    """PoseSolver::Solve -> dict of the result's fields plus `trace`: per iteration (c0, c1, step, last_cost before the test, accepted, singular)"""
    c = np.asarray(cloud, np.float32)
    x, y, yaw = float(x), float(y), float(yaw)
    status = 0
    R = rotz(yaw)
    min_h = math.inf
    for wx, wy in P.wheel_xy:
        w = mulv(R, [wx, wy, -P.vehicle_com_z])
        h, st = average_height_at(c, P, x + w[0], y + w[1], cap)
        status |= st
        min_h = h if h < min_h else min_h
    z = (min_h + P.vehicle_com_z) - 1.0 if math.isfinite(min_h) else 0.0
    last_cost = best_cost = math.inf
    best_R, best_z = R, z
    lam = P.lm_lambda
    end, iterations, trace = END_MAX_ITERS, 0, []

    def ground(pw):
        nonlocal status
        out = []
        for p in pw:
            gp = ground_point(c, P, p[0], p[1], eig, cap)
            if gp["fallback"] == FIT_OVERFLOW:
                status |= STATUS_OVERFLOW
            out.append(gp["point"])
        return out

    for it in range(P.max_iters):
        iterations = it + 1
        pw = wheel_points(P, R, x, y, z)
        if not _finite(pw):
            status |= STATUS_NONFINITE
            break
        res, J = residual_jacobian(P, R, pw, ground(pw))
        c0 = (res[0] * res[0] + res[1] * res[1]) + res[2] * res[2]
        if not math.isfinite(c0):
            status |= STATUS_NONFINITE
            break
        if c0 < best_cost:
            best_cost, best_R, best_z = c0, R, z
        A = [[((J[0][i] * J[0][j] + J[1][i] * J[1][j]) + J[2][i] * J[2][j]) + (lam if i == j else 0.0) for j in range(3)] for i in range(3)]
        b = [-((J[0][i] * res[0] + J[1][i] * res[1]) + J[2][i] * res[2]) for i in range(3)]
        delta = lu3_solve(A, b) if lin == "lu" else np_solve(A, b)
        if delta is None:
            lam *= 10.0
            trace.append((c0, None, None, last_cost, False, True))
            continue
        step = math.sqrt((delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2])
        zt = z + delta[0]
        Rn = mul33(mul33(rotx(delta[1]), roty(delta[2])), R)
        Rt = mul33(rotz(yaw), mul33(rotz(-math.atan2(Rn[1][0], Rn[0][0])), Rn))
        pwt = wheel_points(P, Rt, x, y, zt)
        if not _finite(pwt):
            status |= STATUS_NONFINITE
            break
        rest, _ = residual_jacobian(P, Rt, pwt, ground(pwt))
        c1 = (rest[0] * rest[0] + rest[1] * rest[1]) + rest[2] * rest[2]
        trace.append((c0, c1, step, last_cost, c1 < c0, False))
        if c1 < c0:
            z, R = zt, Rt
            lam = max(lam / 2.0, 1e-8)
            if abs(last_cost - c1) < P.tol_cost and step < P.tol_step:
                end = END_CONVERGED
                break
            last_cost = c1
        else:
            lam *= 5.0
            last_cost = c0
    tilt = mul33(rotz(-yaw), best_R)
    roll, pitch = math.atan2(tilt[2][1], tilt[2][2]), math.atan2(-tilt[2][0], tilt[0][0])
    pw = wheel_points(P, best_R, x, y, best_z)
    n = [best_R[0][2], best_R[1][2], best_R[2][2]]
    dist = []
    if _finite(pw):
        for p in pw:
            i, _ = nearest_xy(c, p[0], p[1])
            dist.append(((p[0] - float(c[i, 0])) * n[0] + (p[1] - float(c[i, 1])) * n[1]) + (p[2] - float(c[i, 2])) * n[2])
    else:
        status |= STATUS_NONFINITE
        dist = [0.0] * len(pw)
    ok = status == 0 and end == END_CONVERGED and not (best_z < P.z_min or best_z > P.z_max) and not (abs(roll) > P.roll_max or abs(pitch) > P.pitch_max) \
        and not any(abs(d) > P.wheel_distance_max for d in dist)
    Rwb = mul33(rotz(yaw), mul33(roty(pitch), rotx(roll)))
    Rbl = [list(P.body_to_lidar_R[0:3]), list(P.body_to_lidar_R[3:6]), list(P.body_to_lidar_R[6:9])]
    t = mulv(Rwb, list(P.body_to_lidar_t))
    lidar = [t[0] + x, t[1] + y, t[2] + best_z] + get_rpy(mul33(Rwb, Rbl))
    return dict(z=best_z, roll=roll, pitch=pitch, R=np.array(best_R), cost=best_cost, wheel_distance=np.array(dist), lidar_pose=np.array(lidar),
                iterations=iterations, end_reason=end, success=bool(ok), status=status, trace=trace)


def decisive(result, P, factor=10.0):
    """True when the discrete outcome (end reason, iteration count) of `result` sits a factor away from every threshold that decided it, at the last iteration
    and at the one before it: the trial cost against the cost (accept is c1 < c0), and for an accepted trial |last_cost - c1| against tol_cost and the step
    against tol_step. A singular step is never decisive"""
    for c0, c1, step, last, accepted, singular in result["trace"][-2:]:
        if singular:
            return False
        if not (c1 < c0 / factor or c1 > c0 * factor):
            return False
        if accepted:
            for v, tol in ((abs(last - c1), P.tol_cost), (step, P.tol_step)):
                if not (v < tol / factor or v > tol * factor):
                    return False
    return True
