"""The CPU statement of the loop closure's ICP (include/rolo_hip.h, "loop-closure ICP"): pcl::IterativeClosestPoint as reference src/backMapping.cpp:2339-2354
configures it (SVD estimation, no rejectors, no RANSAC) and getFitnessScore, in numpy.

PCL is not in the reference tree and cannot be built for the tests, so THIS twin is the parity target of tests/test_gpu_loopicp.py, written from the statement in
the header and not from the HIP unit: parity with a PCL build is unpinned. The association is a brute force in float32 with the statement's expression order
(dx = source - target, d2 = ((dx dx) + (dy dy)) + (dz dz), the first minimum = the smallest target index); the sums are numpy's fp64 sums (their order is not the
device's: they agree to the fp64 summation bound, not bit for bit); the SVD is numpy's."""
import numpy as np

f32, f64 = np.float32, np.float64

NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)
DEFAULTS = dict(max_iterations=100, transformation_epsilon=1e-6, euclidean_fitness_epsilon=1e-6, rotation_epsilon=0.0, max_correspondence_distance=np.inf,
                min_correspondences=3)   # :2342-2346; the cap is the caller's


def transform(T, xyz):
    """rows T0 x + (T1 y + (T2 z + T3)) in float32"""
    T = np.asarray(T, f32).reshape(4, 4)
    p = np.asarray(xyz, f32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([T[r, 0] * x + (T[r, 1] * y + (T[r, 2] * z + T[r, 3])) for r in range(3)], axis=1).astype(f32)


def matmul4(a, b):
    """a b in float32, each entry a0 b0 + a1 b1 + a2 b2 + a3 b3 left to right"""
    a, b = np.asarray(a, f32).reshape(4, 4), np.asarray(b, f32).reshape(4, 4)
    o = np.zeros((4, 4), f32)
    for i in range(4):
        for j in range(4):
            x = a[i, 0] * b[0, j]
            for k in range(1, 4):
                x = f32(x + a[i, k] * b[k, j])
            o[i, j] = x
    return o


def associate(src, tgt, max_dist=np.inf, chunk=256):
    """per source point (n x 3 float32) the nearest target point: (index int32, d2 float32); -1 / inf where (double)d2 > max_dist^2"""
    src, tgt = np.asarray(src, f32)[:, :3], np.asarray(tgt, f32)[:, :3]
    idx = np.zeros(len(src), np.int32); d2 = np.zeros(len(src), f32)
    for a in range(0, len(src), chunk):
        s = src[a:a + chunk]
        dx = s[:, None, 0] - tgt[None, :, 0]; dy = s[:, None, 1] - tgt[None, :, 1]; dz = s[:, None, 2] - tgt[None, :, 2]
        d = ((dx * dx) + (dy * dy)) + (dz * dz)
        assert d.dtype == f32
        k = np.argmin(d, axis=1)   # the first minimum: the smallest index
        idx[a:a + chunk] = k; d2[a:a + chunk] = d[np.arange(len(s)), k]
    cap2 = f64(max_dist) * f64(max_dist)
    drop = ~(d2.astype(f64) <= cap2)
    idx[drop] = -1; d2[drop] = np.inf
    return idx, d2


def pair_terms(src, tgt, idx, d2):
    """the 17 columns whose sums the device forms, one row per kept pair (fp64): 1, d2, p, q, p q^T row-major"""
    keep = idx >= 0
    p = np.asarray(src, f32)[keep, :3].astype(f64); q = np.asarray(tgt, f32)[idx[keep], :3].astype(f64)
    return np.concatenate([np.ones((len(p), 1)), d2[keep].astype(f64)[:, None], p, q, (p[:, :, None] * q[:, None, :]).reshape(len(p), 9)], axis=1)


def umeyama(sums):
    """the 17 sums -> (R, t) in double with q ~ R p + t: Sigma = sum q p^T / n - mean(q) mean(p)^T = U S V^T, R = U diag(1, 1, s) V^T, s = -1 when det U det V < 0"""
    n = sums[0]
    mp, mq = sums[2:5] / n, sums[5:8] / n
    sigma = sums[8:17].reshape(3, 3).T / n - np.outer(mq, mp)
    U, S, Vt = np.linalg.svd(sigma)
    s = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0
    R = U @ np.diag([1.0, 1.0, s]) @ Vt
    return R, mq - R @ mp


def icp(source, target, guess=None, **kw):
    """-> dict(T float32 4 x 4, fitness, converged, iterations, state, n_last, trace = [dict(n, mse, sums, increment)], margin).
    margin: the smallest relative distance, over all iterations, between a quantity that decided an exit test and its threshold (a test with two conditions
    counts its clearly failing condition, or the nearer of its two passing ones): inputs with a margin above 1e-3 leave no exit decision to rounding."""
    P = dict(DEFAULTS); P.update(kw)
    src, tgt = np.asarray(source, f32)[:, :3], np.asarray(target, f32)[:, :3]
    T = np.eye(4, dtype=f32) if guess is None else np.asarray(guess, f32).reshape(4, 4).copy()
    cur = src.copy() if guess is None or np.array_equal(T, np.eye(4, dtype=f32)) else transform(T, src)
    out = dict(T=T, fitness=np.finfo(f64).max, converged=False, iterations=0, state=NOT_CONVERGED, n_last=0, trace=[], margin=np.inf)
    if len(src) == 0 or len(tgt) == 0:
        out["state"] = NO_CORRESPONDENCES
        return out
    rot_thr = P["rotation_epsilon"] if P["rotation_epsilon"] > 0 else 1.0 - P["transformation_epsilon"]
    prev = np.finfo(f64).max
    rel = lambda v, thr: abs(v - thr) / abs(thr) if thr != 0 else abs(v)
    while True:
        idx, d2 = associate(cur, tgt, P["max_correspondence_distance"])
        sums = pair_terms(cur, tgt, idx, d2).sum(axis=0)
        n = int(sums[0])
        rec = dict(n=n, mse=sums[1] / n if n else 0.0, sums=sums, increment=np.zeros((4, 4), f32))
        out["trace"].append(rec); out["n_last"] = n
        if n < P["min_correspondences"] or n < 1:
            out["state"] = NO_CORRESPONDENCES
            break
        R, t = umeyama(sums)
        inc = np.eye(4, dtype=f32); inc[:3, :3] = R.astype(f32); inc[:3, 3] = t.astype(f32)
        rec["increment"] = inc
        cur = transform(inc, cur)
        out["T"] = matmul4(inc, out["T"])
        out["iterations"] += 1
        cosa = 0.5 * (f64(inc[0, 0]) + f64(inc[1, 1]) + f64(inc[2, 2]) - 1.0)
        tsq = f64(inc[0, 3]) ** 2 + f64(inc[1, 3]) ** 2 + f64(inc[2, 3]) ** 2
        mse = rec["mse"]
        if out["iterations"] >= P["max_iterations"]:
            out["state"], out["converged"] = ITERATIONS, True
            break
        # the rotation test in its natural quantity, 1 - cos against 1 - rot_thr (cos itself is within 1e-3 of any threshold near 1)
        m_rot = rel(1.0 - cosa, 1.0 - rot_thr)
        m_t = rel(tsq, P["transformation_epsilon"])
        ok_rot, ok_t = cosa >= rot_thr, tsq <= P["transformation_epsilon"]
        if ok_rot and ok_t:
            out["margin"] = min(out["margin"], m_rot, m_t)
            out["state"], out["converged"] = TRANSFORM, True
            break
        out["margin"] = min(out["margin"], max(m_rot if not ok_rot else 0.0, m_t if not ok_t else 0.0))
        out["margin"] = min(out["margin"], rel(mse, 1e-12))
        if mse < 1e-12:
            out["state"], out["converged"] = ABS_MSE, True
            break
        r = abs(mse - prev) / prev
        out["margin"] = min(out["margin"], rel(r, P["euclidean_fitness_epsilon"]))
        if r < P["euclidean_fitness_epsilon"]:
            out["state"], out["converged"] = REL_MSE, True
            break
        prev = mse
    idx, d2 = associate(cur, tgt, np.inf)
    sums = pair_terms(cur, tgt, idx, d2).sum(axis=0)
    out["trace"].append(dict(n=int(sums[0]), mse=sums[1] / sums[0], sums=sums, increment=np.zeros((4, 4), f32)))
    out["fitness"] = sums[1] / sums[0]
    out["final_cloud"] = cur
    return out


def detect_loop_distance(xyz, times, time_cur, search_radius, time_diff):
    """detectLoopClosureDistance (:2481-2515) without its container test: hits of the radius search around the last pose (squared float distance below radius^2,
    ascending by (distance, index)); the first one with |time - time_cur| > time_diff, or -1 (none, or the last key itself)"""
    xyz = np.asarray(xyz, f32).reshape(-1, 3); times = np.asarray(times, f64).reshape(-1)
    n = len(xyz)
    if n == 0:
        return -1
    d = xyz - xyz[-1]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).astype(f32)
    r2 = f32(search_radius) * f32(search_radius)
    hits = sorted((float(d2[i]), i) for i in range(n) if d2[i] < r2)
    for _, i in hits:
        if abs(times[i] - time_cur) > time_diff:
            return -1 if i == n - 1 else i
    return -1


def rot_angle(R):
    """angle of a rotation matrix, stable near zero"""
    R = np.asarray(R, f64)
    return 2.0 * np.arcsin(min(1.0, np.linalg.norm(R - np.eye(3)) / (2.0 * np.sqrt(2.0))))
