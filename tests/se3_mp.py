"""SE(3) Exp and Log and the Cauchy loss in mpmath at 60 digits, written from the mathematics: the reference that the numpy statement tests/pgo_twin.py and the
device code (rolo_amd/csrc/posegraph.hip) are both held to, and that shares no line with either.

Tangent order [omega, v], poses (R, t), as include/rolo_hip.h states them. No series and no thresholds: at 60 digits the closed forms keep more than 30 digits
down to an angle of 1e-12, and only the angle that is exactly zero takes its limit. The angle of Log is atan2(|w|, (tr R - 1) / 2) with w the vector of the
antisymmetric part, defined for every matrix, so a rotation that is orthogonal only to fp64 rounding has one Log here and in the statement. The translation of
Log is the solution of V u = t with V = I + B W + C W^2, not a formula for V^-1. Every function takes fp64 (or mpmath) numbers and returns mpmath ones;
`floats` brings a result back."""
import mpmath as mp
import numpy as np

DIGITS = 60


def _ctx():
    return mp.workdps(DIGITS)


def vec(a):
    if isinstance(a, mp.matrix):
        return a
    return mp.matrix([mp.mpf(float(x)) if not isinstance(x, mp.mpf) else x for x in (a.reshape(-1) if isinstance(a, np.ndarray) else list(a))])


def mat3(R):
    if isinstance(R, mp.matrix):
        return R
    R = np.asarray(R, np.float64).reshape(3, 3)
    return mp.matrix([[mp.mpf(float(R[r, c])) for c in range(3)] for r in range(3)])


def floats(a):
    """an mpmath vector or matrix as a numpy array of doubles (vectors come back one-dimensional)"""
    out = np.array([[float(a[r, c]) for c in range(a.cols)] for r in range(a.rows)], np.float64)
    return out.reshape(-1) if a.cols == 1 else out


def hat(w):
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def _BC(th):
    """(1 - cos th) / th^2 and (th - sin th) / th^3"""
    if th == 0:
        return mp.mpf(1) / 2, mp.mpf(1) / 6
    return (1 - mp.cos(th)) / th ** 2, (th - mp.sin(th)) / th ** 3


def exp_se3(xi):
    """Exp([omega, v]) = (I + sin th / th W + (1 - cos th) / th^2 W^2, V v), W = hat(omega), th = |omega|"""
    with _ctx():
        xi = vec(xi)
        w, v = xi[:3], xi[3:]
        th = mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
        A = mp.sin(th) / th if th != 0 else mp.mpf(1)
        B, C = _BC(th)
        W = hat(w)
        W2 = W * W
        return mp.eye(3) + A * W + B * W2, (mp.eye(3) + B * W + C * W2) * v


def log_so3(R):
    with _ctx():
        R = mat3(R)
        w = mp.matrix([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2
        s = mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
        c = (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2
        if s == 0:
            assert c > 0, "a half turn has no unique Log"
            return w
        return w * (mp.atan2(s, c) / s)


def log_se3(R, t):
    """-> the 6-vector [omega, u] with Exp of it equal to (R, t)"""
    with _ctx():
        w = log_so3(R)
        th = mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
        B, C = _BC(th)
        W = hat(w)
        u = mp.lu_solve(mp.eye(3) + B * W + C * (W * W), vec(t))
        return mp.matrix([w[0], w[1], w[2], u[0], u[1], u[2]])


def mul(a, b):
    with _ctx():
        Ra, Rb = mat3(a[0]), mat3(b[0])
        return Ra * Rb, Ra * vec(b[1]) + vec(a[1])


def inv(a):
    with _ctx():
        Rt = mat3(a[0]).T
        return Rt, -(Rt * vec(a[1]))


def whitened_r2(e, var6):
    """|e / sigma|^2 of an error 6-vector under the variances var6"""
    with _ctx():
        return sum((e[k] ** 2 / mp.mpf(float(var6[k])) for k in range(6)), mp.mpf(0))


def cauchy(r2, k):
    """mEstimator::Cauchy at squared distance r2 -> rho = k^2 / 2 log(1 + r2 / k^2), w = k^2 / (k^2 + r2)"""
    with _ctx():
        k2 = mp.mpf(float(k)) ** 2
        r2 = mp.mpf(r2)
        return k2 / 2 * mp.log(1 + r2 / k2), k2 / (k2 + r2)


def rotation_angle(Ra, Rb):
    """the angle of Ra^T Rb"""
    with _ctx():
        w = log_so3(mat3(Ra).T * mat3(Rb))
        return mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)


def pose_distance(A, B):
    """largest translation distance (m) and rotation angle (rad) between two pose lists, entries (R, t) in doubles or mpmath numbers; -> doubles"""
    with _ctx():
        dt = dr = mp.mpf(0)
        for (Ra, ta), (Rb, tb) in zip(A, B):
            d = vec(ta) - vec(tb)
            dt = max(dt, mp.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2))
            dr = max(dr, rotation_angle(Ra, Rb))
        return float(dt), float(dr)
