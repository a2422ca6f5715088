"""The mapping node's float pose bookkeeping as a float64 statement, written from the reference lines (src/backMapping.cpp): updateInitialGuess :516-555, saveFrame
:1071-1091 and the incremental pose of publishOdometry :1361-1389, over pcl::getTransformation, pcl::getTranslationAndEulerAngles and Affine3f products / inverse.
The library restates the same lines in float (rolo_amd/csrc/mapper.hip: rolo_mapper_initial_guess / _save_frame / _incremental); tests/test_mapper_twin.py holds it
to this statement within the bound derived here. Poses are transformTobeMapped order (roll, pitch, yaw, x, y, z); an affine is rows 0..2, 3 x 4.

The statement takes the library's float inputs widened, so the inputs carry no error; everything below is the error of the float evaluation.

The bound, from the number of float products and sums and the operand magnitudes. eps = 2^-24: every float product, sum and quotient is within eps |result| of the exact
one. E = 1: glibc documents sinf, cosf, atan2f and asinf at 1 ulp, which is within 2 E eps of a value of magnitude <= 1 (and within 2 E eps |result| in general).
Each affine is carried with dR, the largest error of an entry of its linear part, and dt, the largest error of an entry of its translation.
  pose     pcl::getTransformation. A .. F are within 2 E eps. The worst entry is A * DF - B * E with DF = fl(D * F): DF is within 2 E eps + 2 E eps + eps; A * DF within
           2 E eps + (4 E + 1) eps + eps; B * E within (4 E + 1) eps; the difference (a rotation entry, magnitude <= 1) rounds once more: dR = (10 E + 4) eps. The
           translation is copied: dt = 0. An affine that is read from a float array (lastOdomTransformation, increOdomAffine) has dR = dt = 0.
  product  c_ij = sum_k a_ik b_kj. A row of a and a column of b have 1-norms <= sqrt 3 (rotations), so the operands' errors bring sqrt 3 (dRa + dRb); three products
           and two sums of magnitude <= 1 round: 5 eps. dR = sqrt 3 (dRa + dRb) + 5 eps.
           c_i3 = a_i0 tb_0 + a_i1 tb_1 + a_i2 tb_2 + ta_i: the operands' errors bring dRa |tb|_1 + sqrt 3 dtb + dta; the three products round to within eps |tb|_1 together,
           the three sums have magnitudes <= |tb|_1, |tb|_1 and |tb|_1 + |ta|_inf. dt = (dRa + 4 eps) |tb|_1 + eps |ta|_inf + sqrt 3 dtb + dta.
  inverse  Affine3f::inverse(): cofactors over the determinant, then -L^-1 t. A cofactor is a difference of two products of entries: dcof = 4 dRa + 3 eps. The determinant
           is a row times a column of cofactors: ddet = sqrt 3 (dRa + dcof) + 5 eps; it is 1 to within that, so its reciprocal is within ddet + eps and an entry
           cofactor * reciprocal within dR = dcof + ddet + 2 eps. The translation is three products and two sums of magnitude <= |t|_1: dt = (dR + 3 eps) |t|_1 + sqrt 3 dta.
  angles   pcl::getTranslationAndEulerAngles. roll = atan2(m21, m22) and yaw = atan2(m10, m00): an error dR in both arguments moves the angle by at most sqrt 2 dR / h
           with h the hypotenuse of the arguments (= cos pitch); the float atan2f adds 2 E eps pi. pitch = asin(-m20): dR / sqrt(1 - m20^2) + 2 E eps pi / 2. These are
           first-order in dR / h, so a case whose result has |cos pitch| < 0.05 is outside the statement (the generator re-draws it; saveFrame's planted cases sit far
           from it); with dR / h <= 2 x 10^-4 there, the neglected terms are below one part in a thousand.
Every bound is multiplied by 1.001 for the terms of second order (products of two errors, entries of magnitude 1 + 10^-6)."""
import math

import numpy as np

EPS = 2.0 ** -24
E = 1
SLACK = 1.001
SQ3 = math.sqrt(3.0)
MIN_COS_PITCH = 0.05


class Aff:
    """an affine in float64 with the bounds of its float evaluation"""

    def __init__(self, M, dR=0.0, dt=0.0):
        self.M = np.asarray(M, np.float64).reshape(3, 4)
        self.dR, self.dt = float(dR), float(dt)

    R = property(lambda self: self.M[:, :3])
    t = property(lambda self: self.M[:, 3])


def widen(a):
    return [float(np.float32(v)) for v in np.asarray(a).reshape(-1)]


def aff_of_pose(pose6) -> Aff:
    """pcl::getTransformation(x, y, z, roll, pitch, yaw) = trans2Affine3f :339-342"""
    r, p, y, tx, ty, tz = widen(pose6)
    A, B, C, D, Ec, F = math.cos(y), math.sin(y), math.cos(p), math.sin(p), math.cos(r), math.sin(r)
    DE, DF = D * Ec, D * F
    M = [[A * C, A * DF - B * Ec, B * F + A * DE, tx], [B * C, A * Ec + B * DF, B * DE - A * F, ty], [-D, C * F, C * Ec, tz]]
    return Aff(M, (10 * E + 4) * EPS, 0.0)


def aff_read(m12) -> Aff:
    return Aff(widen(m12))


def mul(a: Aff, b: Aff) -> Aff:
    M = np.zeros((3, 4))
    M[:, :3] = a.R @ b.R
    M[:, 3] = a.R @ b.t + a.t
    tb1, tainf = np.abs(b.t).sum(), np.abs(a.t).max()
    return Aff(M, SQ3 * (a.dR + b.dR) + 5 * EPS, (a.dR + 4 * EPS) * tb1 + EPS * tainf + SQ3 * b.dt + a.dt)


def inverse(a: Aff) -> Aff:
    Ri = np.linalg.inv(a.R)
    M = np.zeros((3, 4))
    M[:, :3] = Ri
    M[:, 3] = -(Ri @ a.t)
    dcof = 4 * a.dR + 3 * EPS
    ddet = SQ3 * (a.dR + dcof) + 5 * EPS
    dR = dcof + ddet + 2 * EPS
    return Aff(M, dR, (dR + 3 * EPS) * np.abs(a.t).sum() + SQ3 * a.dt)


def xyzrpy(a: Aff):
    """pcl::getTranslationAndEulerAngles -> (x y z roll pitch yaw, their bounds, cos pitch)"""
    M = a.M
    roll, pitch, yaw = math.atan2(M[2, 1], M[2, 2]), math.asin(max(-1.0, min(1.0, -M[2, 0]))), math.atan2(M[1, 0], M[0, 0])
    cp = math.sqrt(max(0.0, 1.0 - M[2, 0] * M[2, 0]))
    h_r, h_y = math.hypot(M[2, 1], M[2, 2]), math.hypot(M[1, 0], M[0, 0])
    big = float("inf")
    b_roll = math.sqrt(2.0) * a.dR / h_r + 2 * E * EPS * math.pi if h_r > 0 else big
    b_yaw = math.sqrt(2.0) * a.dR / h_y + 2 * E * EPS * math.pi if h_y > 0 else big
    b_pitch = a.dR / cp + E * EPS * math.pi if cp > 0 else big
    val = np.array([M[0, 3], M[1, 3], M[2, 3], roll, pitch, yaw])
    bnd = SLACK * np.array([a.dt, a.dt, a.dt, b_roll, b_pitch, b_yaw])
    return val, bnd, cp


def initial_guess(tf6, have_keyposes, guess6, last_odom12, last_odom_available):
    """updateInitialGuess :516-555 -> dict(tf value / bound in transformTobeMapped order, last (Aff or None: unchanged), available, cos_pitch)"""
    tf = np.array(widen(tf6))
    zero = np.zeros(6)
    if not have_keyposes:   # :524-531
        tf[:3] = 0.0
        return dict(tf=tf, tf_bound=zero, last=None, available=last_odom_available, cos_pitch=1.0)
    if guess6 is None:      # :536 — odomAvailable false
        return dict(tf=tf, tf_bound=zero, last=None, available=last_odom_available, cos_pitch=1.0)
    back = aff_of_pose(guess6)   # :538-539
    if not last_odom_available:  # :540-543
        return dict(tf=tf, tf_bound=zero, last=back, available=True, cos_pitch=1.0)
    incre = mul(inverse(aff_read(last_odom12)), back)   # :545
    final = mul(aff_of_pose(tf6), incre)                # :546-547
    v, b, cp = xyzrpy(final)                            # :548-549
    return dict(tf=np.array([v[3], v[4], v[5], v[0], v[1], v[2]]), tf_bound=np.array([b[3], b[4], b[5], b[0], b[1], b[2]]), last=back, available=True, cos_pitch=cp)


def save_frame(last_keypose6, tf6, dist_thr, angle_thr):
    """saveFrame :1071-1091 -> dict(save, values = (|roll|, |pitch|, |yaw|, distance), bounds, margins = each value's distance from its threshold, margin = the smallest)"""
    if last_keypose6 is None:
        return dict(save=True, values=None, bounds=None, margin=float("inf"))
    between = mul(inverse(aff_of_pose(last_keypose6)), aff_of_pose(tf6))   # :1076-1080
    v, b, cp = xyzrpy(between)
    dist = math.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
    # d = sqrt(x x + y y + z z) in float. The components' errors move d by at most (|x| + |y| + |z|) dt / d <= sqrt 3 dt. The three products are within eps of
    # themselves and the two sums within eps of sums <= d^2: d^2 is within 3 eps d^2, its root within 1.5 eps d, and the root rounds once: 2.5 eps d
    b_dist = SLACK * ((math.sqrt(3.0) * between.dt) + 2.5 * EPS * dist)
    values = np.array([abs(v[3]), abs(v[4]), abs(v[5]), dist])
    bounds = np.array([b[3], b[4], b[5], b_dist])
    thr = np.array([angle_thr, angle_thr, angle_thr, dist_thr], np.float64)
    save = not bool(np.all(values < thr))
    return dict(save=save, values=values, bounds=bounds, margins=np.abs(values - thr), margin=float(np.abs(values - thr).min()), cos_pitch=cp)


def incremental(front6, back6, tf6, started, incre12):
    """publishOdometry :1361-1389 -> dict(incre (Aff), pose value / bound as x y z roll pitch yaw, cos_pitch)"""
    if not started:   # :1365-1369
        inc = aff_of_pose(tf6)
    else:             # :1372-1373
        inc = mul(aff_read(incre12), mul(inverse(aff_of_pose(front6)), aff_of_pose(back6)))
    v, b, cp = xyzrpy(inc)
    return dict(incre=inc, pose=v, pose_bound=b, cos_pitch=cp)


def pose_of(a: Aff):
    """transformTobeMapped order of an affine, float32"""
    v, _, _ = xyzrpy(a)
    return np.array([v[3], v[4], v[5], v[0], v[1], v[2]], np.float32)


def compose(pose6, delta6):
    """the float32 pose of trans2Affine3f(pose6) * trans2Affine3f(delta6): how the tests plant a step of known size behind a pose"""
    return pose_of(mul(aff_of_pose(pose6), aff_of_pose(delta6)))
