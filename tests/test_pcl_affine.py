"""CPU: the pcl / Eigen pose rules of the host drivers (rolo_amd/csrc/pcl_affine.hpp) against statements that do not include the header, bit for bit.

  aff_of_xyzrpy, its back-end-order and pointer forms, xyzrpy_of     the oracle's orc_get_transformation / orc_get_translation_and_euler (oracle/pyorc.py)
  pcl_rows_of_xyzrpy<double>                                          the same formula in Python floats on the widened values, math.cos / math.sin
  aff_inverse then aff_mul_padded (the odometry increment)            the oracle's orc_odom_increment
  aff_inverse, aff_mul, aff_mul_padded one at a time                  numpy float32 below, one rounded operation per line of arithmetic, in the order written
  aff_mul                                                             also tests/mapper_twin.py's float64 product, within the bound that twin derives

tests/cpp/pcl_affine_test.cpp is compiled with g++ alone (no HIP) and answers every request as hex bit patterns."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import pyorc
import mapper_twin as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEG0 = 0x80000000
IDENTITY = np.eye(4, dtype=F).reshape(16)


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pcl_affine") / "pcl_affine_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rolo_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "pcl_affine_test.cpp"), "-o", exe], check=True)

    def ask(requests):
        """requests: (op, float32 values) -> per request the answer's words as ints, one list per answered line"""
        text = "".join(op + " " + " ".join("%08x" % b for b in bits(v)) + "\n" for op, v in requests)
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr
        lines = [[int(w, 16) for w in line.split()] for line in r.stdout.splitlines()]
        per = [2 if op == "X" else 1 for op, _ in requests]
        assert len(lines) == sum(per)
        out, k = [], 0
        for n in per:
            out.append(lines[k:k + n]); k += n
        return out
    return ask


def bits(v):
    return [int(b) for b in np.ascontiguousarray(v, F).reshape(-1).view(np.uint32)]


def bits64(v):
    return [struct.unpack("<Q", struct.pack("<d", x))[0] for x in v]


# ---- the rules in numpy float32: every * + - / below is one float operation, rounded once, evaluated left to right as written ----
def inverse32(T):
    """Eigen::Transform<float, 3, Affine>::inverse(): cofactors of the linear part over the determinant, translation -(L^-1 t)"""
    a = np.asarray(T, F).reshape(16)
    c = [a[5] * a[10] - a[6] * a[9], a[2] * a[9] - a[1] * a[10], a[1] * a[6] - a[2] * a[5],
         a[6] * a[8] - a[4] * a[10], a[0] * a[10] - a[2] * a[8], a[2] * a[4] - a[0] * a[6],
         a[4] * a[9] - a[5] * a[8], a[1] * a[8] - a[0] * a[9], a[0] * a[5] - a[1] * a[4]]
    det = (a[0] * c[0] + a[1] * c[3]) + a[2] * c[6]
    inv = F(1.0) / det
    o = np.zeros(16, F)
    for i in range(3):
        for j in range(3):
            o[i * 4 + j] = c[i * 3 + j] * inv
    for i in range(3):
        o[i * 4 + 3] = -((o[i * 4] * a[3] + o[i * 4 + 1] * a[7]) + o[i * 4 + 2] * a[11])
    o[15] = F(1.0)
    return o


def mul32(A, B):
    """the affine product: three terms left to right, the translation column adds a's translation last; last row 0 0 0 1"""
    a, b = np.asarray(A, F).reshape(16), np.asarray(B, F).reshape(16)
    c = np.zeros(16, F)
    for i in range(3):
        for j in range(3):
            c[i * 4 + j] = (a[i * 4] * b[j] + a[i * 4 + 1] * b[4 + j]) + a[i * 4 + 2] * b[8 + j]
        c[i * 4 + 3] = ((a[i * 4] * b[3] + a[i * 4 + 1] * b[7]) + a[i * 4 + 2] * b[11]) + a[i * 4 + 3]
    c[15] = F(1.0)
    return c


def mul_padded32(A, B):
    """the 4 x 4 product: every entry is 0 + four terms (the oracle's mat4f_mul)"""
    a, b = np.asarray(A, F).reshape(16), np.asarray(B, F).reshape(16)
    c = np.zeros(16, F)
    for i in range(4):
        for j in range(4):
            s = F(0.0)
            for k in range(4):
                s = s + a[i * 4 + k] * b[k * 4 + j]
            c[i * 4 + j] = s
    return c


def rows_f64(pose):
    """pcl::getTransformation's formula in double on the widened floats, rows 0..2"""
    x, y, z, roll, pitch, yaw = (float(v) for v in pose)
    A, B, C, D, E, Fs = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    DE, DF = D * E, D * Fs
    return [A * C, A * DF - B * E, B * Fs + A * DE, x, B * C, A * E + B * DF, B * DE - A * Fs, y, -D, C * Fs, C * E, z]


# ---- the cases ----
def random_poses(rng, n):
    p = np.empty((n, 6), F)
    p[:, :3] = rng.uniform(-1e3, 1e3, (n, 3))
    p[:, 3:] = rng.uniform(-math.pi, math.pi, (n, 3))
    return p


def poses():
    rng = np.random.default_rng(20261021)
    out = [random_poses(rng, 300), np.zeros((1, 6), F)]
    for k in (3, 4, 5):                     # exactly one zero angle, of either sign
        for zero in (F(0.0), F(-0.0)):
            p = random_poses(rng, 4)
            p[:, k] = zero
            out.append(p)
    for half_pi in (F(math.pi / 2), F(-math.pi / 2)):   # pitch at +-pi/2 rounded to float
        p = random_poses(rng, 4)
        p[:, 4] = half_pi
        p[3, 3] = p[3, 5] = F(0.0)
        out.append(p)
    return np.concatenate(out)


POSES = poses()


def oracle_T(pose):
    return pyorc.get_transformation(*[float(v) for v in pose])


def test_euler_to_matrix_and_back(ask):
    assert bits(oracle_T(POSES[300]))[8] == NEG0   # the all-zero pose: m[8] = -sin(0) = -0
    for pose, (words, dwords) in zip(POSES, ask([("X", p) for p in POSES])):
        T = oracle_T(pose)
        assert words[:16] == bits(T), pose                                        # aff_of_xyzrpy
        assert words[16:22] == bits(pyorc.get_translation_and_euler(T)), pose     # xyzrpy_of
        assert words[22:38] == bits(T), pose                                      # aff_of_rpyxyz
        assert words[38:50] == bits(T[:12]), pose                                 # pcl_rows_of_rpyxyz
        assert len(words) == 50 and dwords == bits64(rows_f64(pose)), pose        # pcl_rows_of_xyzrpy<double>


def test_matrix_to_euler_off_the_rotation_group(ask):
    """products and inverses of poses are rotations only to rounding: xyzrpy_of on them is what the drivers publish"""
    Ms = [mul32(oracle_T(POSES[i]), oracle_T(POSES[i + 1])) for i in range(0, 100, 2)] + [inverse32(oracle_T(POSES[i])) for i in range(100, 120)] + [IDENTITY]
    for M, (words,) in zip(Ms, ask([("E", M) for M in Ms])):
        assert words == bits(pyorc.get_translation_and_euler(M))


def test_odometry_increment(ask):
    """aff_inverse then aff_mul_padded then xyzrpy_of, against the oracle's orc_odom_increment"""
    pairs = [(POSES[i], POSES[i + 1]) for i in range(0, len(POSES) - 1)] + [(POSES[300], POSES[300]), (POSES[7], POSES[7])]
    for (f, b), (words,) in zip(pairs, ask([("D", np.concatenate([f, b])) for f, b in pairs])):
        assert words == bits(pyorc.odom_increment(f, b)), (f, b)


def test_inverse(ask):
    Ts = [oracle_T(p) for p in POSES] + [IDENTITY]
    for T, (words,) in zip(Ts, ask([("I", T) for T in Ts])):
        assert words == bits(inverse32(T))
    # an inverse whose translation comes out -0: -(1 * 0 + 0 * 0 + 0 * 0)
    (words,), (ident,) = ask([("I", IDENTITY), ("1", [])])
    assert ident == bits(IDENTITY)
    assert [words[3], words[7], words[11]] == [NEG0, NEG0, NEG0] and words == bits(inverse32(IDENTITY))


def product_pairs():
    Ts = [oracle_T(p) for p in POSES]
    pairs = [(Ts[i], Ts[i + 1]) for i in range(len(Ts) - 1)]
    pairs += [(IDENTITY, T) for T in Ts[:20] + Ts[300:]] + [(T, IDENTITY) for T in Ts[:20] + Ts[300:]]   # identity times a pose, a pose times identity
    pairs += [(T, inverse32(T)) for T in Ts] + [(inverse32(T), T) for T in Ts[:20]]                       # a pose times its own inverse
    return pairs


def test_products(ask):
    pairs = product_pairs()
    got_m = ask([("M", np.concatenate([a, b])) for a, b in pairs])
    got_p = ask([("P", np.concatenate([a, b])) for a, b in pairs])
    for (a, b), (m,), (p,) in zip(pairs, got_m, got_p):
        assert m == bits(mul32(a, b))
        assert p == bits(mul_padded32(a, b))
        # tests/mapper_twin.py's product in float64 on the widened entries (which carry no error: dR = dt = 0 going in), within its derived bound
        want = tw.mul(tw.aff_read(a[:12]), tw.aff_read(b[:12]))
        got = np.array(m, np.uint32).view(F).astype(np.float64).reshape(4, 4)
        assert np.abs(got[:3, :3] - want.R).max() <= tw.SLACK * want.dR
        assert np.abs(got[:3, 3] - want.t).max() <= tw.SLACK * want.dt
        assert m[12:] == bits([0, 0, 0, 1])


def test_the_two_products_are_two_functions(ask):
    """why both are kept: constructed pairs (not rotations) on which aff_mul and aff_mul_padded give different bits"""
    # sign of zero: every term of c[0] is (-1) * 0 = -0. (-0) + (-0) + (-0) = -0, but 0 + (-0) + ... = +0
    a = IDENTITY.copy(); a[0:3] = F(-1.0)
    b = IDENTITY.copy(); b[0] = b[5] = b[10] = F(0.0)
    # not finite: the padded form's fourth term of a linear entry is a[i][3] * 0 = inf * 0 = NaN; the affine form never forms it
    c = IDENTITY.copy(); c[3] = F(np.inf)
    (m,), (p,) = ask([("M", np.concatenate([a, b])), ("P", np.concatenate([a, b]))])
    assert m == bits(mul32(a, b)) and p == bits(mul_padded32(a, b))
    assert m[0] == NEG0 and p[0] == 0 and m != p
    (m,), (p,) = ask([("M", np.concatenate([c, IDENTITY])), ("P", np.concatenate([c, IDENTITY]))])
    with np.errstate(invalid="ignore"):
        want_m, want_p = mul32(c, IDENTITY), mul_padded32(c, IDENTITY)
    got_p = np.array(p, np.uint32).view(F)
    assert m == bits(want_m) and m[0] == bits([1.0])[0]
    assert np.array_equal(np.isnan(got_p), np.isnan(want_p)) and np.isnan(got_p[0]) and m != p
    assert [w for w, n in zip(p, np.isnan(want_p)) if not n] == [w for w, n in zip(bits(want_p), np.isnan(want_p)) if not n]
