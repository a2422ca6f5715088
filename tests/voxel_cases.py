"""Constructed voxels for K6, the target voxel map (rolo_amd/csrc/voxelmap.hip, voxel_dev.hpp): a numpy restatement of the hash table as its comments publish it, clouds whose
points are planted into chosen voxels so that a probe chain crosses the table's end, sits at the key range's edge or fills a workgroup's LDS table exactly, and a plain reference
of the map: exact sums, correctly rounded. No GPU here; tests/test_voxel_cases.py pins every construction through the oracle, tests/test_gpu_voxel_cases.py runs them.

The table: a slot's key is the three voxel coordinates packed 3 x 21 bits with a bias of 2^20; a key's home is the low 32 bits of the splitmix64 finaliser of the packed word,
masked with slots - 1; collisions step to the next slot, (h + 1) & mask; slots = max(1024, the power of two >= 2 * n_target)."""
from fractions import Fraction
import math

import numpy as np

from oracle import pyorc

KEY_BIAS = 1 << 20
KEY_MIN, KEY_MAX = -(1 << 20), (1 << 20) - 1   # the last voxel coordinates pack() accepts
POLAR_RES = (0.175, 0.175, 2.0)                # the production POLAR grid


# ---- the table, restated ---------------------------------------------------------------------------------------------------------------------------
def pack(k3):
    """(..., 3) integer voxel coordinates -> uint64 packed keys; a coordinate outside [-2^20, 2^20) is an error here (ROLO_EKEYRANGE there)"""
    k = np.asarray(k3, np.int64)
    assert k.shape[-1] == 3 and np.all(k >= KEY_MIN) and np.all(k <= KEY_MAX), "voxel coordinate outside the packed key range"
    u = (k + KEY_BIAS).astype(np.uint64)
    return u[..., 0] | (u[..., 1] << np.uint64(21)) | (u[..., 2] << np.uint64(42))


def unpack(key):
    key = np.asarray(key, np.uint64)
    m = np.uint64(0x1fffff)
    return np.stack([(key & m), ((key >> np.uint64(21)) & m), ((key >> np.uint64(42)) & m)], axis=-1).astype(np.int64) - KEY_BIAS


def hash_key(key):
    """splitmix64 finaliser, low 32 bits"""
    k = np.asarray(key, np.uint64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(30); k *= np.uint64(0xbf58476d1ce4e5b9)
        k ^= k >> np.uint64(27); k *= np.uint64(0x94d049bb133111eb)
        k ^= k >> np.uint64(31)
    return (k & np.uint64(0xffffffff)).astype(np.int64)


def mask_of(n_target):
    slots = 1024
    while slots < 2 * n_target:
        slots <<= 1
    return slots - 1


def home(k3, mask):
    return hash_key(pack(k3)) & mask


def occupied(keys, mask):
    """linear probing of the distinct voxels `keys` (m x 3), in the order given -> {slot: (kx, ky, kz)}. WHICH slots end up taken does not depend on the order of the
    inserts (which key sits in which slot of a chain does)."""
    table = {}
    for k in np.unique(np.asarray(keys, np.int64).reshape(-1, 3), axis=0):
        h = int(home(k, mask))
        while h in table:
            h = (h + 1) & mask
        table[h] = tuple(int(v) for v in k)
    return table


def probe_length(k3, table, mask):
    """slots a lookup of voxel k3 reads (hit or miss) and whether its walk crosses from the last slot to slot 0"""
    h = int(home(k3, mask)); n = 1; wrapped = False
    want = tuple(int(v) for v in k3)
    while h in table and table[h] != want:
        wrapped = wrapped or h == mask
        h = (h + 1) & mask; n += 1
    return n, wrapped, (h in table)


# ---- a probe chain across the table's end ----------------------------------------------------------------------------------------------------------
class Chain:
    """voxels: `length` voxels whose homes are the table's last `last` slots, so the chain they form takes the slots mask - last + 1 .. mask and 0 .. length - last - 1;
    ghosts: voxels NOT in the map whose homes lie on the chain — a lookup of one walks through the wrap to the first free slot;
    filler(n): n more voxels whose homes lie in the table's middle half (they lengthen no chain at either end)"""

    def __init__(self, voxels, ghosts, middle, mask, last):
        self.voxels, self.ghosts, self._middle, self.mask, self.last = voxels, ghosts, middle, mask, last

    def filler(self, n):
        assert n <= len(self._middle)
        return self._middle[:n].copy()


def box_candidates(box):
    r = np.arange(-box, box)
    return np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)


def polar_candidates(res=POLAR_RES, r_bins=64):
    """bins of the POLAR grid a point can be planted in: every azimuth bin that lies whole inside [0, 2 pi), polar-angle bins away from the poles, ranges from one bin out"""
    a = np.arange(0, int(math.floor(2 * math.pi / res[0])))
    b = np.arange(2, int(math.floor(math.pi / res[1])) - 1)
    c = np.arange(1, r_bins)
    return np.stack(np.meshgrid(a, b, c, indexing="ij"), axis=-1).reshape(-1, 3)


def chain_at_table_end(n_target, length=12, last=3, box=24, candidates=None, n_ghosts=6):
    mask = mask_of(n_target)
    cand = box_candidates(box) if candidates is None else np.asarray(candidates, np.int64)
    h = home(cand, mask)
    per = -(-length // last)
    picked, spare = [], []
    for s in range(mask - last + 1, mask + 1):
        at = cand[h == s]
        assert len(at) >= per + 1, "too few candidate voxels with home %d" % s
        picked.append(at[:per]); spare.append(at[per:per + 1])
    voxels = np.concatenate([np.stack([p[i] for p in picked if i < len(p)]) for i in range(per)])[:length]
    table = occupied(voxels, mask)
    want = set(range(mask - last + 1, mask + 1)) | set(range(0, length - last))
    assert set(table) == want and 0 in table, "the chain does not spill over the table's end as planned"
    # ghosts: one spare voxel per end slot (the longest walks) and voxels at home in the spilled part
    ghosts = [g[0] for g in spare]
    for s in range(0, length - last):
        at = cand[h == s]
        if len(at) and len(ghosts) < n_ghosts:
            ghosts.append(at[0])
    ghosts = np.asarray(ghosts[:n_ghosts])
    first_free = length - last
    for g in ghosts:
        n, wrapped, hit = probe_length(g, table, mask)
        assert not hit and (int(home(g, mask)) + n - 1) & mask == first_free
    assert all(probe_length(g, table, mask)[1] for g in ghosts[:last])
    middle = cand[(h > mask // 4) & (h < 3 * (mask // 4))]
    # distinct homes among the fillers themselves: each sits in its own home slot, alone
    _, first = np.unique(home(middle, mask), return_index=True)
    middle = middle[np.sort(first)]
    return Chain(voxels, ghosts, middle, mask, last)


# ---- point builders --------------------------------------------------------------------------------------------------------------------------------
def points_in_voxels(voxels, per, leaf, rng, margin=0.05):
    """`per` points inside each UNIFORM voxel, voxel after voxel: voxel k covers [(k + 0.5) leaf, (k + 1.5) leaf) per axis. float32 n x 4 (w = 0)."""
    v = np.repeat(np.asarray(voxels, np.float64).reshape(-1, 3), per, axis=0)
    u = rng.uniform(margin, 1.0 - margin, size=v.shape)
    pts = np.zeros((v.shape[0], 4), np.float32)
    pts[:, :3] = ((v + 0.5 + u) * leaf).astype(np.float32)
    assert np.array_equal(pyorc.voxel_keys(pts, pyorc.VOXEL_UNIFORM, leaf), v.astype(np.int32)), "a point left its voxel"
    return pts


def points_in_polar_bins(keys, res, per, rng, margin=0.1):
    """`per` points inside each bin (azimuth, polar angle, range) of the POLAR grid: bin (a, b, c) covers azimuth + pi in [a, a + 1) res[0], acos(z / r) in [b, b + 1) res[1],
    r in [c, c + 1) res[2]. float32 n x 4 (w = 0)."""
    k = np.repeat(np.asarray(keys, np.float64).reshape(-1, 3), per, axis=0)
    u = rng.uniform(margin, 1.0 - margin, size=k.shape)
    th = (k[:, 0] + u[:, 0]) * res[0] - math.pi; ph = (k[:, 1] + u[:, 1]) * res[1]; r = (k[:, 2] + u[:, 2]) * res[2]
    pts = np.zeros((k.shape[0], 4), np.float32)
    pts[:, 0] = r * np.sin(ph) * np.cos(th); pts[:, 1] = r * np.sin(ph) * np.sin(th); pts[:, 2] = r * np.cos(ph)
    assert np.array_equal(pyorc.voxel_keys(pts, pyorc.VOXEL_POLAR, 1.0, res), k.astype(np.int32)), "a point left its bin"
    return pts


# ---- the reference map -----------------------------------------------------------------------------------------------------------------------------
def _round_div(total, n):
    return float(total / n)   # Fraction -> float is correctly rounded


def exact_map(cloud, keys, covs=None):
    """voxels in lexicographic key order -> (keys V x 3, counts V, means V x 3, covs V x 3 x 3 or None): every mean (and covariance entry) the correctly rounded quotient
    of the EXACT sum of its voxel's float32 coordinates (fp64 entries of `covs`, n x 4 x 4 or n x 3 x 3) by the count"""
    cloud = np.asarray(cloud); keys = np.asarray(keys, np.int64)
    uk, inv = np.unique(keys, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    V = len(uk)
    counts = np.bincount(inv, minlength=V).astype(np.int64)
    means = np.zeros((V, 3)); out_cov = np.zeros((V, 3, 3)) if covs is not None else None
    for v in range(V):
        idx = np.nonzero(inv == v)[0]
        n = int(counts[v])
        for d in range(3):
            means[v, d] = _round_div(sum((Fraction(float(x)) for x in cloud[idx, d]), Fraction(0)), n)
        if covs is not None:
            for a in range(3):
                for b in range(3):   # entry by entry: the oracle's covariances are symmetric only to rounding, the library's and handed-in ones exactly
                    if b < a and np.array_equal(covs[idx, a, b], covs[idx, b, a]):
                        out_cov[v, a, b] = out_cov[v, b, a]
                    else:
                        out_cov[v, a, b] = _round_div(sum((Fraction(float(x)) for x in covs[idx, a, b]), Fraction(0)), n)
    return uk, counts, means, out_cov


def sort_map(k, c, m, v):
    """a map as the library or the oracle hands it out (keys V x 3, counts, means V x 4, covs V x 4 x 4) in exact_map's order and shapes"""
    o = np.lexsort(np.asarray(k).T[::-1])
    return np.asarray(k)[o].astype(np.int64), np.asarray(c)[o].astype(np.int64), np.asarray(m)[o][:, :3], np.asarray(v)[o][:, :3, :3]


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)))


# ---- the fixed-point sums' contract (voxelmap.hip's header, voxel_dev.hpp fix_scales) --------------------------------------------------------------
# The scales are powers of two with n * max|value| * scale < 2^62: bits_n = bit_length(n), max|coordinate| < 2^(e + 1) with e its binary exponent, not below -1.
def _exponent(maxabs):
    return math.frexp(float(np.float32(maxabs)))[1] - 1 if maxabs > 0 else -127


def quantum_pos(n, maxabs):
    """the position sums count in units of this"""
    return 2.0 ** -(62 - int(n).bit_length() - (max(_exponent(maxabs), -1) + 1))


def quantum_cov(n):
    """... and the covariance sums (entries bounded by 1) in units of this"""
    return 2.0 ** -(62 - int(n).bit_length() - 1)


def maxabs(cloud):
    return float(np.abs(np.asarray(cloud)[:, :3]).max())


def lowest_bit(x):
    """value of the lowest set bit of every float (0 for 0)"""
    x = np.abs(np.asarray(x, np.float64))
    m, e = np.frexp(x)
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = mi & -mi
    return np.where(x > 0, low.astype(np.float64) * 2.0 ** (e.astype(np.float64) - 53), 0.0)


def is_exact(cloud):
    """every coordinate is a whole number of position quanta: the fixed-point sums then hold the exact sums"""
    c = np.asarray(cloud)[:, :3]
    lb = lowest_bit(c)
    return bool(np.all((lb == 0) | (lb >= quantum_pos(c.shape[0], maxabs(cloud)))))


def headroom(cloud):
    """n * max|coordinate| / quantum as a fraction of 2^62 (below 1 by the contract)"""
    n = np.asarray(cloud).shape[0]
    return n * maxabs(cloud) / quantum_pos(n, maxabs(cloud)) / 2.0 ** 62


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------------------
SEED = 20261019
CHAIN_N = 510          # 17 voxels x 30 points: a table of 1 024 slots
ROT_DEG = (0.3, -0.2, 0.4)


def chain_scene(shift_voxels=0):
    """12 chain voxels + 5 fillers, 30 points each, leaf 1.0. shift_voxels moves the whole geometry along all three axes by that many metres (the keys move with it: the
    chain is at the table's end only unshifted)"""
    ch = chain_at_table_end(CHAIN_N)
    vox = np.concatenate([ch.voxels, ch.filler(5)])
    rng = np.random.default_rng(SEED)
    tgt = points_in_voxels(vox + shift_voxels, 30, 1.0, rng)
    ghosts = points_in_voxels(ch.ghosts + shift_voxels, 1, 1.0, rng)
    assert tgt.shape[0] == CHAIN_N
    return dict(chain=ch, voxels=vox + shift_voxels, tgt=tgt, ghost_pts=ghosts, leaf=1.0, n_chain_pts=30 * len(ch.voxels))


def polar_chain_scene():
    ch = chain_at_table_end(CHAIN_N, candidates=polar_candidates())
    vox = np.concatenate([ch.voxels, ch.filler(5)])
    rng = np.random.default_rng(SEED + 1)
    tgt = points_in_polar_bins(vox, POLAR_RES, 30, rng)
    ghosts = points_in_polar_bins(ch.ghosts, POLAR_RES, 1, rng)
    return dict(chain=ch, voxels=vox, tgt=tgt, ghost_pts=ghosts, n_chain_pts=30 * len(ch.voxels))


def rpy_deg_to_R(r, p, y):
    r, p, y = (math.radians(a) for a in (r, p, y))
    Rx = np.array([[1, 0, 0], [0, math.cos(r), -math.sin(r)], [0, math.sin(r), math.cos(r)]])
    Ry = np.array([[math.cos(p), 0, math.sin(p)], [0, 1, 0], [-math.sin(p), 0, math.cos(p)]])
    Rz = np.array([[math.cos(y), -math.sin(y), 0], [math.sin(y), math.cos(y), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def rotvec(R):
    """rotation vector of a rotation matrix near the identity (|.| = the angle): from the skew part, which keeps its digits where acos of the trace has lost them"""
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = float(np.linalg.norm(w))
    return w * (math.asin(min(s, 1.0)) / s) if s > 0 else w


def rotated_source(tgt, deg=ROT_DEG):
    src = np.zeros_like(tgt)
    src[:, :3] = (tgt[:, :3].astype(np.float64) @ rpy_deg_to_R(*deg).T).astype(np.float32)
    return src


# the key range: leaf 2^-10 makes x / leaf exact, and voxel k = floor(x * 1024 - 0.5)
RANGE_LEAF = 2.0 ** -10
_ULP_BELOW_1024 = 2.0 ** -14


def _range_side(xs, rng):
    p = np.zeros((len(xs), 4), np.float32)
    p[:, 0] = xs
    p[:, 1:3] = rng.uniform(-0.02, 0.02, size=(len(xs), 2))
    return p


def key_range_scene(m=40):
    """m consecutive floats just below x = 1024.0 (keys up to 2^20 - 1) and the m floats from the first whose key is -2^20 upward (x = -1024 + 2^-11 ...), y and z small.
    first_out: per end, the first float past it — x = 1024 + 2^-11 has key 2^20, x = -1024 + 7 * 2^-14 has key -2^20 - 1."""
    rng = np.random.default_rng(SEED + 2)
    hi = 1024.0 - _ULP_BELOW_1024 * np.arange(1, m + 1)
    lo = -1024.0 + 2.0 ** -11 + _ULP_BELOW_1024 * np.arange(0, m)
    tgt = np.concatenate([_range_side(hi, rng), _range_side(lo, rng)])
    assert np.array_equal(tgt[:, 0].astype(np.float64), np.concatenate([hi, lo]))   # every x is a float
    return dict(tgt=tgt, leaf=RANGE_LEAF, first_out=(1024.0 + 2.0 ** -11, -1024.0 + 7 * _ULP_BELOW_1024), idx_hi=0, idx_lo=m)


def range_keys(cloud, leaf=RANGE_LEAF):
    """UNIFORM keys in int64 (the oracle's are int32 too, but nothing here relies on what it does past 2^20)"""
    return np.floor(np.asarray(cloud)[:, :3].astype(np.float64) / leaf - 0.5).astype(np.int64)


def one_voxel_cloud(n, seed=SEED + 3):
    """the whole cloud in ONE voxel of leaf 64 at the top of a binade: x the n floats below 1024.0, y and z anywhere in the voxel's (32, 96): n * max * scale is as close to
    2^62 as a cloud of n points gets"""
    rng = np.random.default_rng(seed + n)
    p = np.zeros((n, 4), np.float32)
    p[:, 0] = 1024.0 - _ULP_BELOW_1024 * np.arange(1, n + 1)
    p[:, 1:3] = rng.uniform(36.0, 92.0, size=(n, 2))
    p = p[rng.permutation(n)]
    assert len(np.unique(pyorc.voxel_keys(p, pyorc.VOXEL_UNIFORM, 64.0), axis=0)) == 1
    return p


def tiny_and_far_cloud(per=256):
    """a voxel around the origin with coordinates of 1e-3 .. 1e-6 next to a voxel at 1 000 m (leaf 1.0): 512 points (bits_n = 10) below 1 024 m count in units of 2^-42,
    and a float in [2^-20, 2^-19) with an odd mantissa has its last bit at 2^-43"""
    rng = np.random.default_rng(SEED + 4)
    tiny = np.zeros((per, 4), np.float32)
    tiny[:, :3] = (10.0 ** rng.uniform(-6, -3, size=(per, 3)) * rng.choice([-1.0, 1.0], size=(per, 3))).astype(np.float32)
    far = points_in_voxels(np.array([[999, 999, 999]]), per, 1.0, rng)
    cloud = np.concatenate([tiny, far])
    assert not is_exact(cloud)
    return cloud


def sub_half_cloud(n=300):
    """every |coordinate| < 0.5: the exponent of the maximum is negative (leaf 0.125)"""
    rng = np.random.default_rng(SEED + 5)
    p = np.zeros((n, 4), np.float32)
    p[:, :3] = rng.uniform(-0.49, 0.49, size=(n, 3))
    assert maxabs(p) < 0.5
    return p


def lds_cloud(distinct, n=256, leaf=0.25, interleave=False, groups=1, seed=SEED + 6):
    """`groups` workgroups' worth of n points each, every group with exactly `distinct` voxels of its own, a voxel's points adjacent in input order (interleave: two voxels
    A B A B ...). The voxels sit on a line along x, two leaves apart."""
    rng = np.random.default_rng(seed + distinct + 1000 * groups + int(interleave))
    out = []
    for g in range(groups):
        if interleave:
            assert distinct == 2
            owner = np.arange(n) % 2
        else:
            owner = np.sort(np.arange(n) % distinct) if distinct < n else np.arange(n)
            owner = np.sort(owner)
        vox = np.zeros((n, 3), np.int64)
        vox[:, 0] = 2 * (owner + g * distinct) - distinct * groups
        vox[:, 1] = g
        u = rng.uniform(0.05, 0.95, size=(n, 3))
        p = np.zeros((n, 4), np.float32)
        p[:, :3] = ((vox + 0.5 + u) * leaf).astype(np.float32)
        out.append(p)
    cloud = np.concatenate(out)
    k = pyorc.voxel_keys(cloud, pyorc.VOXEL_UNIFORM, leaf)
    assert len(np.unique(k, axis=0)) == distinct * groups
    for g in range(groups):
        assert len(np.unique(k[g * n:(g + 1) * n], axis=0)) == distinct
    return cloud, leaf


def spd_covariances(n, rng, lo=1e-6, hi=1e6):
    """n x 4 x 4 (3 x 3 block SPD, eigenvalues log-uniform in [lo, hi], last row and column zero) as the caller of setTargetCovariances hands them in"""
    out = np.zeros((n, 4, 4))
    for i in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        w = 10.0 ** rng.uniform(math.log10(lo), math.log10(hi), size=3)
        c = (q * w) @ q.T
        out[i, :3, :3] = 0.5 * (c + c.T)
    return out
