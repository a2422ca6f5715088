"""Constructed rings for extract_kernel (rolo_amd/csrc/front_extract.hpp): projections made as arrays, one case per path and edge of the kernel.

A case is a projection dict — what FrontEnd.project() / pyorc.project return, and what FrontEnd.loadProjection / pyorc.extract_features /
twin_front.extract_features take — plus the feature parameters, a one-line purpose and `expect_paths`: the path word (ROLO_XPATH_*,
include/rolo_hip.h) that the kernel must report for each ring the case is about. Plain numpy, no GPU. tests/test_front_rings_twin.py shows on the
CPU that the C++ oracle and the numpy twin agree on every case and that each case reaches what it is there for; tests/test_gpu_front_rings.py
runs the kernel on them.

How a ring chooses its path (extract_kernel; s / e = startRingIndex / endRingIndex, sector j = [sp_j, ep_j] with sp_j = (s (6 - j) + e j) / 6,
ep_j = (s (5 - j) + e (j + 1)) / 6 - 1, C division; pop = e - s + 10):

  whole-ring fixed point ATTEMPTED iff  surf_threshold > 0 and edge_threshold >= surf_threshold and e - s >= 12 and every sector non-empty
                                        (ep_j > sp_j) and the longest sorted range max(ep_j - sp_j) > 32 (sort segment >= 64)
                                        [a head ring, s < 5, also needs ep_0 >= 5: implied by a non-empty sector 0, whose sp_0 is 4]
  ... APPLIED unless a sector has more than 20 corner picks (CAPPED: discarded, ring redone stage by stage)
  stage by stage, sector j:   EMPTY if sp_j >= ep_j;  SERIAL if it holds the cloud's head (sp_j < 5) and not (surf_threshold > 0 and
                              edge_threshold >= 0);  PARALLEL otherwise

What validated arrays cannot reach, and why no case tries:
  * the tail-ring rule (ep_5 >= n - 5): endRingIndex + 6 <= n gives ep_5 = e - 1 <= n - 7;
  * the serial walk in a sector other than sector 0: s >= 4 always, so sp_j < 5 means j (e - 4) < 6 on the head ring (s = 4), while a
    non-empty sector there needs ep_j >= 5, i.e. j (e - 4) + e >= 16, hence e >= 11 and j = 0. (The third way into the serial walk, a sorted
    range of SEGMAX = MAXH / 4 positions, needs a ring of more than Horizon_SCAN points, which rolo_front_load_projection refuses.)
  * NaN / infinite ranges: std::sort on NaN keys is undefined in the reference; a voxel grid whose cell-count product exceeds 2^63: PCL's
    own int64 product overflows (the pass-through cases keep it between 2^31 and 2^63).
"""
from __future__ import annotations

import numpy as np

F = np.float32

# ---- the path word (include/rolo_hip.h) -------------------------------------------------------------------------------
RING_NONE, RING_CAPPED, RING_APPLIED = 0, 1, 2
SEC_NOT_STAGED, SEC_EMPTY, SEC_PARALLEL, SEC_SERIAL = 0, 1, 2, 3
_RING = {"N": RING_NONE, "C": RING_CAPPED, "A": RING_APPLIED}
_SEC = {"-": SEC_NOT_STAGED, "E": SEC_EMPTY, "P": SEC_PARALLEL, "S": SEC_SERIAL}


def W(ring, sectors="------"):
    """path word from its reading: W('N', 'SPPPPP') = fixed point not attempted, sector 0 on the serial walk, sectors 1..5 parallel"""
    assert len(sectors) == 6
    return _RING[ring] | sum(_SEC[c] << (2 + 2 * j) for j, c in enumerate(sectors))


def ring_level(word):
    return int(word) & 3


def sector_level(word, j):
    return (int(word) >> (2 + 2 * j)) & 3


APPLIED = W("A")
STAGED = W("N", "PPPPPP")
CAPPED = W("C", "PPPPPP")
ALL_EMPTY = W("N", "EEEEEE")


def sectors(s, e):
    """[(sp, ep)] of the six sectors, C integer division (truncation towards zero)"""
    div = lambda a: int(a / 6) if a < 0 else a // 6   # noqa: E731 — |a| is far below 2^53
    return [(div(s * (6 - j) + e * j), div(s * (5 - j) + e * (j + 1)) - 1) for j in range(6)]


# ---- the constructor ----------------------------------------------------------------------------------------------------
def build(pops, H, col="dense", range_=10.0, xyz="random", seed=0):
    """Projection dict of rings with the populations `pops` (in order) on a range image of H columns.

    startRingIndex = count - 1 + 5 before a ring and endRingIndex = count - 1 - 5 after it, count running from 0 to n, as cloudExtraction writes them.
    col:     'dense' (0, 1, 2, ... in every ring), an int k (first column k, then dense), or an array of n columns;
    range_:  a number (constant range) or an array of n ranges;
    xyz:     'random' or an array (n, 4) of x, y, z, intensity — the coordinates matter to the voxel filter only."""
    pops = [int(p) for p in pops]
    n = sum(pops)
    assert all(0 <= p <= H for p in pops)
    ends = np.cumsum(pops); begins = ends - pops
    if isinstance(col, (str, int)):
        first = 0 if col == "dense" else int(col)
        col = np.concatenate([first + np.arange(p) for p in pops] + [np.zeros(0, np.int64)])
    col = np.asarray(col).astype(np.int32)
    rng = np.full(n, range_, F) if np.isscalar(range_) else np.asarray(range_, F)
    if isinstance(xyz, str):
        assert xyz == "random"
        xyz = random_xyz(n, seed)
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 4)
    assert col.shape == (n,) and rng.shape == (n,) and xyz.shape == (n, 4)
    assert n == 0 or (col.min() >= 0 and col.max() < H), "a column outside the range image"
    assert np.isfinite(rng).all() and np.isfinite(xyz).all()
    return dict(n=n, extracted=xyz, point_col_ind=col, point_range=rng, start_ring=(begins - 1 + 5).astype(np.int32), end_ring=(ends - 1 - 5).astype(np.int32))


def ring_slices(pops):
    ends = np.cumsum(pops)
    return [slice(int(b), int(e)) for b, e in zip(ends - np.asarray(pops), ends)]


# ---- column patterns ------------------------------------------------------------------------------------------------------
STEPS = (1, 2, 9, 10, 11, 12, 30)   # 9 / 10 / 11 / 12: the suppression reach breaks at > 10, the occlusion test wants < 10


def step_cols(pops, H, seed, p=(0.3, 0.2, 0.1, 0.1, 0.1, 0.1, 0.1)):
    """every ring: columns rising by random steps from STEPS"""
    g = np.random.default_rng(seed)
    out = []
    for pop in pops:
        c = np.cumsum(g.choice(STEPS, size=pop, p=p)) - 1
        assert pop == 0 or c[-1] < H, "the steps leave the image: another seed or fewer points"
        out.append(c)
    return np.concatenate(out + [np.zeros(0, np.int64)])


def strided_cols(pops, firsts, stride):
    """ring r: firsts[r], firsts[r] + stride, ..."""
    return np.concatenate([f + stride * np.arange(p) for p, f in zip(pops, firsts)])


# ---- range profiles -------------------------------------------------------------------------------------------------------
def noise_range(n, seed, base=10.0, sigma=0.035):
    """curvature = (stencil sum)^2 with a stencil sum of standard deviation sqrt(110) sigma = 0.37: about 1.5 % of the cells above the default edge threshold (0.89),
    60 % below the default surface threshold (0.32) — far too few corners for the cap of 20 per sector"""
    return (base + sigma * np.random.default_rng(seed).standard_normal(n)).astype(F)


def ramp_range(pops, down=False):
    """curvature rising (falling) along every ring: range 10 + eps i^3 has the stencil sum 330 eps i; eps = 0.064 / pop^2 keeps the neighbour differences (< 0.2) below every
    mark. On a ring of 400 the step of the stencil sum per cell (1.3e-4) is far above its rounding (1e-5): the order is exact; on a ring of 1024 (6.7e-6) it is approximate."""
    out = []
    for p in pops:
        i = np.arange(p, dtype=np.float64)
        if down:
            i = p - 1 - i
        out.append((10.0 + 0.064 / p ** 2 * i ** 3).astype(F))
    return np.concatenate(out)


def plateau_range(n, period=23):
    """8.0 everywhere, 8.25 every `period`-th cell: dyadic, so the curvatures are exactly 0, 0.0625 (a spike among the ten) and 6.25 (the spike)"""
    r = np.full(n, 8.0, F)
    r[::period] = 8.25
    return r


def saw_range(n, period=6, base=10.0, d=0.1):
    """a spike of d every `period`-th cell: curvature (10 d)^2 = 1 at the spike — above the default edge threshold, d below the parallel-beam and depth-jump tests —
    and the spikes more than five cells apart, so none suppresses the next: a 170-cell sector holds 28 corner picks"""
    r = np.full(n, base, F)
    r[::period] = F(base) + F(d)
    return r


def jumpy_range(n, seed, toggles=(), rate=0.125, lo=10.0, hi=10.5, sigma=0.01):
    """two depth levels 0.5 apart (above the 0.3 of the occlusion test), the level changing at random cells and at every cell of `toggles`, plus a little noise"""
    g = np.random.default_rng(3000 + seed)
    flip = g.random(n) < rate
    flip[list(toggles)] = True
    level = np.cumsum(flip) % 2
    return (np.where(level == 1, hi, lo) + sigma * g.standard_normal(n)).astype(F)


def jump_range(n, at, lo, hi):
    """range lo up to and including cell `at`, hi behind it"""
    r = np.full(n, lo, F)
    r[at + 1:] = hi
    return r


# ---- coordinates ---------------------------------------------------------------------------------------------------------
def random_xyz(n, seed, span=(50.0, 50.0, 5.0)):
    g = np.random.default_rng(1000 + seed)
    out = np.empty((n, 4), F)
    out[:, :3] = (g.uniform(-1, 1, (n, 3)) * np.asarray(span)).astype(F)
    out[:, 3] = g.uniform(0, 100, n).astype(F)   # the intensity column varies: the centroid averages it too
    return out


def lattice_xyz(n, leaf):
    """points ON the cell boundaries: exact float multiples k * leaf, k negative too — floor(p * (1 / leaf)) decides the cell"""
    i = np.arange(n)
    out = np.empty((n, 4), F)
    out[:, 0] = (i % 7 - 3).astype(F) * F(leaf); out[:, 1] = ((i // 7) % 5 - 2).astype(F) * F(leaf); out[:, 2] = ((i // 35) % 3 - 1).astype(F) * F(leaf)
    out[:, 3] = (i % 11).astype(F)
    return out


def one_cell_xyz(n, leaf, seed):
    """every point inside one cell: each ring's filter is a single serial run as long as its surface scan"""
    g = np.random.default_rng(2000 + seed)
    out = np.empty((n, 4), F)
    out[:, :3] = (g.uniform(0.05, 0.95, (n, 3)) * leaf).astype(F)
    out[:, 3] = g.uniform(0, 100, n).astype(F)
    return out


def own_cell_xyz(n, leaf):
    """every point in a cell of its own along x: as many run heads as points"""
    out = np.zeros((n, 4), F)
    out[:, 0] = (np.arange(n) * 2.5 * leaf - 1.25 * leaf * n).astype(F); out[:, 3] = (np.arange(n) % 13).astype(F)
    return out


# ---- the case table ----------------------------------------------------------------------------------------------------
CASES = {}


def case(name, purpose, pops, H, expect_paths, edge=0.8, surf=0.1, leaf=0.4, **kw):
    """expect_paths: {ring: word}, or one word for every ring"""
    assert name not in CASES
    if not isinstance(expect_paths, dict):
        expect_paths = {r: expect_paths for r in range(len(pops))}
    assert len(pops) <= 16 and (H <= 2048 or len(pops) <= 4)
    CASES[name] = dict(name=name, purpose=purpose, proj=build(pops, H, **kw), pops=list(pops), n_scan=len(pops), horizon_scan=H, edge_threshold=edge, surf_threshold=surf,
                       odometry_surf_leaf_size=leaf, expect_paths={int(r): int(w) for r, w in expect_paths.items()})


def params(c):
    return dict(n_scan=c["n_scan"], horizon_scan=c["horizon_scan"], edge_threshold=c["edge_threshold"], surf_threshold=c["surf_threshold"],
                odometry_surf_leaf_size=c["odometry_surf_leaf_size"])


def rings(*words):
    return dict(enumerate(words))


def _n(pops):
    return int(sum(pops))


# With the default thresholds (0 < surf <= edge) what decides is the population: e - s = pop - 10, sp_j = s + (pop - 10) j / 6. No sector below 17 points; sector 5 only at
# 17; sectors 2, 5 at 18; 1, 3, 5 at 19; all but 0 and 3 at 20; all but 0 at 21 (e - s = 11); all six from 22 (e - s = 12). The longest sorted range is 32 at 208 points and
# 33 at 209: the fixed point is attempted from 209. It is the same for the ring that starts the cloud (s = 4).
_pops = [300, 0, 1, 11, 12, 13, 17, 18, 19, 20, 21, 22, 208, 209, 60]
case("pops_small", "rings of 0, 1, 11, 12, 13 points; each sector pattern of 17..21; both sides of e - s >= 12 / all sectors filled (21, 22) and of the sort segment 64 (208, 209)", _pops, 1024,
     rings(APPLIED, ALL_EMPTY, ALL_EMPTY, ALL_EMPTY, ALL_EMPTY, ALL_EMPTY, W("N", "EEEEEP"), W("N", "EEPEEP"), W("N", "EPEPEP"), W("N", "EPPEPP"), W("N", "EPPPPP"), STAGED, STAGED,
           APPLIED, STAGED), range_=noise_range(_n(_pops), 1))
case("head_small", "the first rings empty and the head ring too small for its sector 0 (ep_0 = 4 < 5)", [0, 0, 21, 250, 40], 1024,
     rings(ALL_EMPTY, ALL_EMPTY, W("N", "EPPPPP"), APPLIED, STAGED), range_=noise_range(311, 2))
case("head_not_ring0", "the head ring is ring 2 and takes the fixed point with its stale {0, 0} entry", [0, 0, 250, 30], 1024, rings(ALL_EMPTY, ALL_EMPTY, APPLIED, STAGED),
     range_=noise_range(280, 3))
case("head_22", "a head ring of 22 points: every sector two cells, sector 0 = cells 4, 5 with the stale entry", [22, 250], 1024, rings(STAGED, APPLIED), range_=noise_range(272, 4))
for _name, _pp in (("cloud_n3", [3, 0, 0]), ("cloud_n10", [10]), ("cloud_n11", [4, 7]), ("cloud_n12", [12, 0])):
    case(_name, "a whole cloud of %d points: %d live curvature cells, no sector" % (_n(_pp), max(0, _n(_pp) - 10)), _pp, 1024, ALL_EMPTY, range_=noise_range(_n(_pp), 5))
case("full_1024", "rings of H - 1 and H points at H = 1024", [1023, 1024, 1024], 1024, APPLIED, range_=noise_range(3071, 6))
case("full_2048", "rings of H - 1 and H points at H = 2048: sectors of 340 positions, sort segments of 512 = SEGMAX", [2047, 2048], 2048, APPLIED, range_=noise_range(4095, 7))

# -- range profiles
case("const", "constant range: every curvature +0, every sort key ties on its value, a surface every sixth cell the length of the ring", [1024, 300, 209, 208], 1024,
     rings(APPLIED, APPLIED, APPLIED, STAGED))
case("const_16", "the same on sixteen full rings (the large case of the sequence test)", [1024] * 16, 1024, APPLIED)
case("ramp_up", "curvature rising along the ring: rank order = position order, every cell a surface candidate", [1024, 400], 1024, APPLIED, range_=ramp_range([1024, 400]))
case("ramp_down", "curvature falling along the ring: rank order opposite to position order", [1024, 400], 1024, APPLIED, range_=ramp_range([1024, 400], down=True))
# 1024-ring: curvature (330 eps i)^2 = 4.1e-10 i^2 passes 1e-4 at i = 497: three sectors of 170 corner candidates, a pick every sixth -> 28 > 20; 400-ring: sectors of 65 cells, at most 11 picks
case("ramp_up_cap", "the ramp with thresholds inside it: the upper half of the long ring is corner candidates in position order, the cap strikes", [1024, 400], 1024, rings(CAPPED, APPLIED),
     edge=1e-4, surf=1e-5, range_=ramp_range([1024, 400]))
case("ramp_down_cap", "... and in opposite order", [1024, 400], 1024, rings(CAPPED, APPLIED), edge=1e-4, surf=1e-5, range_=ramp_range([1024, 400], down=True))
EDGE_PLATEAU = 0.0625
EDGE_BELOW_PLATEAU = float(np.nextafter(F(0.0625), F(0)))
case("plateau_at", "a plateau of curvature exactly 0.0625 and edge_threshold exactly that: the comparison is strict, no corner (edge < surf: staged)", [1024] * 16, 1024, STAGED,
     edge=EDGE_PLATEAU, range_=plateau_range(16384))
case("plateau_below", "... one float below: the plateau is corner candidates of equal curvature", [1024] * 16, 1024, STAGED, edge=EDGE_BELOW_PLATEAU, range_=plateau_range(16384))
# per period of 23 cells ten plateau cells in two groups of five beside the (marked) spike: a pick suppresses its group, so at most 2 x 8 = 16 picks in a sector of 171
case("plateau_fast_at", "the plateau on the fixed point (surf below it)", [1024, 1024, 300], 1024, APPLIED, edge=EDGE_PLATEAU, surf=0.03, range_=plateau_range(2348))
case("plateau_fast_below", "... one float below", [1024, 1024, 300], 1024, APPLIED, edge=EDGE_BELOW_PLATEAU, surf=0.03, range_=plateau_range(2348))
# 1024 points: sectors of 169-170 cells, a spike every sixth -> 28 picks; 300 points: 48-49 cells -> 8 or 9
case("saw_cap", "a saw with 28 corner picks per sector: the fixed point runs, the cap of 20 strikes, the ring is redone stage by stage", [1024, 1024, 300, 208], 1024,
     rings(CAPPED, CAPPED, APPLIED, STAGED), range_=saw_range(2556))
case("saw_cap_staged", "the cap striking in a ring that was staged from the start (edge < surf)", [1024, 300], 1024, STAGED, edge=0.05, range_=saw_range(1324))


def _spikes_range(count):
    """two constant rings of 1024; `count` spikes six cells apart inside sector 1 of ring 1 (cells 1197 .. 1365): exactly `count` corner picks there, none elsewhere"""
    r = np.full(2048, 10.0, F)
    r[1210 + 6 * np.arange(count)] = F(10.0) + F(0.1)   # (from 1210: the last surface pick of sector 0 marks up to cell 1201)
    return r


case("saw_20", "exactly 20 corner picks in a sector: the cap does not strike", [1024, 1024], 1024, APPLIED, range_=_spikes_range(20))
case("saw_21", "exactly 21: it does", [1024, 1024], 1024, rings(APPLIED, CAPPED), range_=_spikes_range(21))

# The depth jump sits between cells 298 and 299 of a 300-point ring: `depth2 - depth1 > 0.3` marks 299 .. 304, and 304 = s of ring 1 is the first cell of its first sector.
# float(1.3) - 1 = 0.29999995 (no mark), float(4.3) - 4 = 0.30000019 (mark), float(0.5 + 0.3f) - 0.5 = 0.3f exactly = 0.300000012: above the double 0.3 the reference compares with
JUMPS = {"jump_1": (F(1.0), F(1.0) + F(0.3)), "jump_4": (F(4.0), F(4.0) + F(0.3)), "jump_half": (F(0.5), F(0.5) + F(0.3))}
for _name, (_lo, _hi) in JUMPS.items():
    case(_name, "a depth jump of %.9g two cells before a ring border, default thresholds" % float(F(_hi - _lo)), [300, 300, 300], 1024, APPLIED, range_=jump_range(900, 298, _lo, _hi))
    case(_name + "_marks", "... with nothing picked (surf_threshold 0): `picked` is the occlusion marks alone; the head sector walks serially", [300, 300, 300], 1024,
         rings(W("N", "SPPPPP"), STAGED, STAGED), surf=0.0, range_=jump_range(900, 298, _lo, _hi))

# ... and falling: `depth1 - depth2 > 0.3` marks 293 .. 298, and 293 = e - 1 of ring 0 is the last cell of its last sector
case("drop_half", "a depth drop of exactly 0.3f two cells before a ring border, default thresholds", [300, 300, 300], 1024, APPLIED, range_=jump_range(900, 298, F(0.5) + F(0.3), F(0.5)))
case("drop_half_marks", "... with nothing picked", [300, 300, 300], 1024, rings(W("N", "SPPPPP"), STAGED, STAGED), surf=0.0, range_=jump_range(900, 298, F(0.5) + F(0.3), F(0.5)))


def _beam_range(d):
    r = np.full(600, 10.0, F)
    for j in (150, 300):   # 300: the first cell of ring 1, its neighbours 299 and 301 on either side of the ring border
        r[j - 1] = r[j + 1] = d
    return r


BEAM_BELOW = F(10.2)                      # 10.1999998 - 10 = 0.199999809 < 0.02 * 10 in double
BEAM_ABOVE = np.nextafter(F(10.2), F(11))  # 0.200000763 > 0.2
case("beam_below", "parallel-beam test one float below 0.02 * range, nothing picked: no mark", [300, 300], 1024, rings(W("N", "SPPPPP"), STAGED), edge=100.0, surf=0.0, range_=_beam_range(BEAM_BELOW))
case("beam_above", "... one float above: cells 150 and 300 marked", [300, 300], 1024, rings(W("N", "SPPPPP"), STAGED), edge=100.0, surf=0.0, range_=_beam_range(BEAM_ABOVE))

# -- thresholds, on two noise rings (the head ring and another)
_r = noise_range(800, 8)
case("thr_equal", "edge == surf: still the fixed point (edge >= surf); at most 67 / 6 + 1 picks per sector", [400, 400], 1024, APPLIED, edge=0.1, surf=0.1, range_=_r)
case("thr_inverted", "edge < surf: a cell can be both kinds of candidate", [400, 400], 1024, STAGED, edge=0.05, surf=0.1, range_=_r)
case("thr_surf0", "surf_threshold 0: no surface candidate, the head sector on the serial walk", [400, 400], 1024, rings(W("N", "SPPPPP"), STAGED), surf=0.0, range_=_r)
case("thr_edge_neg", "edge_threshold < 0: the stale {0, 0} entry of the head sector is a corner candidate — the serial walk as written — and the cap strikes everywhere", [400, 400], 1024,
     rings(W("N", "SPPPPP"), STAGED), edge=-1.0, range_=_r)
case("thr_both_neg", "both thresholds negative: every cell a corner candidate, none a surface", [400, 400], 1024, rings(W("N", "SPPPPP"), STAGED), edge=-1.0, surf=-0.5, range_=_r)

# -- columns
_r = noise_range(120, 9); _r[:11] += F(0.5)   # a depth drop behind cell 10 marks 5 .. 10: no pick of sector 0 reaches point 0 before the stale entry's turn comes, last in the walk
for _c0 in (0, 10, 11, 500):
    case("col0_%d" % _c0, "first column of the cloud %d: how far the corner pick of point 0 (edge < 0) marks back into the guard cells" % _c0, [60, 60], 1024,
         rings(W("N", "SPPPPP"), STAGED), edge=-1.0, col=_c0, range_=_r)
case("steps_staged", "column steps from {1, 2, 9, 10, 11, 12, 30} under depth jumps: the reach of a pick (> 10) and the occlusion test (< 10)", [100, 100, 100], 1024, STAGED,
     col=step_cols([100] * 3, 1024, 1), range_=jumpy_range(300, 1))
case("steps_serial", "... with the head sector on the serial walk", [100, 100], 1024, rings(W("N", "SPPPPP"), STAGED), edge=-1.0, col=step_cols([100] * 2, 1024, 2), range_=jumpy_range(200, 2))
case("steps_fast", "... on the fixed point (noise: too few corners for the cap)", [215, 215], 2048, APPLIED, col=step_cols([215] * 2, 2048, 3), range_=noise_range(430, 10))
case("border_sparse", "sparse rings whose last and next-first columns are 5 apart, a depth jump on each border: marks and reach cross the ring border", [60, 60, 60], 1024, STAGED,
     col=strided_cols([60] * 3, (0, 300, 600), 5), range_=jumpy_range(180, 3, toggles=(60, 120)))
# dense columns: picks are at least six cells apart, at most 7 in a sector of 40
case("border_dense", "... dense rings three columns apart, on the fixed point", [250, 250, 250], 1024, APPLIED, col=strided_cols([250] * 3, (0, 252, 504), 1),
     range_=jumpy_range(750, 4, toggles=(250, 500)))

# -- coordinates: constant range, so a ring's surface scan is every cell of its sectors, pop - 10 points
case("vox_lattice", "points on exact multiples of the leaf, negative ones too", [1024, 300], 1024, APPLIED, xyz=lattice_xyz(1324, 0.4))
case("vox_dense", "random points, several to a cell", [1024, 300], 1024, APPLIED, xyz=random_xyz(1324, 11, span=(3.0, 3.0, 1.0)))
case("vox_one_cell", "all points in one cell: one serial run of 2038 points (a full 2048-ring)", [2048, 300], 2048, APPLIED, xyz=one_cell_xyz(2348, 0.4, 12))
case("vox_own_cell", "every point in its own cell: run heads at every wavefront and 1024-thread boundary; scans of 1024, 1025 and 1026 points", [1034, 1035, 1036], 2048, APPLIED,
     xyz=own_cell_xyz(3105, 0.4))
case("vox_pass", "cell-count product about 1.2e11, in (2^31, 2^63): PCL passes the scan through", [1024, 300], 1024, APPLIED, xyz=random_xyz(1324, 13, span=(1000.0, 1000.0, 1000.0)))
_r = np.full(34, 10.0, F); _r[27] = F(10.1)   # ring 1 = cells 17 .. 33, s = 21, e = 28, sector 5 = {26, 27}: 27 a corner (curvature 1 > 0.5), 26 suppressed and left in the scan
case("vox_scan_1_2", "surface scans of 2 points and of 1 point", [17, 17], 1024, W("N", "EEEEEP"), edge=0.5, range_=_r, xyz=own_cell_xyz(34, 0.4))

# -- the HBM-scratch form (Horizon_SCAN > 2048)
case("big_const", "scratch form, constant range, a full 4096-ring: sectors of 681 positions, sort segments of 1024", [4096, 300, 208, 0], 4096, rings(APPLIED, APPLIED, STAGED, ALL_EMPTY))
case("big_noise", "scratch form, full and almost full rings of noise", [4096, 4095], 4096, APPLIED, range_=noise_range(8191, 14, sigma=0.03))
case("big_cap", "scratch form, the cap strike (113 and 33 picks per sector)", [4096, 1200, 300], 4096, rings(CAPPED, CAPPED, APPLIED), range_=saw_range(5596))
case("big_inverted", "scratch form, edge < surf", [4096, 2000], 4096, STAGED, edge=0.05, range_=noise_range(6096, 15))
case("big_edge_neg", "scratch form, the serial walk of the head sector", [4096], 4096, W("N", "SPPPPP"), edge=-1.0, range_=noise_range(4096, 16))
