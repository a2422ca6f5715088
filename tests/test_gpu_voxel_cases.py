"""GPU: K6, the target voxel map, on the constructed voxels of tests/voxel_cases.py — a probe chain across the table's end, the key range's last voxels and the first ones
past them, fixed-point scales where they are tight, the workgroup table of accumulate_point_wg exactly full, handed-in covariances — in every form a map can be built in.
Each build asserts the form it ran through voxelBuildForm() (rolo_debug_voxel_build), so a case meant for one form cannot silently exercise another.

The reference is voxel_cases.exact_map: exact sums, correctly rounded. Bounds: means within 1 ulp where every coordinate is a whole number of position quanta (is_exact;
equality is what is seen), within half a quantum + 1 ulp otherwise; fixed-point covariances within half a covariance quantum + 1 ulp of the exact mean of the library's own
getTargetCovariances() (those are held to the oracle elsewhere); handed-in covariances (fp64 atomics, arrival order) within m * 2^-53 * max|c|, m the voxel's count."""
import functools

import numpy as np
import pytest

from oracle import pyorc
from rolo_amd._lib import RoloError
from rolo_amd.rotvgicp import RotVGICP, NeighborSearchMethod
import voxel_cases as V

pytestmark = pytest.mark.gpu

INPUT, CURVE, SEARCH, FRAME = 0, 1, 2, 3   # ROLO_VOXBUILD_*
D1, D7, D27 = int(NeighborSearchMethod.DIRECT1), int(NeighborSearchMethod.DIRECT7), int(NeighborSearchMethod.DIRECT27)
Z3 = np.zeros(3)
WORST = {}   # case -> (largest mean difference in ulps / in quanta, largest covariance difference over its bound): printed by the last test


def note(case, **kw):
    w = WORST.setdefault(case, {})
    for k, v in kw.items():
        w[k] = max(w.get(k, 0.0), float(v))
    print(case, " ".join("%s=%.3g" % kv for kv in kw.items()))


def nudged(tgt, leaf):
    """a source for the builds that go through a registration: the target moved by a hundredth of a leaf or two"""
    return (tgt + np.array([0.01, -0.02, 0.015, 0.0]) * leaf).astype(np.float32)


def context(leaf=1.0, polar=None, neighbor=D1):
    g = RotVGICP()
    if polar is not None:
        g.setPolarResolution(*polar)
    else:
        g.setResolution(leaf)
    g.setNeighborSearchMethod(neighbor)
    return g


@functools.lru_cache(maxsize=None)
def primer():
    return V.one_voxel_cloud(256)


def prime_for_curve_order(g, leaf):
    """a first map with >= 16 points per voxel in this context: its next staged build goes over the target in curve order"""
    p = primer()
    g.setResolution(64.0); g.setInputTarget(p); g.setInputSource(p.copy()); g.buildVoxelMap()
    assert g.voxelBuildForm()[0] == INPUT and len(g.voxels()[0]) == 1
    g.setResolution(leaf)


def run_build(g, form, tgt, src, covs=None):
    """one map build of `tgt` in the context, by the route that reaches `form`; raises what the build raises"""
    g.setInputTarget(tgt); g.setInputSource(src)
    if covs is not None:
        g.setTargetCovariances(covs)
    if form in (INPUT, CURVE):
        g.buildVoxelMap()
    else:
        if form == FRAME and covs is None:
            g.computeCovariances()
        g.register_async(None, Z3, Z3, Z3)
        g.register_wait()


def build(form, tgt, src=None, leaf=1.0, polar=None, covs=None, neighbor=D1, g=None):
    """a map of `tgt` built in `form` (asserted); returns the context"""
    src = nudged(tgt, leaf) if src is None else src
    if g is None:
        g = context(leaf, polar, neighbor)
        if form == CURVE and polar is None:
            prime_for_curve_order(g, leaf)
    run_build(g, form, tgt, src, covs)
    got = g.voxelBuildForm()
    fixed = covs is None
    assert got[0] == form, (got, form)
    assert got[1] == int(fixed) and got[3] == V.mask_of(tgt.shape[0]) + 1, got
    if covs is not None and form == INPUT:
        assert got[2] == 1, got    # no search ran on this target: max|coordinate| from the points (maxabs_kernel)
    if covs is None:
        assert got[2] == 0, got    # ... otherwise from the search's bounding box
    return g


def check_map(case, g, tgt, voxel_type=pyorc.VOXEL_UNIFORM, leaf=1.0, covs=None):
    """the common assertions; returns the map in key order"""
    keys = pyorc.voxel_keys(tgt, voxel_type, leaf, V.POLAR_RES)
    assert np.array_equal(g.targetVoxelKeys(), keys)
    handed = covs is not None
    cov = covs if handed else g.getTargetCovariances()
    ek, ec, em, ev = V.exact_map(tgt, keys, cov)
    k, c, m, v = V.sort_map(*g.voxels())
    assert np.array_equal(k, ek) and np.array_equal(c, ec)
    n = tgt.shape[0]
    d = np.abs(m - em)
    if V.is_exact(tgt):
        note(case, mean_ulps=(d / V.ulp(em)).max())
        assert np.all(d <= V.ulp(em))
    else:
        q = V.quantum_pos(n, V.maxabs(tgt))
        note(case, mean_quanta=(d / q).max())
        assert np.all(d <= 0.5 * q + V.ulp(em))
    dc = np.abs(v - ev)
    if handed:
        bound = ec[:, None, None] * 2.0 ** -53 * np.abs(cov[:, :3, :3]).max() * np.ones_like(dc)
    else:
        assert np.abs(cov).max() <= 1.0 + 1e-9   # the bound the covariance scale assumes
        bound = 0.5 * V.quantum_cov(n) + V.ulp(ev)
    note(case, cov_over_bound=(dc / bound).max(), cov_abs=dc.max())
    assert np.all(dc <= bound)
    return k, c, m, v


def same_bytes(a, b, with_cov=True):
    for x, y in list(zip(a, b))[:4 if with_cov else 3]:
        assert np.array_equal(x, y)


def gpu_pairs(g):
    """the correspondence list as a set of (source index, voxel key)"""
    found, keys = g.correspondences()
    return {(int(i), tuple(int(x) for x in keys[i, j])) for i, j in zip(*np.nonzero(found))}


def oracle_pairs(o):
    s, v = o.correspondences()
    vk = o.voxels()[0]
    return {(int(i), tuple(int(x) for x in vk[j])) for i, j in zip(s, v)}


def oracle_for(tgt, src, leaf=1.0, polar=None, neighbor=D1, **kw):
    p = pyorc.default_params(voxel_type=pyorc.VOXEL_POLAR if polar else pyorc.VOXEL_UNIFORM, voxel_resolution=leaf, polar_resolution=polar or V.POLAR_RES,
                             neighbor_search=neighbor, **kw)
    o = pyorc.Reg(p); o.set_target(tgt); o.set_source(src)
    return o


# ---- a. the chain across the table's end -------------------------------------------------------------------------------------------------------------
def test_chain_across_the_table_end_in_every_form():
    sc = V.chain_scene()
    assert 0 in V.occupied(sc["voxels"], sc["chain"].mask)
    maps = []
    for form in (INPUT, CURVE, SEARCH, FRAME):
        g = build(form, sc["tgt"])
        maps.append(check_map("chain/form%d" % form, g, sc["tgt"]))
        g.close()
    for m in maps[1:]:
        same_bytes(maps[0], m)


def test_polar_chain_across_the_table_end():
    sc = V.polar_chain_scene()
    assert 0 in V.occupied(sc["voxels"], sc["chain"].mask)
    maps = []
    src = (sc["tgt"] * np.float32(1.0001)).astype(np.float32)   # along the rays: every point stays in its bin's azimuth and polar angle
    for form in (CURVE, SEARCH):   # a fresh POLAR context's staged build is the curve-order one
        g = build(form, sc["tgt"], src=src, polar=V.POLAR_RES)
        maps.append(check_map("polar chain/form%d" % form, g, sc["tgt"], voxel_type=pyorc.VOXEL_POLAR))
        if form == CURVE:   # ... and the lookups walk the same chain: own bins found, ghosts missed
            both = np.concatenate([sc["tgt"], sc["ghost_pts"]])
            g.setInputSource(both); g.so3_linearize(np.eye(4))
            o = oracle_for(sc["tgt"], both, polar=V.POLAR_RES); o.so3_linearize(np.eye(4))
            assert gpu_pairs(g) == oracle_pairs(o) == {(i, tuple(k)) for i, k in enumerate(np.repeat(sc["voxels"], 30, axis=0).tolist())}
        g.close()
    same_bytes(maps[0], maps[1])


@pytest.mark.parametrize("neighbor", [D1, D7, D27])
def test_lookups_walk_the_chain(neighbor):
    sc = V.chain_scene()
    both = np.concatenate([sc["tgt"], sc["ghost_pts"]])
    n, n_chain = sc["tgt"].shape[0], sc["n_chain_pts"]
    g = context(neighbor=neighbor); g.setInputTarget(sc["tgt"]); g.setInputSource(both)
    g.so3_linearize(np.eye(4))
    assert g.voxelBuildForm()[0] == INPUT
    o = oracle_for(sc["tgt"], both, neighbor=neighbor); o.so3_linearize(np.eye(4))
    got = gpu_pairs(g)
    assert got == oracle_pairs(o)
    own = np.repeat(sc["voxels"], 30, axis=0)
    for i in range(n):   # every point of the target (the chain's 360 first) is found under its own key
        assert (i, tuple(int(x) for x in own[i])) in got
    assert n_chain == 360
    ghost_keys = {tuple(int(x) for x in k) for k in sc["chain"].ghosts}
    assert not any(k in ghost_keys for _, k in got)   # no ghost voxel is ever found
    if neighbor == D1:
        assert not any(i >= n for i, _ in got) and len(got) == n
    g.close()


# ---- b. the three lookup implementations through the chain ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lm_forms_through_the_chain(fixed):
    """align() of the chain scene's rotated copy under fused_lm = 0, 1, 2 and the oracle's: [(pose, (outer iterations, converged, correspondences), lm_form)], oracle"""
    sc = V.chain_scene()
    src = V.rotated_source(sc["tgt"])
    o = oracle_for(sc["tgt"], src, fixed_iterations=fixed)
    rc, _, Td_o, it_o, cv_o = o.align()
    assert rc == 0
    out = []
    for fused in (0, 1, 2):
        g = context(); g.setFusedLm(fused); g.setFixedIterations(fixed)
        g.setInputTarget(sc["tgt"]); g.setInputSource(src)
        g.align()
        assert g.voxelBuildForm()[0] == SEARCH
        st = g.last_stats
        out.append((g.final_transformation_d.copy(), (st.n_outer, bool(st.converged), st.n_correspondences), g.lm_form()))
        g.close()
    return out, (Td_o, it_o, cv_o, len(np.unique(o.correspondences()[0])))


@pytest.mark.parametrize("fixed", [0, 4])
def test_three_lm_forms_look_up_through_the_chain(fixed):
    """pass + controller launches, one launch per trial and the resident kernel each carry their own probe loop: all three find the oracle's correspondences through the chain,
    take its iterations and end at its pose within the bars (1e-5 rad, 1e-4 m)"""
    out, (Td_o, it_o, cv_o, nc_o) = lm_forms_through_the_chain(fixed)
    for fused, (Td, st, form) in enumerate(out):
        dR = np.linalg.norm(V.rotvec(Td[:3, :3] @ Td_o[:3, :3].T)); dt = np.abs(Td[:3, 3] - Td_o[:3, 3]).max()
        print("fused_lm=%d fixed=%d: outer %d (oracle %d), %d correspondences (oracle %d), |dR| = %.3g rad, |dt| = %.3g m, max |T - T(fused_lm=0)| = %.3g" %
              (fused, fixed, st[0], it_o, st[2], nc_o, dR, dt, np.abs(Td - out[0][0]).max()))
        assert dR <= 1e-5 and dt <= 1e-4
        assert st == (it_o, cv_o, nc_o)
        assert (form["rows"] > 0) == (fused == 2), form   # the resident kernel ran, and only then
    assert out[0][1] == out[1][1] == out[2][1]


@pytest.mark.parametrize("fixed", [0, 4])
def test_three_lm_forms_end_at_the_same_bytes(fixed):
    """final_transformation_d the same bytes under fused_lm = 0, 1 and 2. The 510 points are two workgroups of 256 under pass + controller launches and one of 512 in the
    other two forms; a fat workgroup adds its wavefronts' sums in the groups of four that the pass kernel's rows are (lm_point.hpp block_reduce_store), so the one row is the
    sum of the two. (Added in one run of eight, as they were, the forms ended one ulp apart in one entry of the pose: 8.67e-19 on 0.0033, lookups and decisions equal.)"""
    out, _ = lm_forms_through_the_chain(fixed)
    assert out[0][1] == out[1][1] == out[2][1]
    print("max |T(fused_lm=1) - T(0)| = %.3g, max |T(2) - T(0)| = %.3g, max |T(2) - T(1)| = %.3g" %
          (np.abs(out[1][0] - out[0][0]).max(), np.abs(out[2][0] - out[0][0]).max(), np.abs(out[2][0] - out[1][0]).max()))
    assert np.array_equal(out[1][0], out[0][0]) and np.array_equal(out[2][0], out[0][0])


# ---- c. the key range ------------------------------------------------------------------------------------------------------------------------------
def range_source(tgt):
    """the target's own points (the edge voxels are looked up where they are) and one point far outside the key range"""
    out = np.array([[1030.0, 0.001, -0.002, 0.0]], np.float32)
    return np.concatenate([tgt, out])


@pytest.mark.parametrize("form", [INPUT, SEARCH, FRAME])
def test_last_keys_of_the_range(form):
    sc = V.key_range_scene()
    tgt, leaf = sc["tgt"], sc["leaf"]
    src = range_source(tgt)
    g = build(form, tgt, src=src, leaf=leaf, neighbor=D7)
    k, c, m, v = check_map("key range/form%d" % form, g, tgt, leaf=leaf)
    assert k[:, 0].max() == V.KEY_MAX and k[:, 0].min() == V.KEY_MIN   # the unpack round trip at both ends
    g.so3_linearize(np.eye(4))
    o = oracle_for(tgt, src, leaf=leaf, neighbor=D7); o.so3_linearize(np.eye(4))
    got = gpu_pairs(g)
    assert got == oracle_pairs(o)
    own = V.range_keys(tgt)
    for i in (sc["idx_hi"], sc["idx_lo"]):
        assert (i, tuple(int(x) for x in own[i])) in got        # the source points in the last voxels are found
    assert all(V.KEY_MIN <= x <= V.KEY_MAX for _, key in got for x in key)   # the offsets that step to 2^20 and -2^20 - 1 are not, without an error
    assert not any(i == tgt.shape[0] for i, _ in got)           # nor the source point outside the range
    g.close()


@pytest.mark.parametrize("end", [0, 1])
@pytest.mark.parametrize("form", [INPUT, CURVE, SEARCH, FRAME])
def test_first_key_past_the_range_is_an_error(form, end):
    sc = V.key_range_scene()
    tgt, leaf = sc["tgt"], sc["leaf"]
    bad = tgt.copy(); bad[sc["idx_hi"] if end == 0 else sc["idx_lo"], 0] = sc["first_out"][end]
    assert V.range_keys(bad)[:, 0].max() == 2 ** 20 if end == 0 else V.range_keys(bad)[:, 0].min() == -2 ** 20 - 1
    g = context(leaf)
    if form == CURVE:
        prime_for_curve_order(g, leaf)
    with pytest.raises(RoloError) as ei:
        run_build(g, form, bad, nudged(bad, leaf))
    assert ei.value.code == -10
    with pytest.raises(RoloError) as ei:
        g.voxelBuildForm()
    assert ei.value.code == -5   # no map
    build(form, tgt, leaf=leaf, g=g)   # the same context, given a good cloud, builds the right map in the same form
    check_map("after key range error/form%d" % form, g, tgt, leaf=leaf)
    g.close()


def test_non_finite_point_outranks_the_key_range():
    """ROLO_ENONFINITE (-11) and ROLO_EKEYRANGE (-10) in one build: the more negative code is reported. The NaN comes in through a coordinate of a target whose covariances
    are handed in — no neighbour search runs on that target, whose lists are not defined for a NaN point — and the build is the staged one."""
    sc = V.key_range_scene()
    tgt, leaf = sc["tgt"], sc["leaf"]
    covs = V.spd_covariances(tgt.shape[0], np.random.default_rng(5), 1e-3, 1.0)
    bad = tgt.copy(); bad[sc["idx_hi"], 0] = sc["first_out"][0]
    g = context(leaf)
    with pytest.raises(RoloError) as ei:
        run_build(g, INPUT, bad, tgt.copy(), covs)
    assert ei.value.code == -10
    bad2 = bad.copy(); bad2[7, 1] = np.nan
    with pytest.raises(RoloError) as ei:
        run_build(g, INPUT, bad2, tgt.copy(), covs)
    assert ei.value.code == -11
    only_nan = tgt.copy(); only_nan[7, 1] = np.nan
    with pytest.raises(RoloError) as ei:
        run_build(g, INPUT, only_nan, tgt.copy(), covs)
    assert ei.value.code == -11
    build(INPUT, tgt, src=tgt.copy(), leaf=leaf, covs=covs, g=g)
    check_map("after non-finite error", g, tgt, leaf=leaf, covs=covs)
    g.close()


# ---- d. the fixed-point scales -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scale_cloud(name):
    if name.startswith("shift"):
        return V.chain_scene(int(name[5:]))["tgt"], 1.0
    if name.startswith("one"):
        return V.one_voxel_cloud(int(name[3:])), 64.0
    return {"tinyfar": (V.tiny_and_far_cloud(), 1.0), "subhalf": (V.sub_half_cloud(), 0.125)}[name]


@pytest.mark.parametrize("name", ["shift-1000", "shift-60000", "one255", "one256", "one257", "one511", "one512", "tinyfar", "subhalf"])
def test_scales_where_they_are_tight(name):
    tgt, leaf = scale_cloud(name)
    if name.startswith("shift"):
        assert np.all(tgt[:, :3] < 0)        # max |coordinate| is a box MINIMUM
    if name.startswith("one"):
        assert 0.49 < V.headroom(tgt) < 1.0  # n * max * scale against 2^62
    assert V.is_exact(tgt) == (name != "tinyfar")
    maps = []
    for form in (INPUT, SEARCH):
        g = build(form, tgt, leaf=leaf)
        maps.append(check_map("%s/form%d" % (name, form), g, tgt, leaf=leaf))
        g.close()
    same_bytes(maps[0], maps[1])
    covs = V.spd_covariances(tgt.shape[0], np.random.default_rng(11))
    g = build(INPUT, tgt, leaf=leaf, covs=covs)
    handed = check_map("%s/handed-in" % name, g, tgt, leaf=leaf, covs=covs)
    same_bytes(maps[0], handed, with_cov=False)   # positions are fixed point whatever the covariances go through, and the scale from the points is the box's
    g.close()


# ---- e. the workgroup table's edge -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distinct,groups,interleave", [(127, 1, False), (128, 1, False), (129, 1, False), (256, 1, False), (2, 1, True), (129, 4, False)])
def test_workgroup_table_exactly_full_and_one_over(distinct, groups, interleave):
    tgt, leaf = V.lds_cloud(distinct, interleave=interleave, groups=groups)
    maps = []
    for form in (INPUT, SEARCH):
        g = build(form, tgt, leaf=leaf)
        maps.append(check_map("lds %d x %d%s/form%d" % (groups, distinct, " interleaved" if interleave else "", form), g, tgt, leaf=leaf))
        g.close()
    same_bytes(maps[0], maps[1])
    assert len(maps[0][0]) == distinct * groups


# ---- f. handed-in covariances ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, -60000])
def test_handed_in_covariances(shift):
    tgt = V.chain_scene(shift)["tgt"]
    covs = V.spd_covariances(tgt.shape[0], np.random.default_rng(7))
    assert np.abs(covs).max() > 1e5 and np.abs(covs[:, :3, :3]).min() < 1e-4
    maps = []
    for trial in range(2):
        g = build(INPUT, tgt, covs=covs)
        maps.append(check_map("handed-in %d/build %d" % (shift, trial), g, tgt, covs=covs))
        g.close()
    same_bytes(maps[0], maps[1], with_cov=False)   # (the covariances' fp64 atomics arrive in any order: held to the bound, not to their bits)


def test_report():
    """the largest differences seen per case (run with -s)"""
    for case in sorted(WORST):
        print("WORST", case, " ".join("%s=%.3g" % kv for kv in sorted(WORST[case].items())))
