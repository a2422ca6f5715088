"""GPU: rolo_scan2map_optimize on the constructed scenarios of tests/s2m_scenarios.py against the C++ oracle (pyorc.scan2map) on the same arrays — the branches whole lidar
scans never reach (tests/test_gpu_backend.py): rank-deficient and inconsistent plane fits, the fifth neighbour at d2 == 1 exactly and fewer than five points in the
ball, equal distances, one-leaf and few-leaf trees, partial wavefronts and workgroups, the scatter back to the caller's order, the n_selected < 50 exit, a degenerate
first linearisation with its projected step — and both forms of the association kernel (s2m_assoc_kernel, the product; s2m_kernel, its cross-check) on all of them. What the oracle says about these arrays is itself pinned
on the CPU (tests/test_oracle_backend.py: the twin, a float64 statement of the fits, what each case is there to reach).

Bars: flags bit-identical, coefficients <= 1e-6 and poses <= 2e-6 to the oracle (the bars of tests/test_gpu_backend.py); well-conditioned cases also <= FLOAT64_TOL to
the float64 fit (s2m_scenarios.py: 4 x the oracle's own measured deviation)."""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import s2m_scenarios as S
from oracle import pyorc
from rolo_amd.backend import Scan2Map

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("skipped", "iterations", "converged", "degenerate", "n_selected")
TABLES = {"table": (S.table, S.TABLE), "general_pose": (S.table_general_pose, S.TABLE), "ties": (S.ties, S.TIES)}


@pytest.fixture(scope="module")
def s2m():
    g = Scan2Map(edgeFeatureMinValidNum=0, surfFeatureMinValidNum=0)
    yield g
    g.close()


@functools.lru_cache(maxsize=None)
def _table(which):
    """(scenario, names, oracle result, float64 fit) of a case table, computed once and shared"""
    scn, names = TABLES[which][0]()
    return scn, names, pyorc.scan2map(*scn[:5], edge_min=scn[5], surf_min=scn[6]), S.float64_fit(scn)


def _run(g, scn, resident=False):
    corner, surf, mc, ms, guess = scn[:5]
    assert (g.edge_min, g.surf_min) == (scn[5], scn[6])
    if resident:
        g.setSubmap(mc, ms)
    tf, sel, co = g.scan2MapOptimization(corner, surf, None if resident else mc, None if resident else ms, guess, want_debug=True)
    return tf, {k: getattr(g.last_stats, k) for k in STAT_FIELDS}, sel, co


def _hold_one_association(scn, names, oracle, got, cases=None, fit64=None):
    """one iteration, the pose exactly the guess, and feature by feature the oracle's flag and coefficients"""
    tf, st, sel, co = got
    _, st_o, sel_o, co_o = oracle
    assert st_o["iterations"] == 1 and st_o["n_selected"] < 50
    assert st == st_o, (st, st_o)
    assert np.array_equal(tf, scn[4]), f"the pose moved without 50 selected features: {tf} from {scn[4]}"
    flags = [(n, bool(sel[i]), bool(sel_o[i])) for i, n in enumerate(names) if sel[i] != sel_o[i]]
    assert not flags, f"(case, GPU flag, oracle flag): {flags}"
    dev = np.abs(co - co_o).max(axis=1)
    off = [(n, dev[i], co[i], co_o[i]) for i, n in enumerate(names) if not dev[i] <= 1e-6]
    assert not off, f"(case, |GPU - oracle|, GPU coefficients, oracle's): {off}"
    dirty = [n for i, n in enumerate(names) if not sel[i] and (co[i] != 0).any()]
    assert not dirty, f"unselected features with non-zero coefficients: {dirty}"
    if fit64 is not None:
        dev64 = np.abs(co - fit64[1]).max(axis=1)
        off64 = [(n, dev64[i]) for i, n in enumerate(names) if not cases[n].get("oracle_only") and not dev64[i] <= S.FLOAT64_TOL]
        assert not off64, f"(case, |GPU - float64 fit|) above {S.FLOAT64_TOL:.1e}: {off64}"


@pytest.mark.parametrize("which", list(TABLES))
def test_case_tables_match_the_oracle_feature_by_feature(s2m, which):
    scn, names, oracle, fit64 = _table(which)
    _hold_one_association(scn, names, oracle, _run(s2m, scn), TABLES[which][1], fit64)


@pytest.mark.parametrize("m", S.TREE_SIZES)
def test_tree_shapes(s2m, m):
    scn, names = S.tree_sweep(m)
    _hold_one_association(scn, names, pyorc.scan2map(*scn[:5], edge_min=0, surf_min=0), _run(s2m, scn))


@pytest.mark.parametrize("n_corner,n_surf", S.COUNT_PAIRS)
def test_feature_counts_and_scatter_to_caller_order(s2m, n_corner, n_surf):
    scn, names = S.count_sweep(n_corner, n_surf)
    _hold_one_association(scn, names, pyorc.scan2map(*scn[:5], edge_min=0, surf_min=0), _run(s2m, scn))


def test_resident_submap_gives_the_one_call_forms_bits(s2m):
    for which in ("table", "ties"):
        scn, names, oracle, fit64 = _table(which)
        one = _run(s2m, scn)
        res = _run(s2m, scn, resident=True)
        _hold_one_association(scn, names, oracle, res, TABLES[which][1], fit64)
        assert res[1] == one[1] and np.array_equal(res[0], one[0]) and np.array_equal(res[2], one[2])
        diff = [n for i, n in enumerate(names) if not np.array_equal(res[3][i], one[3][i])]
        assert not diff, f"resident and one-call coefficients differ in bits: {diff}"


@pytest.mark.parametrize("variant", list(S.SCENES))
def test_scenes_iterate_project_and_exit_like_the_oracle(s2m, variant):
    scn = S.corridor(variant)
    tf_o, st_o, sel_o, co_o = pyorc.scan2map(*scn[:5], edge_min=0, surf_min=0)
    assert st_o == S.SCENES[variant]
    tf, st, sel, co = _run(s2m, scn)
    assert st == st_o, (st, st_o)
    assert np.array_equal(sel, sel_o), f"{int((sel != sel_o).sum())} flags differ, first at feature {int(np.flatnonzero(sel != sel_o)[0])}"
    assert np.abs(co - co_o).max() <= 1e-6 and not co[~sel].any()
    assert np.abs(tf - tf_o).max() <= 2e-6, (tf, tf_o)
    assert S.scene_pose_problems(variant, tf, scn[4]) == []


SWITCHES = ["ROLO_S2M_PACKETS=0"]
_child_died = []   # a child that ended on a signal, faulted the GPU or ran out of time: nothing more is started on that GPU


@pytest.mark.parametrize("switch", SWITCHES)
def test_every_kernel_form_passes_this_module(switch):
    """the association kernel has two forms — s2m_assoc_kernel (the default: features sorted along the curve, four lanes per feature, the search capped at the
    radius the fits accept) and s2m_kernel (ROLO_S2M_PACKETS=0: one uncapped walk per lane in the caller's order, no search code in common with the other) —, both
    exact searches in front of the same fits: every test above must pass with the second as well (own process: the switches are read once)"""
    assert not _child_died, f"not started: the child for {_child_died[0]} ended on a signal or a timeout"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **dict(kv.split("=") for kv in switch.split()))
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_backend_cases.py"), "-m", "gpu", "-x", "-q", "-k", "not every_kernel_form"],
                           env=env, capture_output=True, text=True, timeout=240, cwd=root)
    except subprocess.TimeoutExpired as e:
        _child_died.append(switch)
        pytest.fail(f"{switch}: no result after {e.timeout} s: {(e.stdout or b'')[-2000:]}")
    print(f"{switch}: child took {time.perf_counter() - t0:.1f} s: {r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ''}")
    if r.returncode < 0 or "illegal memory access" in r.stdout + r.stderr:   # a GPU fault the child survived counts as well
        _child_died.append(switch)
    n_tests = len(TABLES) + len(S.TREE_SIZES) + len(S.COUNT_PAIRS) + 1 + len(S.SCENES)
    assert r.returncode == 0 and f"{n_tests} passed" in r.stdout, r.stdout[-3000:] + r.stderr[-1500:]


def _dump_tables_main(out_dir):
    """body of the child of test_every_kernel_form_gives_the_same_flag_and_coefficient_bits (own process: ROLO_S2M_PACKETS is read once per process)"""
    g = Scan2Map(edgeFeatureMinValidNum=0, surfFeatureMinValidNum=0)
    for which in TABLES:
        _, st, sel, co = _run(g, TABLES[which][0]()[0])
        np.savez(os.path.join(out_dir, which + ".npz"), sel=sel, coeff=co, stats=np.array([st[k] for k in STAT_FIELDS]))
    g.close()
    print("DUMPED", len(TABLES))


def test_every_kernel_form_gives_the_same_flag_and_coefficient_bits(s2m, tmp_path):
    """both forms find the same five neighbours in the same (d2, index) order, so flags and coefficients are the same FLOATS, not only both within the oracle's bar:
    a child with ROLO_S2M_PACKETS=0 writes them for the three case tables (ties, the d2 == 1 edge, rank-deficient fits), this process runs the default form —
    byte-identical, equal stats. The poses are not compared in bits: the two forms sum their rows over different grids. (The name keeps this test, like the one
    above, out of that test's child runs: a child would compare s2m_kernel with itself.)"""
    assert not _child_died, f"not started: the child for {_child_died[0]} ended on a signal or a timeout"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; sys.path[:0] = [%r, %r]; from tests.test_gpu_backend_cases import _dump_tables_main; _dump_tables_main(%r)" % (root, os.path.join(root, "tests"), str(tmp_path))
    try:
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ROLO_S2M_PACKETS="0"), capture_output=True, text=True, timeout=240, cwd=root)
    except subprocess.TimeoutExpired as e:
        _child_died.append("ROLO_S2M_PACKETS=0 (tables)")
        pytest.fail(f"no result after {e.timeout} s: {(e.stdout or b'')[-2000:]}")
    if r.returncode < 0 or "illegal memory access" in r.stdout + r.stderr:
        _child_died.append("ROLO_S2M_PACKETS=0 (tables)")
    assert r.returncode == 0 and f"DUMPED {len(TABLES)}" in r.stdout, r.stdout[-3000:] + r.stderr[-1500:]
    for which in TABLES:
        scn, names = _table(which)[:2]
        _, st, sel, co = _run(s2m, scn)
        ref = np.load(os.path.join(str(tmp_path), which + ".npz"))
        assert st == dict(zip(STAT_FIELDS, ref["stats"].tolist())), (which, st, ref["stats"])
        assert sel.dtype == ref["sel"].dtype and co.dtype == ref["coeff"].dtype == np.float32 and co.shape == ref["coeff"].shape
        flags = [n for i, n in enumerate(names) if sel[i] != ref["sel"][i]]
        assert not flags and sel.tobytes() == ref["sel"].tobytes(), f"{which}: flags differ between the forms: {flags}"
        bits, ref_bits = np.ascontiguousarray(co).view(np.uint32), np.ascontiguousarray(ref["coeff"]).view(np.uint32)
        diff = [(n, co[i], ref["coeff"][i]) for i, n in enumerate(names) if not np.array_equal(bits[i], ref_bits[i])]
        assert not diff, f"{which}: (case, default form's coefficients, one-walk-per-lane form's) differ in bits: {diff}"
