"""GPU: extract_kernel on the constructed rings of tests/front_rings.py, loaded as arrays (rolo_front_load_projection), against the C++ oracle on the same arrays —
bit for bit on curvature, picked, label, corner and surface — and the path every ring took (rolo_debug_extract_paths) against the path its case demands. That the oracle's
answers are shared by the independent numpy twin, and that the cases sit where they claim to, is shown on the CPU (tests/test_front_rings_twin.py)."""
import functools

import numpy as np
import pytest

import front_rings as R
from oracle import pyorc
from rolo_amd import synth
from rolo_amd.frontend import FrontEnd, front_params
from rolo_amd.rotvgicp import RotVGICP

pytestmark = pytest.mark.gpu

OUTPUTS = ("curvature", "picked", "label", "corner", "surface")


@functools.lru_cache(maxsize=None)
def oracle(name):
    c = R.CASES[name]
    return pyorc.extract_features(pyorc.front_params(**R.params(c)), c["proj"])


def load_and_extract(g, c):
    """(outputs, path words) of one case on the context g"""
    fe = FrontEnd(g, front_params(**R.params(c)))
    n = fe.loadProjection(c["proj"])
    return fe.extract(n, debug=True), fe.extractPaths()


def hold_equal(got, want, what):
    for k in OUTPUTS:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
    for k in OUTPUTS:
        assert np.array_equal(got[k], want[k]), (what, k, np.nonzero(np.atleast_1d((got[k] != want[k]).reshape(got[k].shape[0], -1).any(axis=1)))[0][:8])


def hold_paths(paths, c):
    bad = {r: (int(paths[r]), w) for r, w in c["expect_paths"].items() if int(paths[r]) != w}
    assert not bad, f"{c['name']}: ring -> (path word taken, expected): {bad}"


@pytest.mark.parametrize("name", list(R.CASES))
def test_constructed_rings_match_the_oracle_and_take_their_path(name):
    c = R.CASES[name]
    g = RotVGICP()
    try:
        got, paths = load_and_extract(g, c)
        assert paths.shape == (c["n_scan"],)
        hold_equal(got, oracle(name), name)
        hold_paths(paths, c)
        again, paths2 = load_and_extract(g, c)   # the context now holds this case's own marks, labels and staging
        for k in OUTPUTS:
            assert again[k].tobytes() == got[k].tobytes(), k
        assert np.array_equal(paths2, paths)
    finally:
        g.close()


def test_one_context_through_sizes_forms_and_entry_points():
    """One context takes a large case, a small one, the scratch form, the LDS form again, a projected frame and a loaded case: each step gives what a fresh context gives.
    What could go wrong between them: staging rows and scratch of a longer ring left behind, the marks of the previous cloud where nobody cleared them (extract_cleared: a
    projection clears for the extraction that follows, a load does not), the switch between the LDS and the scratch kernel and their staging pitch. (The third flag,
    precleared_np, lives on the odometry driver's private front-end context, which takes no loaded projection: tests/test_gpu_pipeline.py.)"""
    fr = synth.make_frame("vlp16", np.eye(3), np.zeros(3), synth.SEED)
    cfg = dict(n_scan=16, horizon_scan=1800)

    def projected(g):
        fe = FrontEnd(g, front_params(**cfg))
        pg = fe.project(fr.xyz, fr.ring)
        return fe.extract(pg["n"], debug=True), fe.extractPaths()

    steps = ["const_16", "cloud_n11", "big_cap", "saw_cap", None, "thr_edge_neg", "vox_own_cell", "big_edge_neg", "pops_small"]
    fresh = []
    for name in steps:
        g = RotVGICP()
        try:
            fresh.append(projected(g) if name is None else load_and_extract(g, R.CASES[name]))
        finally:
            g.close()
    g = RotVGICP()
    try:
        for name, (want, want_paths) in zip(steps, fresh):
            got, paths = projected(g) if name is None else load_and_extract(g, R.CASES[name])
            hold_equal(got, want, f"step {name}")
            assert np.array_equal(paths, want_paths), name
            if name is not None:
                hold_equal(got, oracle(name), f"step {name} against the oracle")
                hold_paths(paths, R.CASES[name])
        po = pyorc.project(pyorc.front_params(**cfg), fr.xyz, fr.ring)
        hold_equal(fresh[4][0], pyorc.extract_features(pyorc.front_params(**cfg), po), "the projected frame against the oracle")
    finally:
        g.close()


def test_paths_need_an_extraction():
    from rolo_amd._lib import RoloError
    g = RotVGICP()
    try:
        c = R.CASES["head_22"]
        fe = FrontEnd(g, front_params(**R.params(c)))
        with pytest.raises(RoloError) as ei:
            fe.extractPaths()
        assert ei.value.code == -5           # ROLO_ESTATE: nothing extracted yet
        n = fe.loadProjection(c["proj"])
        with pytest.raises(RoloError) as ei:
            fe.extractPaths()
        assert ei.value.code == -5           # ... a projection alone is not one
        fe.extract(n)
        first = fe.extractPaths()
        assert first.shape == (2,)
        fe.loadProjection(c["proj"])
        with pytest.raises(RoloError) as ei:
            fe.extractPaths()
        assert ei.value.code == -5           # a new projection forgets the previous extraction's paths
        fe.extract(n)
        assert np.array_equal(fe.extractPaths(), first)
        other = FrontEnd(g, front_params(**dict(R.params(c), n_scan=3)))
        with pytest.raises(RoloError) as ei:
            other.extractPaths()
        assert ei.value.code == -1           # ROLO_EINVAL: not the n_scan of the projection the extraction ran on
    finally:
        g.close()
