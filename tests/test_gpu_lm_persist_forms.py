"""GPU: the resident LM kernel (fused_lm = 2, lm_persist.hip lm_persist_kernel) in every launch form it has, against the CPU oracle AND against pass + controller launches.

Which instantiation runs, on how many workgroups, with how many points per thread and whether the Mahalanobis cache sits in LDS follows from the cloud size, the load
(schedule.hip prepare_pass), the optimiser and the neighbour search (lm_persist.hip lm_persist_form) and five environment switches. Each case registers a source cloud of exactly n
points through register_async / register_wait with a pinned load hint and checks:
* lm_form() reports the form the case is there for (a case that silently takes another form fails) — the expected rows below are worked out by hand from
  schedule.hip prepare_pass: threads T = 512, workgroups at most 256 (idle) / 64 (busy), points per thread = ceil(n / (T * max workgroups)) with 3 rounded up to 4,
  rows = ceil(n / (T * points per thread)); dynamic LDS = 240 B per row + 48 B per thread and interleaved point if the cache is on;
* against the oracle (pyorc.Reg align + compute_translation): exits, iteration counts, convergence and the correspondence count equal; every trace record up to the first
  whose decision is rounding noise in order, same decision, y0 / yi to 1e-9; poses and translation to 1e-8;
* against fused_lm = 0 in the same process: the same, poses to 1e-10, and no bail-out of the resident kernel.
The switches are read once per process: the environment cases run in child processes."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyorc
from rolo_amd import synth
from rolo_amd.rotvgicp import RotVGICP, LSQ_OPTIMIZER_TYPE, NeighborSearchMethod, RegularizationMethod

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF = 0.5
G = -np.asarray(synth.PREV_STEP_T, np.float64)
L0 = G * 0.97
GUESS = np.eye(4, dtype=np.float32)
GUESS[:3, :3] = synth.rpy_to_R(0.01, -0.015, np.radians(3.0))
LM6, GN6 = int(LSQ_OPTIMIZER_TYPE.LevenbergMarquardt), int(LSQ_OPTIMIZER_TYPE.GaussNewton)
D7, D27 = int(NeighborSearchMethod.DIRECT7), int(NeighborSearchMethod.DIRECT27)
MIN_EIG = int(RegularizationMethod.MIN_EIG)   # no I - m m^T form: six entries per covariance, through the cache


@functools.lru_cache(maxsize=None)
def clouds():
    """the OS1-128x2048 pair (262 144 points per cloud); the source is extended by jittered copies of itself to go past that (as test_gpu_lm_exits _BIG does)"""
    src, tgt, _ = synth.dense_pair("os1-128x2048", seed=synth.SEED)
    j = np.array([0.013, -0.007, 0.011, 0.0], np.float32)
    return np.concatenate([src, src + j, src - j]), tgt


def source(n):
    big, _ = clouds()
    assert n <= big.shape[0]
    return np.ascontiguousarray(big[:n])


def records(trace):
    return [(r["stage"], r["outer"], r["trial"], r["accepted"], r["y0"], r["yi"]) for r in trace]


@functools.lru_cache(maxsize=None)
def oracle(n, knobs):
    """one oracle solve per (cloud size, knobs); knobs: a sorted tuple of rolo_params / orc_params fields"""
    o = pyorc.Reg(pyorc.default_params(voxel_type=pyorc.VOXEL_UNIFORM, voxel_resolution=LEAF, **dict(knobs)))
    o.set_target(clouds()[1]); o.set_source(source(n))
    rc, _, Td, it, cv = o.align(GUESS)
    nc = int(o.correspondences()[0].shape[0])
    rc_t, t, tit = o.compute_translation(np.zeros(3), G, L0)
    return dict(T=np.asarray(Td).tolist(), t=np.asarray(t).tolist(), rot=[rc, it, int(cv), nc], trans=[rc_t, tit], trace=records(o.trace()))


def run_gpu(n, busy, fused, knobs):
    g = RotVGICP(0); g.setResolution(LEAF); g.setLoadHint(1 if busy else 0)
    for k, v in knobs:
        setattr(g._p, k, v)
    g._p.fused_lm = fused; g._push()
    g.setInputTarget(clouds()[1]); g.setInputSource(source(n))
    g.register_async(GUESS, np.zeros(3), G, L0)
    _, _, t = g.register_wait()
    st, ts = g.last_stats, g.last_translation_stats
    out = dict(T=np.asarray(g.final_transformation_d).tolist(), t=np.asarray(t).tolist(), rot=[st.lm_failed, st.n_outer, int(st.converged), st.n_correspondences],
               trans=[ts.lm_failed, ts.n_outer], passes=[st.n_passes, ts.n_passes], trace=records(g.trace()), form=g.lm_form(), bails=g.counters()["persist_bails"])
    g.close()
    return out


def run_both(n, busy, knobs):
    return {str(f): run_gpu(n, busy, f, knobs) for f in (0, 2)}


def same(a, b, rel):
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return abs(a - b) <= rel * max(abs(a), abs(b), 1e-300)


def check_against(ref, got, pose_tol, what):
    assert got["rot"] == ref["rot"] and got["trans"] == ref["trans"], (what, ref["rot"], got["rot"], ref["trans"], got["trans"])
    dT = np.abs(np.array(got["T"]) - np.array(ref["T"])).max(); dt = np.abs(np.array(got["t"]) - np.array(ref["t"])).max()
    assert dT < pose_tol and dt < pose_tol, (what, dT, dt)
    for stage in (0, 1):
        a = [r for r in ref["trace"] if r[0] == stage]; b = [r for r in got["trace"] if r[0] == stage]
        assert len(b) > 0, (what, stage)
        for ra, rb in zip(a, b):
            if abs(ra[4] - ra[5]) <= 1e-7 * abs(ra[4]):   # a decision inside the rounding noise of the sums: the records after it may differ legitimately
                break
            assert tuple(ra[:4]) == tuple(rb[:4]), (what, ra, rb)
            assert same(ra[4], rb[4], 1e-9) and same(ra[5], rb[5], 1e-9), (what, ra, rb)


def form(rows, threads, ppt, sp, batch, mcache):
    return dict(rows=rows, threads=threads, ppt=ppt, sp=sp, batch=batch, mcache=mcache, lds=240 * rows + (48 * threads * sp if mcache else 0))


def check_case(n, knobs, expect, res):
    a, b = res["0"], res["2"]
    what = (n, knobs, expect)
    assert b["form"] == expect, (what, b["form"])
    assert a["form"] == form(0, 0, 0, 0, 0, 0), a["form"]            # pass + controller launches: no resident launch to report
    assert b["bails"] == 0 and a["bails"] == 0, what
    ref = oracle(n, knobs)
    check_against(ref, a, 1e-8, what + ("fused_lm=0 vs oracle",))
    check_against(ref, b, 1e-8, what + ("fused_lm=2 vs oracle",))
    check_against(a, b, 1e-10, what + ("fused_lm=2 vs fused_lm=0",))
    assert a["passes"] == b["passes"] or any(abs(r[4] - r[5]) <= 1e-7 * abs(r[4]) for r in a["trace"]), (what, a["passes"], b["passes"])


# (id, n, busy, knobs, expected form): the size table — what each row pins is in its id
SIZES = [
    ("idle-one-partial-workgroup", 37, False, (), form(1, 512, 1, 1, 1, 1)),
    ("idle-first-row-boundary", 513, False, (), form(2, 512, 1, 1, 1, 1)),
    ("idle-2ppt-partial-last-row", 131073, False, (), form(129, 512, 2, 2, 2, 1)),
    ("idle-3ppt-rounded-to-4", 262145, False, (), form(129, 512, 4, 4, 2, 1)),
    ("idle-largest-grid-under-144k", 417792, False, (), form(204, 512, 4, 4, 2, 1)),
    ("idle-band-lo", 417793, False, (), form(205, 512, 4, 4, 2, 1)),
    ("idle-band-mid", 430000, False, (), form(210, 512, 4, 4, 2, 1)),
    ("idle-band-hi", 452608, False, (), form(221, 512, 4, 4, 2, 1)),
    ("idle-fits-edge-no-cache", 452609, False, (), form(222, 512, 4, 4, 2, 0)),
    ("idle-generic-above-524288", 600000, False, (), form(235, 512, 5, 0, 1, 0)),
    ("busy-2ppt", 32769, True, (), form(33, 512, 2, 2, 2, 1)),
    ("busy-3ppt-rounded-to-4", 65537, True, (), form(33, 512, 4, 4, 2, 1)),
    ("busy-generic-5ppt", 131073, True, (), form(52, 512, 5, 0, 1, 0)),
    ("busy-generic-8ppt", 262144, True, (), form(64, 512, 8, 0, 1, 0)),
    ("busy-generic-19ppt", 600000, True, (), form(62, 512, 19, 0, 1, 0)),
]
# configuration cases at 131 072 points: idle 256 x 1, busy 64 x 4
N = 131072
CONFIGS = [
    ("lm6-idle", False, (("optimizer", LM6),), form(256, 512, 1, 0, 1, 0)),
    ("lm6-busy", True, (("optimizer", LM6),), form(64, 512, 4, 0, 1, 0)),
    ("gn6-idle", False, (("optimizer", GN6),), form(256, 512, 1, 0, 1, 0)),
    ("gn6-busy", True, (("optimizer", GN6),), form(64, 512, 4, 0, 1, 0)),
    ("direct7-idle", False, (("neighbor_search", D7),), form(256, 512, 1, 0, 1, 0)),
    ("direct7-busy", True, (("neighbor_search", D7),), form(64, 512, 4, 0, 1, 0)),
    ("direct27-busy", True, (("neighbor_search", D27),), form(64, 512, 4, 0, 1, 0)),
    ("min-eig-idle", False, (("regularization", MIN_EIG),), form(256, 512, 1, 1, 1, 1)),
    ("min-eig-busy", True, (("regularization", MIN_EIG),), form(64, 512, 4, 4, 2, 1)),
    ("q2-intended-idle", False, (("q2_intended", 1),), form(256, 512, 1, 1, 1, 1)),
    ("q2-intended-busy", True, (("q2_intended", 1),), form(64, 512, 4, 4, 2, 1)),
]


@pytest.mark.parametrize("n,busy,knobs,expect", [c[1:] for c in SIZES], ids=[c[0] for c in SIZES])
def test_resident_form_by_cloud_size(n, busy, knobs, expect):
    check_case(n, knobs, expect, run_both(n, busy, knobs))


@pytest.mark.parametrize("busy,knobs,expect", [c[1:] for c in CONFIGS], ids=[c[0] for c in CONFIGS])
def test_resident_form_by_configuration(busy, knobs, expect):
    check_case(N, knobs, expect, run_both(N, busy, knobs))


# environment cases: (id, environment, [(n, busy, knobs, expected form)]) — one child process each
ENVS = [
    ("batch-1", dict(ROLO_LM_PERSIST_BATCH="1"), [(N, True, (), form(64, 512, 4, 4, 1, 1)), (452609, False, (), form(222, 512, 4, 4, 2, 0))]),
    ("batch-1-no-cache", dict(ROLO_LM_PERSIST_BATCH="1", ROLO_LM_PERSIST_MCACHE="0"), [(N, True, (), form(64, 512, 4, 4, 2, 0))]),
    ("batch-4", dict(ROLO_LM_PERSIST_BATCH="4"), [(N, True, (), form(64, 512, 4, 4, 4, 1)), (452609, False, (), form(222, 512, 4, 4, 2, 0))]),
    # 256 threads: at most 128 workgroups; at 65 536 points that is 2 points per thread, which has no 256-thread form: back to 512 threads
    ("busy-threads-256", dict(ROLO_LM_PERSIST_BUSY_THREADS="256"), [(N, True, (), form(128, 256, 4, 4, 2, 1)), (65536, True, (), form(64, 512, 2, 2, 2, 1))]),
    ("no-interleave", dict(ROLO_LM_PERSIST_INTERLEAVE="0"), [(N, False, (), form(256, 512, 1, 0, 1, 0)), (N, True, (), form(64, 512, 4, 0, 1, 0))]),
    ("no-cache", dict(ROLO_LM_PERSIST_MCACHE="0"), [(N, True, (), form(64, 512, 4, 4, 2, 0)), (N, False, (), form(256, 512, 1, 1, 1, 1))]),
    # grids that are not a multiple of 8 (pass_xcd_block deals them unevenly over the XCDs) at 20 / 32 points per thread
    ("wgs-13", dict(ROLO_LM_PERSIST_WGS="13"), [(N, False, (), form(13, 512, 20, 0, 1, 0)), (N, True, (), form(13, 512, 20, 0, 1, 0))]),
    ("wgs-8", dict(ROLO_LM_PERSIST_WGS="8"), [(N, False, (), form(8, 512, 32, 0, 1, 0)), (N, True, (), form(8, 512, 32, 0, 1, 0))]),
    ("no-xcd-map", dict(ROLO_PASS_XCD="0"), [(N, False, (), form(256, 512, 1, 1, 1, 1)), (N, True, (), form(64, 512, 4, 4, 2, 1)),
                                              (600000, False, (), form(235, 512, 5, 0, 1, 0))]),
]

_CHILD = r"""
import sys, json
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_lm_persist_forms as m
cases = json.loads(sys.argv[2])
print(json.dumps([m.run_both(n, busy, tuple(tuple(kv) for kv in knobs)) for n, busy, knobs in cases]))
"""


@pytest.mark.parametrize("env,cases", [e[1:] for e in ENVS], ids=[e[0] for e in ENVS])
def test_resident_form_by_environment_switch(env, cases):
    arg = json.dumps([(n, busy, knobs) for n, busy, knobs, _ in cases])
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, arg], capture_output=True, text=True, env=dict(os.environ, **env), cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(out) == len(cases)
    for (n, busy, knobs, expect), res in zip(cases, out):
        check_case(n, knobs, expect, res)
