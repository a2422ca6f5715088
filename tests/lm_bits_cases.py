"""The LM chain's recorded bits (tests/golden/lm_forms_bits.npz): the cases, the runner and the record's layout. Shared by the recorder
(profiles/tools/record_lm_bits.py) and tests/test_gpu_lm_bits.py.

The three launch forms of the LM iteration (pass + controller launches, one launch per trial, the resident kernel) are held to each other and to the oracle at 1e-8 to
1e-10 by the form tests; a reordered sum or a product that is no longer fused moves the last bit only and passes them all. The record holds the bytes instead: the
smallest clouds that reach each code path — every points-per-thread form of the resident kernel's bodies, its cache-less and 256-thread forms, the six-entry
covariances, the generic controller, the batch wrapper, the stage-level evaluations and a stand-alone translation stage.

Everything comes from synth.dense_pair("os1-64") (65 536 points): the target is the whole target cloud, the source its first n points; guess and translation inputs are
those of test_gpu_lm_persist_forms.py. The switches are read once per process, so each environment is one child process (run_child)."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

FILE = "lm_forms_bits.npz"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF = 0.5
WGS8 = dict(ROLO_LM_PERSIST_WGS="8")   # 8 workgroups of 512 threads: points per thread = ceil(n / 4096), 3 rounded up to 4
# n -> points per thread at 8 x 512: 1, 2, 3 (rounded to 4), 4, 5 (the generic body)
SIZES = ((4059, 1), (8155, 2), (12001, 4), (16347, 4), (20011, 5))
ZERO_FORM = dict(rows=0, threads=0, ppt=0, sp=0, batch=0, mcache=0, lds=0)   # pass + controller launches, one launch per trial: no resident launch to report


def knob_sets():
    from rolo_amd.rotvgicp import LSQ_OPTIMIZER_TYPE as O, NeighborSearchMethod as N, RegularizationMethod as R
    so3, lm6, gn6 = int(O.SO3_LevenbergMarquardt), int(O.LevenbergMarquardt), int(O.GaussNewton)
    d1, d7 = int(N.DIRECT1), int(N.DIRECT7)
    # six-entry covariances (no I - m m^T form) come from NORMALIZED_MIN_EIG, not MIN_EIG: MIN_EIG's entries are unbounded, so the voxel map sums them with
    # floating-point atomics (api.hip voxel_fixed_cov) and the map — with everything after it — is not the same bits from run to run; the bounded regularisations
    # go through fixed point and are
    nme = int(R.NORMALIZED_MIN_EIG)
    # name -> (knobs, interleaved bodies?): lm_persist_form takes the interleaved bodies (and the Mahalanobis cache) for the SO(3) optimiser with DIRECT1 only
    return {
        "so3-d1-plane": ((("optimizer", so3), ("neighbor_search", d1), ("regularization", int(R.PLANE))), True),     # interleaved bodies, the m form of the covariance
        "lm6-d7": ((("optimizer", lm6), ("neighbor_search", d7)), False),                                             # the generic body and rot_step_t<6>
        "gn6-d1-nmineig": ((("optimizer", gn6), ("neighbor_search", d1), ("regularization", nme)), False),            # Gauss-Newton, six-entry covariances, generic body
        "so3-d1-nmineig": ((("optimizer", so3), ("neighbor_search", d1), ("regularization", nme)), True),             # six-entry covariances through the cache
    }


def form(rows, threads, ppt, sp, batch, mcache):
    """as test_gpu_lm_persist_forms.form: dynamic LDS = 240 B per row + 48 B per thread and interleaved point if the cache is on"""
    return dict(rows=rows, threads=threads, ppt=ppt, sp=sp, batch=batch, mcache=mcache, lds=240 * rows + (48 * threads * sp if mcache else 0))


def expected_form(n, ppt, interleaved):
    """the resident launch of n points on 512-thread workgroups at `ppt` points per thread (lm_persist_form, worked out by hand as in test_gpu_lm_persist_forms.py):
    interleaved bodies with the cache at 1, 2 and 4 points per thread (four go through in batches of 2), the generic body otherwise"""
    rows = -(-n // (512 * ppt))
    if not interleaved or ppt not in (1, 2, 4):
        return form(rows, 512, ppt, 0, 1, 0)
    return form(rows, 512, ppt, ppt, 2 if ppt == 4 else ppt, 1)


# environment name -> (environment, what runs in it); every environment has ROLO_LM_PERSIST_WGS=8
ENVS = {
    "wgs8": dict(WGS8),
    "wgs8-no-cache": dict(WGS8, ROLO_LM_PERSIST_MCACHE="0"),
    "wgs8-busy-256": dict(WGS8, ROLO_LM_PERSIST_BUSY_THREADS="256"),
    "wgs8-no-nrm": dict(WGS8, ROLO_PASS_NRM="0"),
    "wgs8-ctrl-generic": dict(WGS8, ROLO_CTRL_GENERIC="1"),
}
N_CASES = {"wgs8": 5 * 3 * 4 + 2 + 1 + 2, "wgs8-no-cache": 2, "wgs8-busy-256": 2, "wgs8-no-nrm": 8, "wgs8-ctrl-generic": 8}


def _inputs():
    from rolo_amd import synth
    from test_gpu_lm_persist_forms import G, GUESS, L0
    src, tgt, _ = synth.dense_pair("os1-64", seed=synth.SEED)
    return src, tgt, G, GUESS, L0


def _operator(tgt, src, knobs, fused, busy=False):
    from rolo_amd.rotvgicp import RotVGICP
    g = RotVGICP(0); g.setResolution(LEAF); g.setLoadHint(1 if busy else 0)
    for k, v in knobs:
        setattr(g._p, k, v)
    g._p.fused_lm = fused; g._push()
    g.setInputTarget(tgt); g.setInputSource(src)
    return g


def _ints(g):
    st, ts, c, f = g.last_stats, g.last_translation_stats, g.counters(), g.lm_form()
    z = [0] * 6
    return ([st.lm_failed, st.n_outer, st.converged, st.n_passes, st.n_correspondences, st.n_cost_only] if st is not None else z) + \
           ([ts.lm_failed, ts.n_outer, ts.converged, ts.n_passes, ts.n_correspondences, ts.n_cost_only] if ts is not None else z) + \
           [c["kept_trials"], c["model_trials"], c["persist_bails"]] + [f[k] for k in ("rows", "threads", "ppt", "sp", "batch", "mcache", "lds")]


def _case(name, g, T, t, extra=()):
    return dict(name=name, T=np.asarray(T, np.float64).reshape(16), t=np.asarray(t, np.float64).reshape(3), ints=_ints(g), trace=g.trace(), extra=list(extra))


def _register(name, tgt, src, knobs, fused, want_form, busy, G, GUESS, L0):
    g = _operator(tgt, src, knobs, fused, busy)
    g.register_async(GUESS, np.zeros(3), G, L0)
    _, Td, t = g.register_wait()
    got = g.lm_form()
    assert got == want_form, (name, got, want_form)   # a case that drifts to another form fails rather than passes
    assert g.counters()["persist_bails"] == 0, name
    out = _case(name, g, Td, t)
    g.close()
    return out


def run(env_name):
    """every case of one environment, in this process (whose environment must be ENVS[env_name]): a list of case records"""
    for k, v in ENVS[env_name].items():
        assert os.environ.get(k) == v, (k, "run() belongs in a child process started with the environment's switches: run_child")
    src, tgt, G, GUESS, L0 = _inputs()
    sets = knob_sets()
    first = lambda n: np.ascontiguousarray(src[:n])
    out = []
    if env_name == "wgs8":
        for n, ppt in SIZES:
            for fused in (0, 1, 2):
                for sname, (knobs, inter) in sets.items():
                    want = expected_form(n, ppt, inter) if fused == 2 else ZERO_FORM
                    out.append(_register("n %d fused %d %s" % (n, fused, sname), tgt, first(n), knobs, fused, want, False, G, GUESS, L0))
        # a batch of two members through the batch wrapper (rot_pass_batch_kernel, ctrl_batch_kernel, frame_begin_batch_kernel)
        from rolo_amd.rotvgicp import RotVGICPBatch
        b = RotVGICPBatch(2)
        for m, n in zip(b.members, (4059, 8155)):
            m.setResolution(LEAF); m.setLoadHint(0); m.setInputTarget(tgt); m.setInputSource(first(n))
        b.register_async(np.stack([GUESS, GUESS]), np.zeros((2, 3)), np.tile(G, (2, 1)), np.tile(L0, (2, 1)))
        _, Td, t = b.register_wait()
        for i, m in enumerate(b.members):
            out.append(_case("batch member %d" % i, m, Td[i], t[i]))
        b.close()
        # the stage-level evaluation calls of test_gpu_registration.py::test_linearize_stages (eval_begin_kernel, t3_eval_begin_kernel), at its poses
        from rolo_amd import synth
        g = _operator(tgt, first(8155), (), 0)
        T = np.eye(4); T[:3, :3] = synth.rpy_to_R(0.004, -0.007, 0.02)
        T2 = np.eye(4); T2[:3, :3] = synth.rpy_to_R(0.0045, -0.0065, 0.021)
        tp = np.array([0.01, -0.004, 0.002])
        T6 = T.copy(); T6[:3, 3] = (0.01, -0.02, 0.005)
        extra = []
        e, H, bb = g.so3_linearize(T); extra += [e] + H.ravel().tolist() + bb.tolist()
        extra.append(g.compute_error(T2))
        e, H, bb = g.t3_linearize(tp, G, L0); extra += [e] + H.ravel().tolist() + bb.tolist()
        extra.append(g.compute_t_error(tp, G, L0))
        e, H, bb = g.linearize(T6); extra += [e] + H.ravel().tolist() + bb.tolist()
        c = _case("stage-level evaluations", g, np.zeros(16), np.zeros(3), extra)
        c["trace"] = []   # no LM chain ran on this context: nothing has set its trace count
        out.append(c)
        g.close()
        # a stand-alone compute_translation after align (trans_begin_kernel)
        for fused in (0, 2):
            g = _operator(tgt, first(8155), (), fused)
            g.align(GUESS)
            Td = np.array(g.final_transformation_d)
            tr_rot = g.trace()
            t = g.computeTranslation(np.zeros(3), G, L0)
            c = _case("align then compute_translation fused %d" % fused, g, Td, t)
            c["trace"] = tr_rot + c["trace"]
            out.append(c)
            g.close()
    elif env_name in ("wgs8-no-cache", "wgs8-busy-256"):
        n = 16347
        for sname in ("so3-d1-plane", "so3-d1-nmineig"):
            want = form(8, 512, 4, 4, 2, 0) if env_name == "wgs8-no-cache" else form(16, 256, 4, 4, 2, 1)   # 256 threads: twice the workgroups, ceil(16347 / 1024) = 16 rows
            out.append(_register("n %d busy fused 2 %s" % (n, sname), tgt, first(n), sets[sname][0], 2, want, True, G, GUESS, L0))
    else:
        n = 4059
        for fused in (0, 2):
            for sname, (knobs, inter) in sets.items():
                out.append(_register("n %d fused %d %s" % (n, fused, sname), tgt, first(n), knobs, fused, expected_form(n, 1, inter) if fused == 2 else ZERO_FORM, False, G, GUESS, L0))
    assert len(out) == N_CASES[env_name], (env_name, len(out))
    return pack(out)


def pack(cases):
    """the record's arrays: case k's trace records at trace_start[k] : trace_start[k + 1], its further values (the stage-level evaluations' e, H, b) at extra_start[k] : extra_start[k + 1]"""
    ti, tf, ts, ex, es = [], [], [0], [], [0]
    for c in cases:
        for r in c["trace"]:
            ti.append([r["stage"], r["outer"], r["trial"], r["accepted"]])
            tf.append([r["y0"], r["yi"], r["rho"], r["lam"], r["dnorm"]])
        ts.append(len(ti)); ex += c["extra"]; es.append(len(ex))
    return dict(names=np.array([c["name"] for c in cases]), Td=np.array([c["T"] for c in cases], np.float64).reshape(-1, 4, 4), t=np.array([c["t"] for c in cases], np.float64).reshape(-1, 3),
                # rotation stage, translation stage: lm_failed, n_outer, converged, n_passes, n_correspondences, n_cost_only; kept, modelled, bails; lm_form()
                ints=np.array([c["ints"] for c in cases], np.int32).reshape(-1, 22), trace_start=np.array(ts, np.int64),
                trace_ints=np.array(ti, np.int32).reshape(-1, 4), trace_y0_yi_rho_lambda_dnorm=np.array(tf, np.float64).reshape(-1, 5),
                extra_start=np.array(es, np.int64), extra=np.array(ex, np.float64))


def raw(a):
    """an array as its bytes: a NaN equals itself, a negative zero differs from a positive one"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.kind in "fiu" else a


def differences(a, b):
    """the arrays of two records that are not the same bytes, each with the first rows that differ"""
    if sorted(a) != sorted(b):
        return [("keys", sorted(a), sorted(b))]
    out = []
    for k in a:
        if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape:
            out.append((k, a[k].dtype, a[k].shape, b[k].dtype, b[k].shape))
        elif not np.array_equal(raw(a[k]), raw(b[k])):
            out.append((k, np.flatnonzero(np.any((raw(a[k]) != raw(b[k])).reshape(len(a[k]), -1), axis=1))[:8].tolist()))
    return out


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import lm_bits_cases as m
rec = m.run(sys.argv[2])
for _ in range(int(sys.argv[4]) - 1):
    again = m.run(sys.argv[2])
    if m.differences(rec, again):
        raise SystemExit("not reproducible from run to run: %s %s" % (sys.argv[2], m.differences(rec, again)))
np.savez(sys.argv[3], **rec)
"""


def run_child(env_name, runs=1, timeout=300):
    """run(env_name) in a fresh process with the environment's switches; runs = 2: twice in that process, and the child fails if the two differ"""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "rec.npz")
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, env_name, out, str(runs)], capture_output=True, text=True, env=dict(os.environ, **ENVS[env_name]), cwd=ROOT, timeout=timeout)
        if r.returncode != 0:
            raise RuntimeError("%s: exit %d\n%s" % (env_name, r.returncode, (r.stdout + r.stderr)[-3000:]))
        with np.load(out) as z:
            return {k: z[k] for k in z.files}


def key(env_name, k):
    return env_name + "/" + k
