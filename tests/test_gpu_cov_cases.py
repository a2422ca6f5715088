"""GPU: the covariance stage (K5's second half: the moments epilogue / knn_neighbourhood_moments, jacobi_svd3, knn_covariance_finish and the four tail forms) on the
constructed clusters of tests/cov_cases.py against EXACT arithmetic, and the PLANE short form C_A = I - m m^T with its three readers (rotated_cov of the pass kernels,
the lm_kernel loads, lmp_rotated_cov of the resident kernel).

The covariances: 6 rules x k = 20, 7, 33, 100 x the `regular` and `mixed` clouds, source and target; every assertion of the statement (cov_cases.check_covariances).
The bar per rule is 10 x the oracle's recorded deviation from exact arithmetic, floored at 8 * 2^-53, relative to the largest |entry| — read from the fixture
(tests/golden/cov_cases.npz), never from the device. Kernel and oracle run the same operations in the same order with correctly rounded sqrt and division and no
contraction; the 10 covers the order of the few places that are not stated (the 3 x 3 products), not another algorithm. Every member of a cluster must be within the bar
of the exact matrix, which bounds the spread inside a cluster too; the device's own k lists must stay inside the cluster (the premise).
Each kernel form runs in a child process of its own (the switches are read once per process): ROLO_KNN_MOMENTS = 1, = 0, and = 1 with ROLO_KNN_SUB = 0.

The plane form: on `mixed` at k = 20 every source point has either a finite m with |(I - m m^T) - C6| <= 8 * 2^-53, or a NaN in m.x and six entries whose eigenvalues
are NOT (1, 1, +-1e-3); W, T2 and R2 are all finite. Then, with a well-conditioned handed-in target (4 I + S) and the device's own six-entry source covariances on the
oracle's side, so3_linearize / linearize / compute_error at the identity and at a float32 rotation of ~0.01 rad taken as it is (rotated_cov's R R^T term), at
test_linearize_stages' bars, and align under setFusedLm(0), (1), (2) at check_solve's bars — with the default switches and again with ROLO_PASS_NRM = 0."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 240


def _cov_main():
    """body of test_covariances_against_exact_arithmetic (own process)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cov_cases as cc
    from rolo_amd.rotvgicp import RotVGICP
    cases, dev = cc.load()
    bars = cc.bars(dev)
    worst = np.zeros(6)
    signs = {r: {1: 0, -1: 0} for r in range(6)}
    failed = []
    for cloud in cc.CLOUDS:
        for k in cc.KS:
            s, t = cases[(cloud, k, "src")], cases[(cloud, k, "tgt")]
            for rule in range(6):
                g = RotVGICP(); g.setResolution(1.0); g.setCorrespondenceRandomness(k); g.setRegularizationMethod(rule)
                g.setInputTarget(t.xyz1); g.setInputSource(s.xyz1)
                g.computeCovariances()
                got = (g.getSourceCovariances(), g.getTargetCovariances())
                if rule == cc.PLANE:   # the premise, on the device's own lists
                    for which, c in ((0, s), (1, t)):
                        assert cc.knn_inside_clusters(c, g.knn(which)[0]), "%s: a neighbour list leaves its cluster" % c.key
                g.close()
                ref = cc.oracle_covariances(rule, k, s.pts, t.pts)
                for c, cov, r in zip((s, t), got, ref):
                    assert (cov[:, 3, :] == 0).all() and (cov[:, :, 3] == 0).all()
                    try:
                        w, sg = cc.check_covariances(c, rule, cov[:, :3, :3], bars[rule], ref=r)
                    except AssertionError as ex:   # (every cloud and rule is compared and printed before the test fails)
                        failed.append(str(ex)); print("FAILED", ex, flush=True)
                        continue
                    worst[rule] = max(worst[rule], w); signs[rule][1] += sg[1]; signs[rule][-1] += sg[-1]
                print("COV %-8s k=%-3d %-20s worst ratio so far %.3f" % (cloud, k, cc.RULES[rule], worst[rule]), flush=True)
    for rule in range(6):
        print("WORST %-20s bar %.3e  worst ratio to the bar %.3f  R2 signs +1: %d  -1: %d" % (cc.RULES[rule], bars[rule], worst[rule], signs[rule][1], signs[rule][-1]))
    assert not failed, "%d clouds x rules miss the statement:\n%s" % (len(failed), "\n".join(failed[:6]))
    print("COV_CASES_OK")


FORMS = {"moments": dict(ROLO_KNN_MOMENTS="1"), "indices": dict(ROLO_KNN_MOMENTS="0"), "moments-packets": dict(ROLO_KNN_MOMENTS="1", ROLO_KNN_SUB="0")}


def _child(body, env_extra):
    env = dict(os.environ)
    for k in ("ROLO_KNN_MOMENTS", "ROLO_KNN_SUB", "ROLO_PASS_NRM"):
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); from tests.test_gpu_cov_cases import %s; %s()" % (ROOT, body, body)],
                       env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=ROOT)
    print(r.stdout[-6000:])
    assert r.returncode == 0, "child exit status %d\n" % r.returncode + r.stdout[-4000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("form", list(FORMS))
def test_covariances_against_exact_arithmetic(form):
    assert "COV_CASES_OK" in _child("_cov_main", FORMS[form])


# ---------------------------------------------------------------- the plane form and its readers ----------------------------------------------------------------
def _near(c):
    """the clusters of a cloud within +-60 m (no 40 m cluster): each inside one 1 m voxel"""
    keep = c.near[c.owner]
    return np.ascontiguousarray(c.xyz1[keep]), c.pcls[keep]


def _target_covs(n):
    """4 I + S, S a seeded symmetric positive definite matrix of norm <= 0.5"""
    rng = np.random.default_rng(20261020)
    A = rng.standard_normal((n, 3, 3))
    S = A @ np.swapaxes(A, 1, 2)
    S *= (0.5 * rng.random(n) / np.linalg.norm(S, 2, axis=(1, 2)))[:, None, None]
    C = np.zeros((n, 4, 4)); C[:, :3, :3] = 4.0 * np.eye(3) + S
    return C


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def _plane_main():
    """body of test_plane_form_and_its_readers (own process)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cov_cases as cc
    from oracle import pyorc
    from rolo_amd import synth
    from rolo_amd._lib import RoloError
    from rolo_amd.rotvgicp import NeighborSearchMethod, RotVGICP
    from tests.test_gpu_registration import rot_angle
    cases, _ = cc.load()
    s, t = cases[("mixed", 20, "src")], cases[("mixed", 20, "tgt")]
    nrm_on = os.environ.get("ROLO_PASS_NRM", "1") != "0"
    errs = []   # every figure is printed before the test fails

    def expect(ok, msg):
        if not ok:
            errs.append(msg); print("FAILED", msg, flush=True)

    # ---- the read-back and the identity, on the whole `mixed` cloud — and once more with the target's 800 points as the source: three of its collinear points leave the
    # sweep with a sign fix on the second column, so the poisoned side of the rule is there as well
    def identity(a, b, tag, states):
        g = RotVGICP(); g.setResolution(1.0); g.setInputTarget(b.xyz1); g.setInputSource(a.xyz1)
        if states:
            with pytest.raises(RoloError):
                g.sourcePlaneForm()                 # not computed
        g.computeCovariances()
        if not nrm_on:
            with pytest.raises(RoloError):
                g.sourcePlaneForm()                 # the passes read the six entries always
            g.close()
            return
        m = g.sourcePlaneForm()
        C6 = g.getSourceCovariances()[:, :3, :3]
        finite = np.isfinite(m[:, 0])
        assert np.isfinite(m[:, 1:]).all() and np.isfinite(C6).all()
        ident = np.abs((np.eye(3)[None] - m[:, :, None] * m[:, None, :]) - C6).max((1, 2))
        ev = np.linalg.eigvalsh(C6)             # ascending, from the six entries alone
        is_plane = (np.abs(ev[:, 1:] - 1.0).max(1) <= 1e-12) & (np.abs(np.abs(ev[:, 0]) - 1e-3) <= 1e-12)
        for cl in range(7):
            sel = a.pcls == cl
            print("PLANE_FORM %s %-2s points %3d  finite m %3d  poisoned %3d  worst |(I - m m^T) - C6| %.3e" % (
                tag, cc.CLASSES[cl], sel.sum(), (sel & finite).sum(), (sel & ~finite).sum(), ident[sel & finite].max() if (sel & finite).any() else 0.0), flush=True)
        bad = finite & ~(ident <= cc.FLOOR)
        expect(not bad.any(), "%s: plane-form points whose six entries are not I - m m^T: %s (classes %s), worst %.3e" % (tag, np.nonzero(bad)[0][:8], a.pcls[bad][:8], ident[bad].max() if bad.any() else 0.0))
        over = ~finite & is_plane
        expect(not over.any(), "%s: poisoned points whose six entries are a plane form: %s (classes %s)" % (tag, np.nonzero(over)[0][:8], a.pcls[over][:8]))
        expect(finite[np.isin(a.pcls, (cc.W, cc.T2, cc.R2))].all(), "%s: a W, T2 or R2 point is poisoned" % tag)
        if states:
            g.setRegularizationMethod(cc.MIN_EIG); g.computeCovariances()
            with pytest.raises(RoloError):
                g.sourcePlaneForm()                 # not PLANE
            g.setRegularizationMethod(cc.PLANE)
            g.setSourceCovariances(np.pad(C6, ((0, 0), (0, 1), (0, 1))))
            with pytest.raises(RoloError):
                g.sourcePlaneForm()                 # handed-in covariances
        g.close()

    identity(s, t, "source", True)
    identity(t, s, "target-as-source", False)

    # ---- the readers: clusters within +-60 m, a well-conditioned handed-in target, the device's own six entries on the oracle's side. Twice: the fixture's source on
    # its target (every point of the plane form), and the roles swapped (poisoned points among those that find a voxel: the six-entry branch of the three readers)
    R32 = synth.rpy_to_R(0.004, -0.007, 0.006).astype(np.float32)       # ~0.01 rad, float32, NOT re-orthonormalised
    assert 0.009 < np.linalg.norm([0.004, -0.007, 0.006]) < 0.011 and np.abs(R32.astype(np.float64) @ R32.astype(np.float64).T - np.eye(3)).max() > 0
    guess = np.eye(4, dtype=np.float32); guess[:3, :3] = R32

    def readers(A, B, tag, want_poisoned):
        src, _ = _near(A)
        tgt, _ = _near(B)
        CT = _target_covs(tgt.shape[0])

        def both(fused):
            g = RotVGICP(); g.setResolution(1.0); g.setFusedLm(fused); g.setNeighborSearchMethod(NeighborSearchMethod.DIRECT7)
            g.setInputTarget(tgt); g.setInputSource(src)
            g.computeCovariances()
            CS = g.getSourceCovariances()
            ev = np.linalg.eigvalsh(CS[:, :3, :3])
            assert np.isfinite(CS).all() and ev.min() >= -1 - 1e-12 and ev.max() <= 1 + 1e-12, (ev.min(), ev.max())   # so C_B + R C_A R^T >= 2.5 I whatever the null spaces did
            poisoned = ~np.isfinite(g.sourcePlaneForm()[:, 0]) if nrm_on else np.zeros(src.shape[0], bool)
            g.setTargetCovariances(CT)
            o = pyorc.Reg(pyorc.default_params(voxel_type=pyorc.VOXEL_UNIFORM, voxel_resolution=1.0, neighbor_search=pyorc.DIRECT7))
            o.set_target(tgt); o.set_source(src)
            o.set_source_covs(CS); o.set_target_covs(CT)
            return o, g, poisoned

        o, g, poisoned = both(0)
        for name, T in (("identity", np.eye(4)), ("float32 rotation", guess.astype(np.float64))):
            for fn in ("so3_linearize", "linearize"):
                eo, Ho, bo = getattr(o, fn)(T)
                eg, Hg, bg = getattr(g, fn)(T)
                print("STAGE %s %-16s %-13s error %.6e  rel: error %.2e  H %.2e  b %.2e" % (tag, name, fn, eo, abs(eg - eo) / abs(eo), _rel(Hg, Ho), _rel(bg, bo)), flush=True)
                expect(eo > 0 and abs(eg - eo) <= 1e-9 * abs(eo) and _rel(Hg, Ho) <= 1e-9 and _rel(bg, bo) <= 1e-9, "%s: %s at the %s misses 1e-9" % (tag, fn, name))
                with_voxel = np.unique(o.correspondences()[0])
                assert with_voxel.shape[0] > 100
                print("READERS %s %-16s source points %d  with a voxel %d  poisoned %d  poisoned with a voxel %d" % (
                    tag, name, src.shape[0], with_voxel.shape[0], poisoned.sum(), poisoned[with_voxel].sum()), flush=True)
                if nrm_on and want_poisoned:
                    assert poisoned[with_voxel].sum() >= 1, "no poisoned point finds a voxel: the six-entry branch is not reached"
            eo, eg = o.compute_error(T), g.compute_error(T)
            print("STAGE %s %-16s %-13s error %.6e  rel %.2e" % (tag, name, "compute_error", eo, abs(eg - eo) / abs(eo)), flush=True)
            expect(abs(eg - eo) <= 1e-9 * abs(eo), "%s: compute_error at the %s misses 1e-9" % (tag, name))
        g.close()

        for fused in (0, 1, 2):
            o, g, _ = both(fused)
            rc, Tf_o, Td_o, it_o, cv_o = o.align(guess)
            assert rc == 0
            Tf_g = g.align(guess)
            Td_g = g.final_transformation_d
            st = g.last_stats
            print("ALIGN %s fused=%d  iterations %d / %d  converged %d / %d  angle %.2e  |dT_d| %.2e" % (
                tag, fused, st.n_outer, it_o, st.converged, cv_o, rot_angle(Td_g[:3, :3], Td_o[:3, :3]), np.abs(Td_g - Td_o).max()), flush=True)
            expect(rot_angle(Td_g[:3, :3], Td_o[:3, :3]) <= 1e-5 and np.abs(Td_g - Td_o).max() < 1e-8 and np.abs(Tf_g - Tf_o).max() < 1e-6, "%s: align, fused %d: the pose" % (tag, fused))
            expect(st.n_outer == it_o and bool(st.converged) == cv_o and st.lm_failed == 0, "%s: align, fused %d: iterations or flags" % (tag, fused))
            a = [r for r in o.trace() if r["stage"] == 0]; b = [r for r in g.trace() if r["stage"] == 0]
            assert a and b
            for ro, rg in zip(a, b):     # the decisions, as check_solve compares them: while the step is significant
                if abs(ro["y0"] - ro["yi"]) <= 1e-7 * abs(ro["y0"]):
                    break
                expect((ro["outer"], ro["trial"], ro["accepted"]) == (rg["outer"], rg["trial"], rg["accepted"]), "%s: align, fused %d: a decision of the trace: %s / %s" % (tag, fused, ro, rg))
                expect(abs(ro["y0"] - rg["y0"]) <= 1e-9 * abs(ro["y0"]) and abs(ro["yi"] - rg["yi"]) <= 1e-9 * abs(ro["yi"]), "%s: align, fused %d: a cost of the trace: %s / %s" % (tag, fused, ro, rg))
                expect(abs(ro["lam"] - rg["lam"]) <= 1e-6 * abs(ro["lam"]), "%s: align, fused %d: a damping of the trace" % (tag, fused))
            g.close()

    readers(s, t, "source-on-target", False)
    readers(t, s, "target-on-source", True)
    assert not errs, "\n".join(errs[:10])
    print("PLANE_FORM_OK")


@pytest.mark.parametrize("pass_nrm", [None, 0])
def test_plane_form_and_its_readers(pass_nrm):
    assert "PLANE_FORM_OK" in _child("_plane_main", {} if pass_nrm is None else dict(ROLO_PASS_NRM=str(pass_nrm)))
