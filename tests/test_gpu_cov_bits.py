"""GPU: the neighbourhood covariances (the six unique entries per point, source and target) and the float64 pose of one 2-iteration registration have the BITS recorded in
tests/golden/cov_bits.npz — by tests/golden/make_golden_cov_bits.py on the GPU, at the parent of the commit that shares the reciprocal among the moments epilogue's
divisions and replaces the divisions of the tail's SVD by sign copies and shared reciprocals. The fixture is the yardstick for any later change to walk_write_moments or
to make_jacobi / jacobi_pair / jacobi_svd3 that claims to keep every bit: it compares with what the earlier code computed, never with the code under test.

The clouds (rebuilt here by the generator's own cov_bits_clouds): 2 048 points cut from synth.dense_pair("vlp16"), and a line, a duplicates and a lattice cloud of 200 / 217
points — rank-1 neighbourhoods whose SVD sign fixes hang on the last bits, zero distances, exact ties and exactly zero moments (which take the plain-division path).
Re-recorded once, with the library of the commit that made the six entries of a plane-form point I - m m^T where they were not (knn_covariance_finish; tests/test_gpu_cov_cases.py):
8 + 21 points of the line cloud, whose y is rounded (two singular values tiny, not zero), and with them its pose (by 1.1e-8), changed on purpose; the other nine arrays were
compared with the earlier recording first and kept every bit.
Both forms of the walk's epilogue (ROLO_KNN_MOMENTS = 1 / 0), and the 64-query packets (ROLO_KNN_SUB = 0) beside the walk picked by size, each in its own process
(the switches are read once per process)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cov_bits.npz")


def _bits_main():
    """body of test_covariances_and_pose_keep_the_recorded_bits (own process)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_cov_bits as gen
    want = np.load(GOLDEN)
    got = gen.compute()
    assert sorted(got) == sorted(want.files), (sorted(got), sorted(want.files))
    bad = []
    for k in want.files:
        a, b = want[k], got[k]
        same = a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b, equal_nan=k.endswith("_pose")))   # (a pose is NaN where the parent found no correspondences either)
        ndiff = int((a != b).sum()) if a.shape == b.shape else -1
        print("BITS", k, a.shape, "equal" if same else "DIFFERENT: %d entries, max |diff| %.3e" % (ndiff, float(np.nanmax(np.abs(a - b))) if a.shape == b.shape else np.nan), flush=True)
        if not same:
            bad.append(k)
    assert not bad, bad
    print("BITS_OK", len(want.files))


@pytest.mark.parametrize("sub", [None, 0])
@pytest.mark.parametrize("moments", [1, 0])
def test_covariances_and_pose_keep_the_recorded_bits(moments, sub):
    env = dict(os.environ, ROLO_KNN_MOMENTS=str(moments))
    env.pop("ROLO_KNN_SUB", None)
    if sub is not None:
        env["ROLO_KNN_SUB"] = str(sub)
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); from tests.test_gpu_cov_bits import _bits_main; _bits_main()" % ROOT],
                       env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "BITS_OK 12" in r.stdout
