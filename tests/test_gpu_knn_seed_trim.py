"""GPU: the trimmed seed phase of the k = 20 neighbour search — merge_chunk without a sort of the tail, and the first seed leaf written straight into the list of sentinels
(knn_seed_net.hpp first_two_chunks, knn_packet.hpp knn_seed_leaf<true>) — at the cloud sizes where the first seed is a special leaf, in every forced walk form
(ROLO_KNN_SUB = 0: 64-query packets, 2 / 4: lanes per query) and with the walk leaving moments or index lists (ROLO_KNN_MOMENTS = 1 / 0). Neighbour indices and float
distances equal the oracle's bit for bit; the covariances of the pair launch (which leaves no lists to read) agree with the oracle's to 1e-9, the bound of
tests/test_gpu_knn_seeds.py.

The sizes (leaves of 16 points, packets of 64): 20 and 21 — one full and one partial leaf, whose padding points carry the sentinel key through the first leaf's network;
33, 48, 49 — the only packet's first seed is followed by a partial or by no further leaf; 64 and 65 — exactly one packet, and a second one whose first own leaf is the
cloud's last, partial one, with a seed before it and none after; 79, 80, 81, 96, 97 — the second packet's own leaves end the cloud (partial, full, one point into the next),
no leaf after them; 129 and 257 — a third and a fifth packet of one point; 1 000 — packets with seeds on both sides. One more cloud of 257 points holds 40 copies of one
point: whole chunks tie in d2 and the index decides. The oracle's lists are computed once per session and handed to the child processes in a file (the switches are read
once per process)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 20
SIZES = (20, 21, 33, 48, 49, 64, 65, 79, 80, 81, 96, 97, 129, 257, 1000)


def _clouds():
    rng = np.random.default_rng(20261020)
    def xyz1(p):
        return np.ascontiguousarray(np.concatenate([p.astype(np.float32), np.ones((p.shape[0], 1), np.float32)], 1))
    out = [(f"random{n}", xyz1(rng.uniform(-8, 8, (n, 3)))) for n in SIZES]
    p = rng.uniform(-8, 8, (257, 3)).astype(np.float32)
    p[rng.choice(257, 40, replace=False)] = p[0]
    out.append(("copies257", xyz1(p)))
    return out


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """every cloud with the oracle's lists and covariances: cloud i is searched as the source of the pair (cloud i, cloud i + 1), and as the target of the pair before"""
    from oracle import pyorc
    clouds = _clouds()
    d = {"names": np.array([n for n, _ in clouds])}
    for i, (name, c) in enumerate(clouds):
        idx, d2 = pyorc.knn(c, K)
        o = pyorc.Reg(pyorc.default_params(voxel_type=1, voxel_resolution=0.5)); o.set_target(clouds[(i + 1) % len(clouds)][1]); o.set_source(c)
        assert o.compute_covariances() == 0
        d[f"xyz{i}"] = c; d[f"idx{i}"] = idx; d[f"d2{i}"] = d2; d[f"cov{i}"] = o.source_covs()
    path = str(tmp_path_factory.mktemp("knn_seed_trim") / "reference.npz")
    np.savez(path, **d)
    return path


def _trim_main(path):
    """body of test_trimmed_seed_lists_match_the_oracle (own process: ROLO_KNN_SUB and ROLO_KNN_MOMENTS are read once per process)"""
    from rolo_amd.rotvgicp import RotVGICP
    d = np.load(path)
    names = [str(n) for n in d["names"]]
    out = []
    for i, name in enumerate(names):
        j = (i + 1) % len(names)
        src, tgt = d[f"xyz{i}"], d[f"xyz{j}"]
        g = RotVGICP(); g.setResolution(0.5)
        g.setInputTarget(tgt); g.setInputSource(src)
        idx_g, d2_g = g.knn(0)
        idx_t, d2_t = g.knn(1)   # the neighbour cloud as the second cloud of the launch
        g.computeCovariances()   # the pair launch (both clouds in one grid), the walk's epilogue as ROLO_KNN_MOMENTS says
        ecov = float(np.abs(g.getSourceCovariances() - d[f"cov{i}"]).max())
        ecov_t = float(np.abs(g.getTargetCovariances() - d[f"cov{j}"]).max())
        res = dict(name=name, n=int(src.shape[0]), idx=bool(np.array_equal(idx_g, d[f"idx{i}"])), d2=bool(np.array_equal(d2_g, d[f"d2{i}"])),
                   idx_t=bool(np.array_equal(idx_t, d[f"idx{j}"])), d2_t=bool(np.array_equal(d2_t, d[f"d2{j}"])),
                   cov_err=ecov, cov_err_t=ecov_t)
        print("TRIM", res, flush=True)
        out.append(res)
        g.close()
    bad = [r for r in out if not (r["idx"] and r["d2"] and r["idx_t"] and r["d2_t"] and r["cov_err"] <= 1e-9 and r["cov_err_t"] <= 1e-9)]
    assert not bad, bad
    print("TRIM_OK", len(out))


@pytest.mark.parametrize("moments", [1, 0])
@pytest.mark.parametrize("sub", [0, 2, 4])
def test_trimmed_seed_lists_match_the_oracle(reference, sub, moments):
    env = dict(os.environ, ROLO_KNN_SUB=str(sub), ROLO_KNN_MOMENTS=str(moments))
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); from tests.test_gpu_knn_seed_trim import _trim_main; _trim_main(%r)" % (ROOT, reference)],
                       env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "TRIM_OK %d" % (len(SIZES) + 1) in r.stdout
