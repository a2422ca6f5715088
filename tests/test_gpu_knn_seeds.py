"""GPU: the seed lists of the k = 20 neighbour search, built by sorting / merging networks (knn_seed_net.hpp, knn_packet.hpp seed_chunk) instead of one sorted insert per
candidate, at the smallest clouds where that path can go wrong — in every forced walk form (ROLO_KNN_SUB = 0: 64-query packets, 2 / 4: lanes per query) and with the walk
leaving moments or index lists (ROLO_KNN_MOMENTS = 1 / 0). Neighbour indices and float distances equal the oracle's bit for bit, covariances agree to 1e-9.

The clouds: 21, 64, 80, 96, 100, 257 and 1 031 random points (a single partial packet, padded lanes, a padded last leaf; 96 points are exactly the six seed leaves of the only
packet, so the tree walk adds nothing; first and last packets have their seed range clipped at the ends of the curve); 1 031 points of which 40 are copies of one point (whole
chunks of 8 tie in d2 and the index decides); a 6 x 6 x 6 lattice plus 41 points (exact distance ties across chunks). The oracle's lists and covariances are computed once per
session and handed to the child processes in a file (the switches are read once per process)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 20


def _clouds():
    rng = np.random.default_rng(20260918)
    def xyz1(p):
        return np.ascontiguousarray(np.concatenate([p.astype(np.float32), np.ones((p.shape[0], 1), np.float32)], 1))
    out = [(f"random{n}", xyz1(rng.uniform(-8, 8, (n, 3)))) for n in (21, 64, 80, 96, 100, 257, 1031)]
    p = rng.uniform(-8, 8, (1031, 3)).astype(np.float32)
    p[rng.choice(1031, 40, replace=False)] = p[0]
    out.append(("copies1031", xyz1(p)))
    lat = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * np.float32(0.5)
    p = np.concatenate([lat, rng.uniform(0, 2.5, (41, 3)).astype(np.float32)])
    out.append(("lattice257", xyz1(p[rng.permutation(p.shape[0])])))
    return out


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """every cloud with the oracle's lists and covariances: cloud i is searched as the source of the pair (cloud i, cloud i + 1)"""
    from oracle import pyorc
    clouds = _clouds()
    d = {"names": np.array([n for n, _ in clouds])}
    for i, (name, c) in enumerate(clouds):
        idx, d2 = pyorc.knn(c, K)
        o = pyorc.Reg(pyorc.default_params(voxel_type=1, voxel_resolution=0.5)); o.set_target(clouds[(i + 1) % len(clouds)][1]); o.set_source(c)
        assert o.compute_covariances() == 0
        d[f"xyz{i}"] = c; d[f"idx{i}"] = idx; d[f"d2{i}"] = d2; d[f"cov{i}"] = o.source_covs()
    path = str(tmp_path_factory.mktemp("knn_seeds") / "reference.npz")
    np.savez(path, **d)
    return path


def _seeds_main(path):
    """body of test_seed_lists_match_the_oracle (own process: ROLO_KNN_SUB and ROLO_KNN_MOMENTS are read once per process)"""
    from rolo_amd.rotvgicp import RotVGICP
    d = np.load(path)
    names = [str(n) for n in d["names"]]
    out = []
    for i, name in enumerate(names):
        src, tgt = d[f"xyz{i}"], d[f"xyz{(i + 1) % len(names)}"]
        g = RotVGICP(); g.setResolution(0.5)
        g.setInputTarget(tgt); g.setInputSource(src)
        idx_g, d2_g = g.knn(0)
        idx_t, d2_t = g.knn(1)   # the neighbour cloud as the second cloud of the launch
        j = (i + 1) % len(names)
        g.computeCovariances()   # the pair launch (both clouds in one grid), the walk's epilogue as ROLO_KNN_MOMENTS says
        ecov = float(np.abs(g.getSourceCovariances() - d[f"cov{i}"]).max())
        ecov_t = float(np.abs(g.getTargetCovariances() - d[f"cov{j}"]).max())
        res = dict(name=name, n=int(src.shape[0]), idx=bool(np.array_equal(idx_g, d[f"idx{i}"])), d2=bool(np.array_equal(d2_g, d[f"d2{i}"])),
                   idx_t=bool(np.array_equal(idx_t, d[f"idx{j}"])), d2_t=bool(np.array_equal(d2_t, d[f"d2{j}"])), cov_err=ecov, cov_err_t=ecov_t)
        print("SEEDS", res, flush=True)
        out.append(res)
        g.close()
    bad = [r for r in out if not (r["idx"] and r["d2"] and r["idx_t"] and r["d2_t"] and r["cov_err"] <= 1e-9 and r["cov_err_t"] <= 1e-9)]
    assert not bad, bad
    print("SEEDS_OK", len(out))


@pytest.mark.parametrize("moments", [1, 0])
@pytest.mark.parametrize("sub", [0, 2, 4])
def test_seed_lists_match_the_oracle(reference, sub, moments):
    env = dict(os.environ, ROLO_KNN_SUB=str(sub), ROLO_KNN_MOMENTS=str(moments))
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); from tests.test_gpu_knn_seeds import _seeds_main; _seeds_main(%r)" % (ROOT, reference)],
                       env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "SEEDS_OK 9" in r.stdout
