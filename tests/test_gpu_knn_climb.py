"""GPU: the k = 20 neighbour search whose packet walk CLIMBS from the packet's own subtree (knn_packet.hpp packet_climb), tests both child boxes of a node as one pair
with one clamped compare per child (knn_box_pair.hpp) and reads its bound from the list's last slot — at the smallest clouds where the climb or the clamp can go wrong,
in every forced walk form (ROLO_KNN_SUB = 0: 64-query packets, 2 / 4: lanes per query) and with the walk leaving moments or index lists (ROLO_KNN_MOMENTS = 1 / 0).
Neighbour indices and float distances equal the oracle's (pyorc.knn) bit for bit, covariances agree to 1e-9. Every cloud is searched as the source and as the target
of a pair launch: cloud i is the source of the pair (cloud i, cloud i + 1).

The clouds:
  * 20, 21, 63 and 64 random points: P < 4 or a = 1 — no climb, the bound infinite after the seeds (20 points: it ends exactly full). One point: the library refuses a
    cloud of fewer than k points (ROLO_ETOOFEW) as the oracle does (orc_knn returns -2), so no list exists to compare — test_one_point_is_refused_as_by_the_oracle;
  * 65, 96, 97, 128 and 129 points: a second (third) packet that is mostly padding, P = 8 / 16 with all-padding sibling subtrees;
  * 257, 1 031 and 4 097 points: P = 32 ... 512, the last packet clipped;
  * two clusters of 300 points 50 m apart and 5 points between them: whole siblings out of reach of all but a few lanes, a high sibling reached after low ones were not;
  * a 6 x 6 x 6 lattice plus 41 points: box distances exactly equal to the bound, "<=" must explore;
  * 1 031 points with 40 copies of one point;
  * 64 next to 4 097 points in one launch: `split`, and a different P per cloud;
  * the 4 097-point cloud sharded by query point (rolo_set_shard_knn) into three slices: the union of the slices' lists is bit-identical to the unsharded lists.
The oracle's lists and covariances are computed once per session and handed to the child processes in a file (the switches are read once per process)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 20
WORLD = 3


def _xyz1(p):
    return np.ascontiguousarray(np.concatenate([p.astype(np.float32), np.ones((p.shape[0], 1), np.float32)], 1))


def _clouds():
    rng = np.random.default_rng(20261019)
    out = [(f"random{n}", _xyz1(rng.uniform(-8, 8, (n, 3)))) for n in (20, 21, 63, 64, 4097, 65, 96, 97, 128, 129, 257, 1031)]   # (64 next to 4 097: the unequal pair)
    a = rng.normal(0, 1.5, (300, 3)); b = rng.normal(0, 1.5, (300, 3)) + np.array([50.0, 0, 0])
    mid = np.stack([np.linspace(10, 40, 5), rng.uniform(-1, 1, 5), rng.uniform(-1, 1, 5)], 1)
    p = np.concatenate([a, b, mid]).astype(np.float32)
    out.append(("clusters605", _xyz1(p[rng.permutation(p.shape[0])])))
    lat = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * np.float32(0.5)
    p = np.concatenate([lat, rng.uniform(0, 2.5, (41, 3)).astype(np.float32)])
    out.append(("lattice257", _xyz1(p[rng.permutation(p.shape[0])])))
    p = rng.uniform(-8, 8, (1031, 3)).astype(np.float32)
    p[rng.choice(1031, 40, replace=False)] = p[0]
    out.append(("copies1031", _xyz1(p)))
    return out


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    from oracle import pyorc
    clouds = _clouds()
    d = {"names": np.array([n for n, _ in clouds])}
    for i, (name, c) in enumerate(clouds):
        idx, d2 = pyorc.knn(c, K)
        o = pyorc.Reg(pyorc.default_params(voxel_type=1, voxel_resolution=0.5)); o.set_target(clouds[(i + 1) % len(clouds)][1]); o.set_source(c)
        assert o.compute_covariances() == 0
        d[f"xyz{i}"] = c; d[f"idx{i}"] = idx; d[f"d2{i}"] = d2; d[f"cov{i}"] = o.source_covs()
    path = str(tmp_path_factory.mktemp("knn_climb") / "reference.npz")
    np.savez(path, **d)
    return path


def _climb_main(path):
    """body of test_climbed_lists_match_the_oracle (own process: ROLO_KNN_SUB and ROLO_KNN_MOMENTS are read once per process)"""
    from rolo_amd.rotvgicp import RotVGICP
    from rolo_amd._lib import lib, check
    d = np.load(path)
    names = [str(n) for n in d["names"]]
    out = []
    for i, name in enumerate(names):
        j = (i + 1) % len(names)
        src, tgt = d[f"xyz{i}"], d[f"xyz{j}"]
        g = RotVGICP(); g.setResolution(0.5)
        g.setInputTarget(tgt); g.setInputSource(src)
        idx_g, d2_g = g.knn(0)
        idx_t, d2_t = g.knn(1)
        g.computeCovariances()   # the pair launch (both clouds in one grid), the walk's epilogue as ROLO_KNN_MOMENTS says
        ecov = float(np.abs(g.getSourceCovariances() - d[f"cov{i}"]).max())
        ecov_t = float(np.abs(g.getTargetCovariances() - d[f"cov{j}"]).max())
        res = dict(name=name, n=int(src.shape[0]), idx=bool(np.array_equal(idx_g, d[f"idx{i}"])), d2=bool(np.array_equal(d2_g, d[f"d2{i}"])),
                   idx_t=bool(np.array_equal(idx_t, d[f"idx{j}"])), d2_t=bool(np.array_equal(d2_t, d[f"d2{j}"])), cov_err=ecov, cov_err_t=ecov_t)
        print("CLIMB", res, flush=True)
        out.append(res)
        g.close()
    bad = [r for r in out if not (r["idx"] and r["d2"] and r["idx_t"] and r["d2_t"] and r["cov_err"] <= 1e-9 and r["cov_err_t"] <= 1e-9)]
    assert not bad, bad
    print("CLIMB_OK", len(out))

    # the 4 097-point cloud in three slices of whole 256-query workgroups (its 64-point neighbour beside it: one slice holds all of that one, two hold nothing)
    i = names.index("random4097"); small = names.index("random64")
    src, tgt = d[f"xyz{i}"], d[f"xyz{small}"]
    n = src.shape[0]
    seen = np.zeros(n, int)
    for r in range(WORLD):
        g = RotVGICP(); g.setResolution(0.5)
        g.setInputTarget(tgt); g.setInputSource(src)
        g.setSourceCovariances(np.full((n, 4, 4), np.nan)); g.setTargetCovariances(np.full((tgt.shape[0], 4, 4), np.nan))   # poison: the rank fills its slice only
        check(lib().rolo_set_shard_knn(g._h, 1), "rolo_set_shard_knn")
        check(lib().rolo_set_shard(g._h, r, WORLD), "rolo_set_shard")
        g.computeCovariances()
        cov = g.getSourceCovariances()
        own = ~np.isnan(cov[:, 0, 0])
        idx_g, d2_g = g.knn(0)   # the slice's lists (the other rows are not this rank's)
        res = dict(rank=r, own=int(own.sum()), idx=bool(np.array_equal(idx_g[own], d[f"idx{i}"][own])), d2=bool(np.array_equal(d2_g[own], d[f"d2{i}"][own])),
                   cov_err=float(np.abs(cov[own] - d[f"cov{i}"][own]).max()) if own.any() else 0.0)
        print("SHARD", res, flush=True)
        assert res["idx"] and res["d2"] and res["cov_err"] <= 1e-9, res
        seen += own
        g.close()
    assert (seen == 1).all(), (int((seen == 0).sum()), int((seen > 1).sum()))   # the slices tile the cloud exactly
    print("SHARDS_OK", WORLD)


@pytest.mark.parametrize("moments", [1, 0])
@pytest.mark.parametrize("sub", [0, 2, 4])
def test_climbed_lists_match_the_oracle(reference, sub, moments):
    env = dict(os.environ, ROLO_KNN_SUB=str(sub), ROLO_KNN_MOMENTS=str(moments))
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); from tests.test_gpu_knn_climb import _climb_main; _climb_main(%r)" % (ROOT, reference)],
                       env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "CLIMB_OK 15" in r.stdout and "SHARDS_OK 3" in r.stdout


def test_one_point_is_refused_as_by_the_oracle():
    """fewer points than k: the oracle has no list (orc_knn: -2) and the library says ROLO_ETOOFEW before any launch — there is no walk to climb"""
    from oracle import pyorc
    from rolo_amd.rotvgicp import RotVGICP
    from rolo_amd._lib import RoloError
    one = _xyz1(np.array([[1.0, 2.0, 3.0]]))
    idx = np.zeros((1, K), np.int32); d2 = np.zeros((1, K), np.float32)
    assert pyorc.lib().orc_knn(pyorc._f(one), 1, 4, K, 0, pyorc._i(idx), pyorc._f(d2)) == -2
    g = RotVGICP(); g.setResolution(0.5)
    g.setInputTarget(_clouds()[0][1]); g.setInputSource(one)
    with pytest.raises(RoloError) as e:
        g.knn(0)
    assert e.value.code == -2   # ROLO_ETOOFEW
    g.close()
