"""CPU: the constructed covariance cases (tests/cov_cases.py) — the committed fixture is what the module builds, every premise of the construction holds, and the oracle
meets every assertion of the exact statement. The oracle's deviation from exact arithmetic over the well-defined clusters is the recorded bar of the GPU test
(tests/test_gpu_cov_cases.py): 10 x that, floored at 8 * 2^-53, relative to the largest |entry|."""
import numpy as np
import pytest

import cov_cases as cc
from oracle import pyorc


@pytest.fixture(scope="module")
def rebuilt():
    return cc.build_fixture()


@pytest.fixture(scope="module")
def loaded():
    return cc.load()


def test_the_fixture_is_fresh(rebuilt):
    """every array of the committed file has the bytes that the module builds now (the zip container carries time stamps: the arrays are compared, one by one)"""
    z = np.load(cc.GOLDEN)
    assert sorted(z.files) == sorted(rebuilt)
    for k in z.files:
        a, b = z[k], np.asarray(rebuilt[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    import os
    assert os.path.getsize(cc.GOLDEN) < os.path.getsize(os.path.join(os.path.dirname(cc.GOLDEN), "cov_bits.npz"))


def test_each_premise_holds(loaded):
    cases, _ = loaded
    seen = set()
    for (cloud, k, side), c in cases.items():
        n = c.pts.shape[0]
        assert n % 256 != 0 and n == k * len(c.cls)
        assert cc.separation_ok(c.pts, c.owner), c.key
        idx, _ = pyorc.knn(c.xyz1, k)
        assert cc.knn_inside_clusters(c, idx), c.key           # the k-NN of every point is its own cluster
        for j in range(len(c.cls)):                            # the classes, from the exact matrix alone
            s1, s2, C = cc.exact_moments(c.pts[c.owner == j])
            assert cc.exact_class(C) == c.cls[j], (c.key, j)
            if cloud == "regular":                             # no zero among the nine sums: every wavefront takes the shared-reciprocal path
                assert c.cls[j] == cc.W and cc.sums_regular(dict(s1=s1, s2=s2)), (c.key, j)
        seen |= {(k, int(v)) for v in c.cls}
    for k in cc.KS:
        assert ((cases[("regular", k, "src")].pts.shape[0] + 255) // 256) != ((cases[("regular", k, "tgt")].pts.shape[0] + 255) // 256)
        assert ((cases[("mixed", k, "src")].pts.shape[0] + 255) // 256) != ((cases[("mixed", k, "tgt")].pts.shape[0] + 255) // 256)
        want = set(range(7)) if k in (20, 7) else set(range(7)) - {cc.T2, cc.T3}
        assert {v for kk, v in seen if kk == k} == want, (k, seen)


def _oracle_dev(cases):
    dev = np.zeros(6)
    out = {}
    for cloud in cc.CLOUDS:
        for k in cc.KS:
            s, t = cases[(cloud, k, "src")], cases[(cloud, k, "tgt")]
            for rule in range(6):
                cs, ct = cc.oracle_covariances(rule, k, s.pts, t.pts)
                out[(cloud, k, rule)] = (cs, ct)
                for c, cov in ((s, cs), (t, ct)):
                    sel = (c.pcls == cc.W) | (c.pcls == cc.T2)
                    E = c.exp[c.block[c.owner], rule]
                    dev[rule] = max(dev[rule], (np.abs(cov[sel] - E[sel]).max((1, 2)) / np.abs(E[sel]).max((1, 2))).max())
    return dev, out


@pytest.fixture(scope="module")
def oracle_runs(loaded):
    return _oracle_dev(loaded[0])


def test_the_bars_are_recorded(loaded, oracle_runs):
    """per regularisation: the oracle's largest deviation from the exact matrix over the W and T2 clusters of all k, relative to the largest |entry|"""
    dev = oracle_runs[0]
    for r, a, b in zip(cc.RULES, dev, cc.bars(loaded[1])):
        print("BAR %-20s oracle deviation %.3e  -> bar of the GPU test %.3e" % (r, a, b))
    assert np.array_equal(dev, loaded[1]), (dev, loaded[1])
    assert (dev < 1e-11).all()   # (the oracle is that close to exact arithmetic; the older tests compare with it at 1e-9 absolute)


@pytest.mark.parametrize("rule", range(6), ids=cc.RULES)
def test_the_oracle_meets_every_assertion(loaded, oracle_runs, rule):
    cases, dev = loaded
    bar = cc.bars(dev)[rule]
    worst, signs = 0.0, {1: 0, -1: 0}
    for cloud in cc.CLOUDS:
        for k in cc.KS:
            for side, cov in zip(("src", "tgt"), oracle_runs[1][(cloud, k, rule)]):
                w, s = cc.check_covariances(cases[(cloud, k, side)], rule, cov, bar, ref=cov)
                worst = max(worst, w); signs[1] += s[1]; signs[-1] += s[-1]
    print("ORACLE %-20s worst ratio to the bar %.3f, R2 signs +1: %d, -1: %d" % (cc.RULES[rule], worst, signs[1], signs[-1]))
