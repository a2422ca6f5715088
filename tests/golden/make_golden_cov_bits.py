"""Records tests/golden/cov_bits.npz: the bits of the neighbourhood covariances (the six unique entries per point, source and target) and of the float64 pose of one
2-iteration registration, as the library of the commit this is run at computes them on the GPU — the yardstick of tests/test_gpu_cov_bits.py for changes to the moments
epilogue of the neighbour search and to the tail's SVD that must not move a bit. The clouds are rebuilt by the test from the same code (cov_bits_clouds below): 2 048 points
cut from synth.dense_pair("vlp16") (1 024 of the source, 1 024 of the target) and the lattice, duplicates and line clouds of tests/test_gpu_registration.py's
_degenerate_cloud (exact ties, zero distances, rank-1 neighbourhoods: two singular values zero, the sign fixes of the SVD decided by its last bits).

Both forms of the walk's epilogue (ROLO_KNN_MOMENTS = 1 / 0) are run, each in its own process (the switch is read once per process); they must agree bit for bit before
anything is written. Run from the repository root at the PARENT of a change, on the GPU:   python tests/golden/make_golden_cov_bits.py
(A change that moves bits on purpose records with its own library, after the arrays it does not mean to move compared equal to the earlier recording.)"""
import os
import subprocess
import sys
import zlib

import numpy as np

sys.path.insert(0, os.getcwd())

OUT = os.path.join("tests", "golden", "cov_bits.npz")
SIX = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
N_DEGENERATE = 200


def _xyz1(p):
    return np.ascontiguousarray(np.concatenate([p.astype(np.float32), np.ones((p.shape[0], 1), np.float32)], 1))


def _degenerate(kind, n, rng):
    """the lattice / duplicates / line clouds of tests/test_gpu_registration.py::_degenerate_cloud"""
    if kind == "lattice":
        m = int(np.ceil(n ** (1 / 3))) + 1
        g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
        pts = g[rng.permutation(g.shape[0])[:n]] * np.float32(0.25)
    elif kind == "duplicates":
        base = rng.uniform(-20, 20, (n // 3 + 1, 3)).astype(np.float32)
        pts = np.concatenate([base, base, base])[rng.permutation(3 * base.shape[0])[:n]]
    else:  # "line"
        t = np.sort(rng.uniform(-30, 30, n)).astype(np.float32)
        pts = np.stack([t, np.float32(0.5) * t + np.float32(1.0), np.float32(-0.25) * t], 1)
    return _xyz1(pts)


def cov_bits_clouds():
    """[(name, source, target, voxel resolution)]"""
    from rolo_amd import synth
    src, tgt, _ = synth.dense_pair("vlp16")
    out = [("vlp16", _xyz1(src[:: src.shape[0] // 1024][:1024, :3]), _xyz1(tgt[:: tgt.shape[0] // 1024][:1024, :3]), 1.0)]
    for kind in ("line", "duplicates", "lattice"):
        rng = np.random.default_rng(zlib.crc32(f"cov-bits-{kind}".encode()))
        out.append((kind, _degenerate(kind, N_DEGENERATE, rng), _degenerate(kind, N_DEGENERATE + 17, rng), 1.0))
    return out


def six(c):
    return np.ascontiguousarray(np.stack([c[:, a, b] for a, b in SIX], 1))


def compute():
    """{name_src, name_tgt: (n, 6) float64; name_pose: (4, 4) float64 (NaN where the registration finds no correspondences)} with the library this process loads"""
    from rolo_amd.rotvgicp import RotVGICP
    d = {}
    for name, src, tgt, res in cov_bits_clouds():
        g = RotVGICP(); g.setResolution(res); g.setInputTarget(tgt); g.setInputSource(src)
        g.computeCovariances()
        d[name + "_src"] = six(g.getSourceCovariances()); d[name + "_tgt"] = six(g.getTargetCovariances())
        g.close()
        g = RotVGICP(); g.setResolution(res); g.setFixedIterations(2); g.setInputTarget(tgt); g.setInputSource(src)
        try:
            g.align()
            d[name + "_pose"] = np.array(g.final_transformation_d, np.float64)
        except Exception as ex:   # no correspondences (ROLO_ENOCORR): the reference's behaviour too
            print("align:", name, ex, flush=True)
            d[name + "_pose"] = np.full((4, 4), np.nan)
        g.close()
    return d


def main():
    if len(sys.argv) > 1:   # child: one form of the epilogue
        np.savez(sys.argv[1], **compute())
        return
    import tempfile
    forms = []
    with tempfile.TemporaryDirectory() as tmp:
        for m in (1, 0):
            path = os.path.join(tmp, f"m{m}.npz")
            subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, ROLO_KNN_MOMENTS=str(m)), check=True, timeout=300)
            forms.append(dict(np.load(path)))
    for k in forms[0]:
        same = forms[0][k].tobytes() == forms[1][k].tobytes()
        print(k, forms[0][k].shape, "finite" if np.isfinite(forms[0][k]).all() else "NOT finite", "both forms the same bits" if same else "FORMS DIFFER")
        assert same, k
    np.savez_compressed(OUT, **forms[0])
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
