"""Scan Context on the key map: descriptor and detection times ("Scan Context").

Records into --out (profiles/r08/scancontext.json):
  descriptor   one 30 000-point cloud: from host points (upload, downSizeFilterSC at 0.5, descriptor) and from a key frame's resident surface cloud
  reference    detection in the reference's form (3 candidates from the ring keys, search_ratio 0.1) over 1 000, 10 000 and 100 000 stored descriptors
  exhaustive   detection in the original paper's form (every searched descriptor a candidate, all 60 shifts) over 1 000 and 10 000
Each figure: device time between two HIP events on the key map's stream (rolo_keymap_sc_last_ms), median of --reps calls after --warmup, with min / p10 / p90 /
max; beside it the host clock around the same calls (they end in a stream synchronise). No bar is set on these numbers: the parent has no such path and the
reference cannot be built. `twin_cpu_ms` is the numpy statement of the tests (tests/sc_twin.py: serial Python loops, a statement of arithmetic and NOT a
baseline), timed once where it finishes in seconds."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sc_twin as T  # noqa: E402
from rolo_amd.backend import KeyFrameMap  # noqa: E402

f32 = np.float32


def stats(ms):
    a = np.array(ms, np.float64)
    return dict(median_ms=float(np.median(a)), min_ms=float(a.min()), p10_ms=float(np.percentile(a, 10)), p90_ms=float(np.percentile(a, 90)), max_ms=float(a.max()), n=len(ms))


def timed(km, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    dev, host = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); host.append((time.perf_counter() - t0) * 1e3); dev.append(km.scLastMs())
    return dict(device=stats(dev), host_clock=stats(host))


def scan(n, seed):
    """a scan-like cloud: ground and scattered structure within 60 m"""
    rng = np.random.default_rng(seed)
    r = 60.0 * np.sqrt(rng.random(n)); a = rng.uniform(0, 2 * np.pi, n)
    z = np.where(rng.random(n) < 0.6, -1.8 + 0.05 * rng.standard_normal(n), rng.uniform(-1.8, 8.0, n))
    return np.stack([r * np.cos(a), r * np.sin(a), z, np.zeros(n)], 1).astype(f32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30); ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="1000,10000,100000"); ap.add_argument("--exhaustive-sizes", default="1000,10000")
    ap.add_argument("--out", default=os.path.join("profiles", "r08", "scancontext.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sc_time.py needs a GPU: a timing taken without one says nothing")
    res = dict(workload=dict(points=30000, leaf=0.5, small_cloud_points=48, reps=a.reps, warmup=a.warmup))
    # ---- descriptor ----
    km = KeyFrameMap()
    big = scan(30000, 1)
    k = km.addKeyFrame(np.zeros((0, 4), f32), big, np.zeros(6, f32), 0.0)
    calls = 3 * (a.reps + a.warmup) + 1
    while True:   # grow the store first, so that no timed call re-allocates it: it grows by half, so after n adds it holds at least n; stop with room for every timed call
        n = km.scSize()
        cap = 0
        while cap <= n:
            cap = cap + cap // 2 + 64
        if cap - n > calls:
            break
        km.scAddCloud(big[:64], 0.0)
    km.scAddCloud(big[:64], 0.0)   # the add that re-allocates, when the loop stopped exactly at a full store
    res["descriptor_from_host_points_leaf_0.5"] = timed(km, lambda: km.scAddCloud(big, 0.5), a.reps, a.warmup)
    res["descriptor_from_host_points_no_filter"] = timed(km, lambda: km.scAddCloud(big, 0.0), a.reps, a.warmup)
    res["descriptor_from_resident_surface"] = timed(km, lambda: km.scAddSurface(k), a.reps, a.warmup)
    t0 = time.perf_counter(); want = T.make_scancontext(big); tk = T.keys(want); res["descriptor_twin_cpu_ms"] = (time.perf_counter() - t0) * 1e3
    got = km.scDescriptor(km.scSize() - 1)
    same = bool(all(np.array_equal(g, w) for g, w in zip(got, (want,) + tk)))
    km.close()
    # ---- detection ----
    sizes = [int(s) for s in a.sizes.split(",")]; ex_sizes = [int(s) for s in a.exhaustive_sizes.split(",")]
    nmax = max(sizes + ex_sizes)
    km = KeyFrameMap()
    p = km.scParams()
    km.scSetParams(p)
    pool = scan(48 * 4096, 2)
    rng = np.random.default_rng(3)
    t0 = time.perf_counter()
    for i in range(nmax + 1):
        j = int(rng.integers(0, 4096 - 1))
        km.scAddCloud(pool[48 * j: 48 * j + 48 + (i % 7)], 0.0)
    res["fill_store_host_clock_s"] = dict(descriptors=nmax + 1, seconds=time.perf_counter() - t0)
    query = nmax
    res["reference_form_K3_ratio0.1"] = {}
    res["exhaustive_form_Kall_ratio1.0"] = {}
    for n in sizes:
        p.num_candidates = 3; p.search_ratio = 0.1; km.scSetParams(p)
        res["reference_form_K3_ratio0.1"][str(n)] = timed(km, lambda: km.scDetect(query, n), a.reps, a.warmup)
    for n in ex_sizes:
        p.num_candidates = 0; p.search_ratio = 1.0; km.scSetParams(p)
        res["exhaustive_form_Kall_ratio1.0"][str(n)] = timed(km, lambda: km.scDetect(query, n), max(5, a.reps // 3), 2)
    # the twin on the smallest size: the same answer, and its CPU time (labelled: not a baseline)
    n0 = min(sizes + ex_sizes)
    st = T.Store()
    rng = np.random.default_rng(3)
    picks = []
    for i in range(nmax + 1):
        j = int(rng.integers(0, 4096 - 1))
        picks.append((j, i))
    for j, i in picks[:n0] + [picks[query]]:
        st.add(pool[48 * j: 48 * j + 48 + (i % 7)])
    twin = {}
    for name, K, ratio in (("reference_form_K3_ratio0.1", 3, 0.1), ("exhaustive_form_Kall_ratio1.0", 0, 1.0)):
        st.P.update(num_candidates=K, search_ratio=ratio)
        p.num_candidates = K; p.search_ratio = ratio; km.scSetParams(p)
        t0 = time.perf_counter(); w = st.detect(n0, n0); ms = (time.perf_counter() - t0) * 1e3
        g = km.scDetect(query, n0)
        twin[name] = dict(descriptors=n0, twin_cpu_ms=ms)
        same = same and (g.nn_idx, g.nn_align, g.min_dist, g.loop_id) == (w["nn_idx"], w["nn_align"], float(w["min_dist"]), w["loop_id"])
    res["twin_cpu_statement_not_a_baseline"] = twin
    res["gpu_equals_twin_bitwise"] = same
    km.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    assert same, "the device's answer differs from the twin's"


if __name__ == "__main__":
    main()
