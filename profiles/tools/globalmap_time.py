"""The global map from resident key frames: the one-shot form against the streamed form, and the sizes past the one-shot limit (ISSUE "global map on the GPU
from resident key frames").

Workload: key frames of 1 500 corner and 30 000 surface points (submap_time.py's hall, 100 distinct sensor-frame clouds reused along the track), 2 m apart on a
circle of 700 m radius, leaf 1.0 (config/params.yaml:69). Records into --out (profiles/r16/globalmap.json):
  (a) one list just under 2^26 points: the one-shot form (batch 2^26) against the streamed form at batch 2^20 / 2^22 / 2^24. A list of at most `batch` points
      is one-shot by rule, so the streamed form at batch 2^26 is measured on (c)'s list
  (b) a publishGlobalMap-sized call: the first 1 000 key frames at the default batch, and one-shot
  (c) about 2 * 10^8 points (every key frame listed three times: the list may repeat, the store need not grow) at batch 2^24 and 2^26
  (d) for scale only: the CPU oracle's composition of (b) (get_transformation + transform_cloud_f + voxelgrid), OMP threads as the environment sets them; the GPU
      result of (b) is compared with it bit for bit on the way
Device time is what rolo_keymap_global_last_ms reports (between HIP events on the key map's stream: box pass + sort-and-merge pass + finish); each figure is the
median of --reps calls after --warmup, with min / p10 / p90 / max, and the host clock around the whole call beside it."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import pyorc  # noqa: E402
from rolo_amd.backend import KeyFrameMap  # noqa: E402
from submap_time import make_keyframes  # noqa: E402

f32 = np.float32


def track_pose(k, spacing=2.0, radius=700.0):
    a = spacing * k / radius
    return np.array([0.001 * np.sin(k), 0.001 * np.cos(k), a + np.pi / 2, radius * np.cos(a), radius * np.sin(a), 1.8], f32)


def stats(v):
    a = np.asarray(v, np.float64)
    return dict(median_ms=float(np.median(a)), min_ms=float(a.min()), p10_ms=float(np.percentile(a, 10)), p90_ms=float(np.percentile(a, 90)), max_ms=float(a.max()), n=len(a))


def measure(km, idx, leaf, batch, reps, warmup):
    km.setGlobalBatch(batch)
    parts, wall = [], []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        km.globalMap(idx, leaf, download=False)
        w = time.perf_counter() - t0
        if r >= warmup:
            parts.append(km.globalLastMs().astype(np.float64)); wall.append(w * 1e3)
    parts = np.array(parts)
    info = km.globalInfo()
    return dict(batch=int(batch), info=info, device=stats(parts.sum(axis=1)), box_pass=stats(parts[:, 0]), sort_merge_pass=stats(parts[:, 1]), finish=stats(parts[:, 2]),
                host_wall=stats(wall))


def oracle_compose(base, poses, idx, leaf):
    parts = []
    for k in idx:
        p = [float(v) for v in poses[k]]
        T = pyorc.get_transformation(p[3], p[4], p[5], p[0], p[1], p[2])
        for cloud in base[k % len(base)][:2]:
            moved = cloud.copy()
            moved[:, :3] = pyorc.transform_cloud_f(np.ascontiguousarray(cloud[:, :3]), T)
            parts.append(moved)
    return pyorc.voxelgrid(np.concatenate(parts), leaf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corner", type=int, default=1500); ap.add_argument("--surf", type=int, default=30000); ap.add_argument("--distinct", type=int, default=100)
    ap.add_argument("--publish-frames", type=int, default=1000); ap.add_argument("--leaf", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=10); ap.add_argument("--warmup", type=int, default=2); ap.add_argument("--oracle-reps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join("profiles", "r16", "globalmap.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("globalmap_time.py needs a GPU: a timing taken without one says nothing")
    per = a.corner + a.surf
    n_frames = (2 ** 26 - 1) // per                      # the longest list of whole key frames under 2^26 points
    base = make_keyframes(a.distinct, a.corner, a.surf)
    poses = [track_pose(k) for k in range(n_frames)]
    km = KeyFrameMap()
    for k in range(n_frames):
        km.addKeyFrame(base[k % a.distinct][0], base[k % a.distinct][1], poses[k], 0.5 * k)
    res = dict(workload=dict(key_frames=n_frames, corner_per_frame=a.corner, surf_per_frame=a.surf, distinct_clouds=a.distinct, leaf=a.leaf,
                             resident_points=n_frames * per, omp_threads=os.environ.get("OMP_NUM_THREADS", "unset")))
    all_idx = np.arange(n_frames, dtype=np.int32)
    # (a)
    ta = dict(list_points=n_frames * per)
    ta["one_shot"] = measure(km, all_idx, a.leaf, 2 ** 26, a.reps, a.warmup)
    one_shot = km.globalMapPoints()
    for e in (20, 22, 24):
        ta[f"streamed_2^{e}"] = measure(km, all_idx, a.leaf, 2 ** e, a.reps, a.warmup)
        assert km.globalMapPoints().tobytes() == one_shot.tobytes(), e
        ta[f"streamed_2^{e}"]["over_one_shot"] = ta[f"streamed_2^{e}"]["device"]["median_ms"] / ta["one_shot"]["device"]["median_ms"]
    ta["streamed_equals_one_shot_bytes"] = True
    res["a_one_shot_against_streamed"] = ta
    del one_shot
    # (b)
    pub = all_idx[:a.publish_frames]
    tb = dict(list_points=int(len(pub)) * per, default_batch=measure(km, pub, a.leaf, 0, a.reps, a.warmup), one_shot=measure(km, pub, a.leaf, 2 ** 26, a.reps, a.warmup))
    gpu_b = km.globalMapPoints()
    res["b_publish_global_map"] = tb
    # (c)
    big = np.concatenate([all_idx, all_idx[::-1], all_idx])
    try:
        tc = dict(list_points=int(len(big)) * per)
        for e in (24, 26):
            tc[f"streamed_2^{e}"] = measure(km, big, a.leaf, 2 ** e, max(a.reps // 2, 3), 1)
        res["c_two_hundred_million_points"] = tc
    except Exception as ex:   # the device's memory does not allow it: say so
        res["c_two_hundred_million_points"] = dict(list_points=int(len(big)) * per, failed=str(ex))
    # (d)
    if a.oracle_reps > 0:
        ts = []
        for _ in range(a.oracle_reps):
            t0 = time.perf_counter(); want = oracle_compose(base, poses, pub.tolist(), a.leaf); ts.append((time.perf_counter() - t0) * 1e3)
        res["d_cpu_oracle_composition_of_b"] = dict(stats(ts), gpu_equals_oracle_bitwise=bool(want.shape == gpu_b.shape and np.array_equal(want.view(np.uint32), gpu_b.view(np.uint32))))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    km.close()


if __name__ == "__main__":
    main()
