"""Sub-map assembly, CPU composition and upload route against the key map (ISSUE "assemble the back end's sub-map on the GPU").

Workload: 50 key frames of 1 500 corner and 30 000 surface points each in a synthetic hall (ground, two walls, a ceiling strip; poles and door edges),
2 m apart, fused at the reference's leaves 0.2 / 0.4. Records into --out (profiles/r07/submap.json):
  (i)   the CPU oracle's composition (get_transformation + transform_cloud_f + voxelgrid per cloud), OMP threads as the environment sets them
  (ii)  the parent's route: the finished sub-map uploaded through rolo_scan2map_set_submap (upload + two tree builds)
  (iii) rolo_keymap_extract alone                                                   — against (i)
  (iv)  rolo_keymap_extract + rolo_scan2map_set_submap_keymap                        — against (ii); the tree build inside it is reported on its own
  (vi)  median / maximum run length (points per cell) of the two sorts
Each figure: median of --reps calls after --warmup, with min / p10 / p90 / max. Host clock around calls that end in a device synchronise.
(v) per-kernel times: run this file with --loop-only under `rocprofv3 --kernel-trace --stats --output-format csv` in a run of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import pyorc  # noqa: E402
from rolo_amd.backend import KeyFrameMap, Scan2Map  # noqa: E402

f32 = np.float32


def make_keyframes(n_frames, n_corner, n_surf, seed=20):
    """sensor-frame clouds of a hall 16 m wide and 6 m high along x: planes (surface) and vertical poles / door edges (corner), 1 cm noise, 35 m range"""
    rng = np.random.default_rng(seed)
    frames = []
    for k in range(n_frames):
        yaw = 0.02 * np.sin(0.3 * k)
        pose = np.array([0.001 * np.sin(k), 0.001 * np.cos(k), yaw, 2.0 * k, 0.3 * np.sin(0.2 * k), 1.8], f32)
        x0 = float(pose[3])
        # surface: 45 % ground, 20 % each wall, 15 % ceiling strip
        parts = []
        for share, kind in ((0.45, "ground"), (0.2, "wall+"), (0.2, "wall-"), (0.15, "ceil")):
            m = int(round(share * n_surf))
            x = x0 + rng.uniform(-35, 35, m)
            if kind == "ground":
                p = np.stack([x, rng.uniform(-8, 8, m), np.zeros(m)], 1)
            elif kind == "ceil":
                p = np.stack([x, rng.uniform(-3, 3, m), np.full(m, 6.0)], 1)
            else:
                p = np.stack([x, np.full(m, 8.0 if kind == "wall+" else -8.0), rng.uniform(0, 6, m)], 1)
            parts.append(p)
        surf_w = np.concatenate(parts)[:n_surf]
        # corner: poles every 5 m along both walls, 0.3 m off the wall
        pole_x = 5.0 * np.round((x0 + rng.uniform(-35, 35, n_corner)) / 5.0)
        corner_w = np.stack([pole_x, np.where(rng.random(n_corner) < 0.5, 7.7, -7.7), rng.uniform(0, 6, n_corner)], 1)
        T = pyorc.get_transformation(*[float(v) for v in (pose[3], pose[4], pose[5], pose[0], pose[1], pose[2])]).reshape(4, 4).astype(np.float64)
        Ti = np.linalg.inv(T)
        out = []
        for w in (corner_w, surf_w):
            w = w + rng.normal(0, 0.01, w.shape)
            s = w @ Ti[:3, :3].T + Ti[:3, 3]
            out.append(np.concatenate([s, rng.uniform(0, 100, (len(s), 1))], 1).astype(f32))
        frames.append((out[0], out[1], pose, 0.5 * k))
    return frames


def oracle_compose(frames, leaves):
    fused = []
    for t in range(2):
        parts = []
        for fr in frames:
            p = [float(v) for v in fr[2]]
            T = pyorc.get_transformation(p[3], p[4], p[5], p[0], p[1], p[2])
            moved = fr[t].copy()
            moved[:, :3] = pyorc.transform_cloud_f(np.ascontiguousarray(fr[t][:, :3]), T)
            parts.append(moved)
        fused.append(np.concatenate(parts))
    return [pyorc.voxelgrid(fused[t], leaves[t]) for t in range(2)], fused


def run_lengths(pts, leaf):
    """points per occupied cell, with the filter's own float arithmetic for the cell coordinates"""
    inv = f32(1.0) / f32(leaf)
    ijk = np.floor(pts[:, :3] * inv).astype(np.int64)
    ijk -= ijk.min(axis=0)
    div = ijk.max(axis=0) + 1
    key = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    cnt = np.unique(key, return_counts=True)[1]
    return dict(cells=int(len(cnt)), median=float(np.median(cnt)), p99=float(np.percentile(cnt, 99)), max=int(cnt.max()))


def stats(ts):
    a = np.array(ts) * 1e3
    return dict(median_ms=float(np.median(a)), min_ms=float(a.min()), p10_ms=float(np.percentile(a, 10)), p90_ms=float(np.percentile(a, 90)), max_ms=float(a.max()), n=len(ts))


def timed(fn, reps, warmup, sync):
    for _ in range(warmup):
        fn(); sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); sync(); ts.append(time.perf_counter() - t0)
    return stats(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50); ap.add_argument("--corner", type=int, default=1500); ap.add_argument("--surf", type=int, default=30000)
    ap.add_argument("--reps", type=int, default=30); ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "r07", "submap.json"))
    ap.add_argument("--loop-only", type=int, default=0, help="only run extract + hand-over this many times (for a kernel trace)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("submap_time.py needs a GPU: a timing taken without one says nothing")
    sync = torch.cuda.synchronize
    leaves = (0.2, 0.4)
    frames = make_keyframes(a.frames, a.corner, a.surf)
    km = KeyFrameMap(0, *leaves)
    for c, s, pose, tm in frames:
        km.addKeyFrame(c, s, pose, tm)
    idx = list(range(a.frames))
    reg = Scan2Map()
    if a.loop_only:
        for _ in range(a.loop_only):
            km.extractCloud(idx); reg.setSubmapFrom(km); sync()
        return
    (wc, ws), fused = oracle_compose(frames, leaves)
    mc, ms = km.extractCloud(idx)
    gc, gs = km.submap()
    same = bool(np.array_equal(gc, wc) and np.array_equal(gs, ws))
    res = dict(workload=dict(frames=a.frames, corner_per_frame=a.corner, surf_per_frame=a.surf, fused_corner=int(len(fused[0])), fused_surf=int(len(fused[1])),
                             submap_corner=int(mc), submap_surf=int(ms), leaves=leaves, omp_threads=os.environ.get("OMP_NUM_THREADS", "unset")),
               gpu_equals_oracle_bitwise=same,
               run_length=dict(corner=run_lengths(fused[0], leaves[0]), surf=run_lengths(fused[1], leaves[1])))
    res["i_cpu_oracle_composition"] = timed(lambda: oracle_compose(frames, leaves), max(20, a.reps // 1), 2, lambda: None)
    reg2 = Scan2Map()
    res["ii_parent_route_set_submap_upload"] = timed(lambda: reg2.setSubmap(wc, ws), a.reps, a.warmup, sync)
    res["iii_extract"] = timed(lambda: km.extractCloud(idx), a.reps, a.warmup, sync)

    def both():
        km.extractCloud(idx); reg.setSubmapFrom(km)
    res["iv_extract_plus_set_submap_keymap"] = timed(both, a.reps, a.warmup, sync)
    km.extractCloud(idx)
    res["iv_tree_build_part_set_submap_keymap_alone"] = timed(lambda: reg.setSubmapFrom(km), a.reps, a.warmup, sync)
    res["iv_tree_build_share"] = res["iv_tree_build_part_set_submap_keymap_alone"]["median_ms"] / res["iv_extract_plus_set_submap_keymap"]["median_ms"]
    # one scan's downsampleCurrentScan for scale
    res["downsample_one_scan_surf_30000"] = timed(lambda: km.downsample(frames[0][1], leaves[1]), a.reps, a.warmup, sync)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    assert same, "the key map's sub-map differs from the oracle composition"


if __name__ == "__main__":
    main()
