"""Loop-closure ICP on the key map: assembly, tree build, iteration and fitness-pass times ("Loop closure").

The reference's shape: one key frame against 51 (historyKeyframeSearchNum 25), downSizeFilterICP at 0.4, setMaxCorrespondenceDistance 60 (the RS form,
2 x historyKeyframeSearchRadius) and 150 (the SC form). Scene: synthetic VLP-16 frames on two laps of an ellipse through the hall, 60 key frames a lap; key
frame 89 stands where 29 stood, so its loop cloud is matched against key frames 4 .. 54.

Records into --out (profiles/r09/loop_icp.json), per form: the sizes, the exit, and the median over --reps calls after --warmup of the device time between HIP
events (rolo_keymap_loop_last_ms): assembly of each loop cloud, set-up (guess, curve sort of both clouds, the target's tree), all iterations and the time per
iteration, the fitness pass, the whole ICP call; beside them the host clock around the calls. `kdtree_cpu` is the numpy twin's ICP loop with scipy's cKDTree for
the association (query on 16 host threads, tree build included) on the same clouds, wall clock: for scale, NOT a baseline (the reference's PCL cannot be built
here), and its iterations need not equal the device's to the last one (a kd-tree's double distances break ties otherwise)."""
import argparse
import json
import os
import sys
import time

import numpy as np
from scipy.spatial import cKDTree
from scipy.spatial.transform import Rotation

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_twin as T  # noqa: E402
from oracle import pyorc  # noqa: E402
from rolo_amd import synth  # noqa: E402
from rolo_amd.backend import KeyFrameMap, loop_icp_params  # noqa: E402

f32 = np.float32
LEAF, SEARCH_NUM, CUR, PRE = 0.4, 25, 89, 29


def scene_pose(k):
    kk = k % 60
    phi = kk * 2.0 * np.pi / 60.0
    yaw = 0.01 * kk + (0.05 if k >= 60 else 0.0)
    return synth.rpy_to_R(0.0, 0.0, yaw), np.array([20.0 * np.cos(phi) + (0.3 if k >= 60 else 0.0), 12.0 * np.sin(phi), 0.0])


def med(v):
    return float(np.median(np.array(v, np.float64)))


def kdtree_icp(src, tgt, cap, threads):
    """the twin's loop (tests/icp_twin.py) with a kd-tree association"""
    t0 = time.perf_counter()
    tree = cKDTree(tgt[:, :3].astype(np.float64))
    t_build = time.perf_counter() - t0
    cur = src[:, :3].copy(); Tt = np.eye(4, dtype=f32); prev = np.finfo(np.float64).max; it = 0; state = 0
    while True:
        d, i = tree.query(cur.astype(np.float64), workers=threads)
        keep = d * d <= cap * cap
        if keep.sum() < 3:
            state = T.NO_CORRESPONDENCES
            break
        p = cur[keep].astype(np.float64); q = tgt[i[keep], :3].astype(np.float64); d2 = (d[keep] ** 2)
        sums = np.concatenate([[len(p)], [d2.sum()], p.sum(0), q.sum(0), (p[:, :, None] * q[:, None, :]).sum(0).ravel()])
        R, t = T.umeyama(sums)
        inc = np.eye(4, dtype=f32); inc[:3, :3] = R; inc[:3, 3] = t
        cur = T.transform(inc, cur); Tt = T.matmul4(inc, Tt); it += 1
        mse = sums[1] / sums[0]
        cosa = 0.5 * (float(inc[0, 0]) + float(inc[1, 1]) + float(inc[2, 2]) - 1.0); tsq = float((inc[:3, 3].astype(np.float64) ** 2).sum())
        if it >= 100: state = T.ITERATIONS; break
        if cosa >= 1.0 - 1e-6 and tsq <= 1e-6: state = T.TRANSFORM; break
        if mse < 1e-12: state = T.ABS_MSE; break
        if abs(mse - prev) / prev < 1e-6: state = T.REL_MSE; break
        prev = mse
    d, _ = tree.query(cur.astype(np.float64), workers=threads)
    return dict(state=state, iterations=it, fitness=float((d * d).mean()), tree_build_ms=t_build * 1e3, wall_ms=(time.perf_counter() - t0) * 1e3, threads=threads)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--col-stride", type=int, default=1); ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join("profiles", "r09", "loop_icp.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("loop_icp_time.py needs a GPU: a timing taken without one says nothing")
    fo = pyorc.front_params(n_scan=16, horizon_scan=1800)
    R0, t0 = scene_pose(0)
    maps = dict(RS=KeyFrameMap(), SC=KeyFrameMap())   # RS: poses as they are, clouds by their own poses; SC: poses relative to key 0, clouds by key 0's pose
    t_gen = time.perf_counter()
    for k in range(CUR + 1):
        Rk, tk = scene_pose(k)
        fr = synth.make_frame("vlp16", Rk, tk, synth.SEED + k, col_stride=a.col_stride)
        e = pyorc.extract_features(fo, pyorc.project(fo, fr.xyz, fr.ring))
        c, s = pyorc.voxelgrid(e["corner"], 0.2), pyorc.voxelgrid(e["surface"], 0.4)
        maps["RS"].addKeyFrame(c, s, np.concatenate([Rotation.from_matrix(Rk).as_euler("xyz"), tk]).astype(f32), float(k))
        maps["SC"].addKeyFrame(c, s, np.concatenate([Rotation.from_matrix(R0.T @ Rk).as_euler("xyz"), R0.T @ (tk - t0)]).astype(f32), float(k))
    res = dict(workload=dict(key_frames=CUR + 1, cur=CUR, pre=PRE, search_num=SEARCH_NUM, leaf=LEAF, col_stride=a.col_stride, reps=a.reps, warmup=a.warmup,
                             scene_seconds=time.perf_counter() - t_gen))
    for form, cap, wrt in (("RS", 60.0, None), ("SC", 150.0, 0)):
        km = maps[form]
        P = loop_icp_params(cap)
        rows, host = [], []
        for r in range(a.reps + a.warmup):
            h0 = time.perf_counter()
            ns = km.loopCloud(0, CUR, 0, wrt, LEAF); nt = km.loopCloud(1, PRE, SEARCH_NUM, wrt, LEAF)
            h1 = time.perf_counter()
            out = km.loopIcp(P)
            h2 = time.perf_counter()
            if r >= a.warmup:
                rows.append(km.loopLastMs().astype(np.float64)); host.append(((h1 - h0) * 1e3, (h2 - h1) * 1e3))
        ms = np.array(rows); host = np.array(host)
        it = max(out["iterations"], 1)
        rec = dict(max_correspondence_distance=cap, wrt_key=wrt, n_source=ns, n_target=nt, state=out["state"], iterations=out["iterations"], fitness=out["fitness"],
                   n_last=out["n_last"],
                   device_ms=dict(assembly_source=med(ms[:, 4]), assembly_target=med(ms[:, 5]), setup_sort_and_tree=med(ms[:, 0]), iterations_total=med(ms[:, 1]),
                                  per_iteration=med(ms[:, 1]) / it, fitness_pass=med(ms[:, 2]), icp_total=med(ms[:, 3]),
                                  total_with_assembly=med(ms[:, 3] + ms[:, 4] + ms[:, 5]), icp_total_min=float(ms[:, 3].min()), icp_total_max=float(ms[:, 3].max())),
                   host_clock_ms=dict(assembly_both=med(host[:, 0]), icp_call=med(host[:, 1])))
        src, tgt = km.loopCloudPoints(0, ns), km.loopCloudPoints(1, nt)
        rec["kdtree_cpu_for_scale_not_a_baseline"] = kdtree_icp(src, tgt, cap, a.threads)
        res[form] = rec
        km.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
