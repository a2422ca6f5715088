"""The mapping node's per-scan step ("The per-scan step"): wall time per scan of the call-by-call route against rolo_mapper_scan.

Scans: the VLP-16 trajectory of tests/test_gpu_mapper.py (13 frames, 16 x 1800, the oracle front end's features, 0.6 m and 0.5 s apart). Twelve key frames (scans
0 .. 11 at their true poses, down-sampled at 0.2 / 0.4) are resident before the clock starts and stay twelve: the saveFrame thresholds are out of reach, so no
measured scan is saved. The 200 measured scans walk the trajectory up and down (0, 1, .. 12, 11, .. 0, 1, ..), each with its true pose as the odometry guess.

  --leg A   the call-by-call route of INTEGRATION.md: rolo_keyposes_select_nearby, rolo_keymap_extract, rolo_scan2map_set_submap_keymap, two rolo_keymap_downsample,
            rolo_scan2map_optimize on host clouds, and the node's float bookkeeping in numpy. It uses only calls that exist before the mapper does, so that it can be
            taken at the commit before (and, for the comparison of like with like, at this one too: --name A_here).
  --leg B   MapOptimization.scan (rolo_mapper_scan), with rolo_mapper_last_ms's parts.
Both legs report the median and the mean of the host clock around one scan after --warmup scans, and the poses they end at. A leg is merged into --out
(profiles/r20/mapper.json) under its name."""
import argparse
import json
import os
import sys
import time

import numpy as np
from scipy.spatial.transform import Rotation

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import pyorc  # noqa: E402
from rolo_amd import synth  # noqa: E402
from rolo_amd.backend import KeyFrameMap, Scan2Map, PoseGraph, pose6_to_T  # noqa: E402

f32 = np.float32
CFG = dict(n_scan=16, horizon_scan=1800)
CORNER_LEAF, SURF_LEAF, DENSITY, RADIUS = 0.2, 0.4, 2.0, 50.0
N_KEYS = 12
FAR = 1e9   # saveFrame thresholds no step reaches


def frame_pose(k):
    R = synth.rpy_to_R(0.002 * k, -0.001 * k, 0.03 * k)
    t = np.array([0.6 * k, 0.05 * k, 0.0])
    return R, t, np.concatenate([Rotation.from_matrix(R).as_euler("xyz"), t]).astype(f32)


def trajectory():
    fo = pyorc.front_params(**CFG)
    out = []
    for k in range(13):
        R, t, pose = frame_pose(k)
        fr = synth.make_frame("vlp16", R, t, synth.SEED + k)
        e = pyorc.extract_features(fo, pyorc.project(fo, fr.xyz, fr.ring))
        out.append((e["corner"], e["surface"], pose))
    return out


def walk(n):
    """0, 1, .. 12, 11, .. 1, 0, 1, .."""
    return [abs((i + 12) % 24 - 12) for i in range(n)]


def preload(km, graph, traj):
    """twelve key frames at their true poses, the graph's chain beside them"""
    prev = None
    for k in range(N_KEYS):
        c, s, pose = traj[k]
        km.addKeyFrame(pyorc.voxelgrid(c, CORNER_LEAF), pyorc.voxelgrid(s, SURF_LEAF), pose, 0.5 * k)
        T = pose6_to_T(pose, np.float64)
        graph.addPose(T)
        if prev is None:
            graph.addPrior(0, T, PoseGraph.PRIOR_VARIANCES)
        else:
            graph.addBetween(k - 1, k, np.linalg.inv(prev) @ T, PoseGraph.ODOM_VARIANCES)
        prev = T


# ---- leg A's float bookkeeping: updateInitialGuess and saveFrame in numpy float32 (the library's statement is rolo_mapper_initial_guess / _save_frame) ----
def aff(p):
    return pose6_to_T(p, f32)


def pose_of(T):
    return np.array([np.arctan2(T[2, 1], T[2, 2]), np.arcsin(-T[2, 0]), np.arctan2(T[1, 0], T[0, 0]), T[0, 3], T[1, 3], T[2, 3]], f32)


def leg_a(traj, n, warmup):
    km, s2m, graph = KeyFrameMap(0, CORNER_LEAF, SURF_LEAF), Scan2Map(), PoseGraph()
    preload(km, graph, traj)
    tf, last, wall, its = np.zeros(6, f32), None, [], []
    for i, k in enumerate(walk(n)):
        c, s, guess = traj[k]
        stamp = 6.0 + 0.5 * i
        t0 = time.perf_counter()
        back = aff(guess)                                                                  # updateInitialGuess :516-555
        if last is not None:
            tf = pose_of((aff(tf) @ (np.linalg.inv(last) @ back)).astype(f32))
        last = back
        km.extractCloud(km.selectNearby(stamp, RADIUS, DENSITY, 10.0))                      # extractSurroundingKeyFrames
        s2m.setSubmapFrom(km)
        cds, sds = km.downsample(c, CORNER_LEAF), km.downsample(s, SURF_LEAF)               # downsampleCurrentScan
        tf = s2m.scan2MapOptimization(cds, sds, None, None, tf)                             # scan2MapOptimization
        between = pose_of((np.linalg.inv(aff(km.poses[-1])) @ aff(tf)).astype(f32))         # saveFrame :1071-1091
        assert np.abs(between[:3]).max() < FAR and np.linalg.norm(between[3:]) < FAR
        wall.append(1e3 * (time.perf_counter() - t0))
        its.append(s2m.last_stats.iterations)
    err = np.abs(tf - traj[walk(n)[-1]][2])
    for x in (s2m, graph, km):
        x.close()
    w = np.array(wall[warmup:])
    return {"wall_ms_median": float(np.median(w)), "wall_ms_mean": float(w.mean()), "scans": int(len(w)), "s2m_iterations_mean": float(np.mean(its[warmup:])),
            "key_frames": N_KEYS, "last_pose_error": [float(v) for v in err]}


def leg_b(traj, n, warmup):
    from rolo_amd.backend import MapOptimization, mapper_params
    m = MapOptimization(0, mapper_params(mappingSurfLeafSize=SURF_LEAF, surroundingKeyframeDensity=DENSITY, surroundingkeyframeAddingDistThreshold=FAR,
                                         surroundingkeyframeAddingAngleThreshold=FAR))
    preload(m.keymap, m.graph, traj)
    wall, parts, its, kept = [], [], [], 0
    for i, k in enumerate(walk(n)):
        c, s, guess = traj[k]
        t0 = time.perf_counter()
        r = m.scan(6.0 + 0.5 * i, c, s, initialGuess=guess)
        wall.append(1e3 * (time.perf_counter() - t0))
        assert r["processed"] and r["keyframe"] == -1
        parts.append(m.lastMs()); its.append(r["s2m"][1]); kept += int(not r["submap_rebuilt"])
    err = np.abs(r["transformTobeMapped"] - traj[walk(n)[-1]][2])
    m.close()
    w, p = np.array(wall[warmup:]), np.median(np.array(parts[warmup:], np.float64), axis=0)
    names = ("downsample", "submap", "scan2map", "commit", "graph", "total")
    return {"wall_ms_median": float(np.median(w)), "wall_ms_mean": float(w.mean()), "scans": int(len(w)), "s2m_iterations_mean": float(np.mean(its[warmup:])),
            "key_frames": N_KEYS, "submaps_kept": kept, "device_ms_median": {a: float(v) for a, v in zip(names, p)}, "last_pose_error": [float(v) for v in err]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["A", "B"], required=True)
    ap.add_argument("--name", default=None, help="key in the output file (default: the leg)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "mapper.json"))
    ap.add_argument("--scans", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    traj = trajectory()
    res = (leg_a if a.leg == "A" else leg_b)(traj, a.scans + a.warmup, a.warmup)
    rec = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            rec = json.load(f)
    rec.setdefault("what", "host clock around one scan of the mapping node's step, ms; 12 resident key frames, no scan saved; A: call by call, B: rolo_mapper_scan "
                           "(device_ms_median: rolo_mapper_last_ms's parts)")
    rec[a.name or a.leg] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(a.name or a.leg, json.dumps(res))


if __name__ == "__main__":
    main()
