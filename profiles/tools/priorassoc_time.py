"""The ground-prior association's ICPs ("Ground-prior association"): B stored patches against the laser's ground patch, as ONE
rolo_loopicp_align_batch call and as B rolo_loopicp_align calls one after another (the path before the batch form existed: the baseline).

Ground: prior_assoc_cases' kind of terrain — a curved ground with three ripples of 0.08 .. 0.15 m, so that no direction is left to slide along — uniform at
41.7 points per square metre (profiles/r17's density). The target is the patch of groundPatchSize 2 m and 20 m around the origin; candidate b is every second
point of it with 3 mm of noise, moved back by its own small motion (up to 0.03 rad and 0.1 m per axis), so the candidates take different numbers of iterations.
Settings: GroundPriorCloser's (cap = groundPatchSize, 100 iterations, both epsilons 1e-6).

Records into --out (profiles/r18/priorassoc.json), per patch size and B = 1 / 4 / 16 / 64, the median over --reps runs after --warmup of the device time between
HIP events, set-up (sorts, tree, tables) and iterations (with the fitness passes) separately, and the host clock around the calls:
  batch    rolo_loopicp_batch_last_ms of the one call
  serial   the sums of rolo_loopicp_last_ms over the B calls
and ratio = serial / batch for each. The results of the two routes are compared bit for bit on the way (`same_bits`)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from rolo_amd import synth  # noqa: E402
from rolo_amd.backend import LoopIcp, loop_icp_params  # noqa: E402

f32 = np.float32
DENSITY = 41.7


def ground(half, seed=1):
    rng = np.random.default_rng(seed)
    n = int(DENSITY * (2 * half) ** 2)
    x, y = rng.uniform(-half, half, n), rng.uniform(-half, half, n)
    z = 0.01 * x * x - 0.008 * y * y + 0.03 * x
    for _ in range(3):
        amp, lam, th, ph = rng.uniform(0.08, 0.15), rng.uniform(0.9, 2.0), rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
        z = z + amp * np.sin(2 * np.pi * (np.cos(th) * x + np.sin(th) * y) / lam + ph)
    out = np.zeros((n, 4), f32)
    out[:, 0], out[:, 1], out[:, 2] = x, y, z
    return out


def candidate(patch, b):
    rng = np.random.default_rng(100 + b)
    M = np.eye(4)
    M[:3, :3] = synth.rpy_to_R(*rng.uniform(-0.03, 0.03, 3)); M[:3, 3] = rng.uniform(-0.1, 0.1, 3)
    p = patch[::2, :3].astype(np.float64) + rng.normal(0, 0.003, (len(patch[::2]), 3))
    out = np.zeros((len(p), 4), f32)
    out[:, :3] = ((p - M[:3, 3]) @ M[:3, :3]).astype(f32)
    return out


def med(v):
    return np.median(np.array(v, np.float64), axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "priorassoc.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--patch-sizes", type=float, nargs="+", default=[2.0, 20.0])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 16, 64])
    a = ap.parse_args()
    rec = {"what": "device ms between HIP events, median of %d after %d warm-up runs; host_ms: the host clock around the same calls; ratio = serial / batch" % (a.reps, a.warmup),
           "ground": "curved ground with ripples, %.1f points per m^2; candidates: every second point, 3 mm noise, own small motion" % DENSITY, "patch_sizes": {}}
    icp_b, icp_s = LoopIcp(), LoopIcp()
    for size in a.patch_sizes:
        g = ground(0.5 * size + 1.0)
        h = 0.5 * size
        target = g[(np.abs(g[:, 0]) <= h) & (np.abs(g[:, 1]) <= h)]
        P = loop_icp_params(size, max_iterations=100, transformation_epsilon=1e-6, euclidean_fitness_epsilon=1e-6)
        row = {"target_points": int(len(target)), "batches": {}}
        for B in a.batches:
            srcs = [candidate(target, b) for b in range(B)]
            bat, ser, hb, hs = [], [], [], []
            same = True
            for k in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                rb = icp_b.alignBatch(srcs, target, P)
                hb.append(1e3 * (time.perf_counter() - t0))
                m = icp_b.batchLastMs()
                bat.append([m[0], m[1], m[3]])
                acc = np.zeros(3)
                t0 = time.perf_counter()
                rs = []
                for s in srcs:
                    rs.append(icp_s.align(s, target, P))
                    m = icp_s.lastMs()
                    acc += [m[0], m[1] + m[2], m[3]]
                hs.append(1e3 * (time.perf_counter() - t0))
                ser.append(acc)
                same = same and all(x["T"].tobytes() == y["T"].tobytes() and x["fitness"] == y["fitness"] and x["iterations"] == y["iterations"] for x, y in zip(rb, rs))
            it = np.array([r["iterations"] for r in rb])
            mb, ms = med(bat[a.warmup:]), med(ser[a.warmup:])
            names = ("setup_ms", "iterations_ms", "total_ms")
            row["batches"][str(B)] = {
                "source_points": int(len(srcs[0])), "iterations_min_median_max_sum": [int(it.min()), float(np.median(it)), int(it.max()), int(it.sum())],
                "converged": int(sum(r["converged"] for r in rb)), "same_bits": bool(same),
                "batch": {**{n: float(v) for n, v in zip(names, mb)}, "host_ms": float(med(hb[a.warmup:]))},
                "serial": {**{n: float(v) for n, v in zip(names, ms)}, "host_ms": float(med(hs[a.warmup:]))},
                "ratio": {**{n: float(s / b) if b > 0 else None for n, s, b in zip(names, ms, mb)}, "host_ms": float(med(hs[a.warmup:]) / med(hb[a.warmup:]))}}
            print(size, B, json.dumps(row["batches"][str(B)]), flush=True)
        rec["patch_sizes"][str(size)] = row
    icp_b.close(); icp_s.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
