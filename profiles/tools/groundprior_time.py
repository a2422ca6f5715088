"""The ground prior's device times ("Ground prior"): grid build, patch cut and the batched terrain pose solve.

Ground: a tilted plane (8 % and 5 %) with 2 cm noise, uniform at 41.7 points per square metre, so that a fit's 0.6 m disc holds about 47 neighbours, at 10^5
points (49 m a side) and 10^6 points (155 m a side). Vehicle and solver settings: rolo_priorpose_default_params (the shipped four wheels).

Records into --out (profiles/r17/groundprior.json) the median over --reps calls after --warmup of the device time between HIP events (rolo_ground_last_ms):
  grid_build   rolo_ground_set_cloud's kernels (box, keys, radix sort, cell starts, sorted points) — the host's packing and the upload are not inside the events
  patch        rolo_ground_extract_patch at groundPatchSize 20 m around the middle (count, scan, ordered copy), the copy back to the host not inside
  solve        rolo_priorpose_solve for B = 1, 40 (the ESKF's future path) and 4 096 poses spread over the middle 20 m, with the iteration counts it took
beside the host clock around each call. `statement_host_s` is tests/prior_twin.py (numpy, brute-force searches, one core) on the same poses, B = 1 and 40 only:
for scale, NOT a baseline — there is no device form of the reference to compare with, and its PCL / FLANN cannot be built here. What share of a solve the serial
ordered sums take is not measured: it would need stamps inside the kernel."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prior_twin as tw  # noqa: E402
from rolo_amd.backend import GroundModel, PriorPoseSolver  # noqa: E402

f32 = np.float32
DENSITY = 41.7


def ground(n, seed=1):
    rng = np.random.default_rng(seed)
    half = 0.5 * np.sqrt(n / DENSITY)
    xy = rng.uniform(-half, half, (n, 2))
    out = np.zeros((n, 5), f32)
    out[:, 0], out[:, 1] = xy[:, 0], xy[:, 1]
    out[:, 2] = 0.08 * xy[:, 0] - 0.05 * xy[:, 1] + 0.2 + 0.02 * rng.standard_normal(n)
    out[:, 3] = rng.uniform(0, 255, n)
    return out


def poses(B, seed=2):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(-10, 10, B), rng.uniform(-10, 10, B), rng.uniform(-np.pi, np.pi, B)])


def med(v):
    return float(np.median(np.array(v, np.float64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "groundprior.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 40, 4096])
    ap.add_argument("--statement-batches", type=int, nargs="+", default=[1, 40])
    a = ap.parse_args()
    rec = {"what": "device ms between HIP events (rolo_ground_last_ms), median of %d after %d warm-up calls; host_ms: the host clock around the same calls" % (a.reps, a.warmup),
           "ground": "tilted plane 8 %% / 5 %%, 2 cm noise, %.1f points per m^2" % DENSITY, "sizes": {}}
    gm = GroundModel()
    for n in a.sizes:
        cloud = ground(n)
        row = {}
        dev, host = [], []
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            gm.setCloud(cloud)
            host.append(1e3 * (time.perf_counter() - t0)); dev.append(gm.lastMs()[0])
        row["grid_build"] = {"device_ms": med(dev[a.warmup:]), "host_ms": med(host[a.warmup:]), **gm.info()}
        dev, host = [], []
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            patch = gm.extractPatch(0.0, 0.0, 20.0)
            host.append(1e3 * (time.perf_counter() - t0)); dev.append(gm.lastMs()[1])
        row["patch_20m"] = {"device_ms": med(dev[a.warmup:]), "host_ms": med(host[a.warmup:]), "points": int(patch.shape[0])}
        s = PriorPoseSolver(gm)
        row["solve"] = {}
        for B in a.batches:
            ps = poses(B)
            dev, host = [], []
            for k in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                r = s.solve(ps)
                host.append(1e3 * (time.perf_counter() - t0)); dev.append(gm.lastMs()[2])
            it = r["iterations"]
            row["solve"][str(B)] = {"device_ms": med(dev[a.warmup:]), "host_ms": med(host[a.warmup:]), "iterations_min_median_max": [int(it.min()), float(np.median(it)), int(it.max())],
                                    "converged": int((r["end_reason"] == 0).sum()), "success": int(r["success"].sum()),
                                    "mean_fit_hits": float(np.mean(s.fitSurface(ps[:min(B, 64), :2])["hits"]))}
            if B in a.statement_batches:
                t0 = time.perf_counter()
                for p in ps:
                    tw.solve(cloud, tw.Params(), *p)
                row["solve"][str(B)]["statement_host_s"] = time.perf_counter() - t0
        rec["sizes"][str(n)] = row
        print(n, json.dumps(row), flush=True)
    gm.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
