"""Time of a projection with a de-skew armed WITHOUT times (azimuth_flag_kernel + azimuth_time_kernel in front of K1 / K2) beside one armed with handed-over times
and an un-armed one, between events on the context's stream; a 131 072-point frame, median of --reps projections. A projection through rolo_project_frame
includes the copies of the frame to the device and of the range image back, the same in all three forms: the azimuth kernels are the difference of the first two.

    python profiles/tools/azimuth_time.py [--reps 50] [--out FILE.json]        (ROLO_HIP_LIB=... for another build of the library)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from rolo_amd import _lib, synth                                               # noqa: E402
from rolo_amd.frontend import FrontEnd, deskew_params, front_params             # noqa: E402
from rolo_amd.rotvgicp import RotVGICP                                          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("azimuth_time.py needs a GPU: a timing taken without one says nothing")
    fr = synth.make_frame("os1-128", np.eye(3), np.zeros(3), synth.SEED)
    xyz = np.asarray(fr.xyz, np.float32); ring = np.asarray(fr.ring, np.uint16)
    order = np.argsort(-np.arctan2(xyz[:, 1], xyz[:, 0]), kind="stable")[:131072]
    xyz = np.ascontiguousarray(xyz[order]); ring = np.ascontiguousarray(ring[order])
    n = len(ring)
    g = RotVGICP()
    fe = FrontEnd(g, front_params(n_scan=128, horizon_scan=1024))
    stream = torch.cuda.ExternalStream(_lib.lib().rolo_ctx_stream(g._h))
    d = deskew_params([0.004, -0.006, 0.035], 0.1, 0.0987)
    times = np.linspace(0, 0.1, n).astype(np.float32)
    arm = {"azimuth": lambda: fe.setDeskewFromCloud(d), "times": lambda: fe.setDeskew(d, times), "unarmed": lambda: None}
    res = {"library": _lib.LIB_PATH, "points": n, "reps": a.reps}
    for _ in range(5):
        for f in arm.values():
            f(); fe.project(xyz, ring)
    ms = {k: [] for k in arm}
    for _ in range(a.reps):
        for k, f in arm.items():                                                 # interleaved: drift hits the three forms alike
            f()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); fe.project(xyz, ring); e1.record(stream); e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    for k in arm:
        v = np.sort(np.array(ms[k]))
        res[k + "_us"] = dict(median=round(1e3 * float(np.median(v)), 1), p10=round(1e3 * float(v[len(v) // 10]), 1), p90=round(1e3 * float(v[(9 * len(v)) // 10]), 1))
    res["azimuth_minus_times_us"] = round(res["azimuth_us"]["median"] - res["times_us"]["median"], 1)
    g.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
