"""Pose-graph optimisation on the device: where the time of one optimise goes, by graph size and loop count ("Pose graph").

For N in {1e3, 1e4, 6e4} key poses x {1, 10, 100} loops: a closed circuit driven twice (tests/pgo_twin.py's generator: odometry drifting by 2 mrad / 2 cm per
step, loops from truth plus 1 mrad / 1 cm, the reference's noise models and prior), every pose and factor added, then ONE optimise after the last loop with
GTSAM's default tolerances. Recorded into --out (profiles/r10/posegraph.json): the four parts of rolo_pgo_last_ms (linearise + assemble and retract + cost between
HIP events; the cyclic reduction's factorisation and the PCG loop, which share one launch, by the device's wall clock inside it), the host clock around the call,
the exit, iterations, trials and PCG iterations. `keyframe_call`: the zero-loop per-key-frame use, the median of --reps addOdomFactor + optimise calls on a graph of
N - reps poses without loops. `host_direct_solve_s`: scipy's sparse direct solve (spsolve, SuperLU on the host cores) of the SAME first linear system, taken from
the device's linearisation, wall clock: for scale, NOT a baseline (the reference's iSAM2 is incremental and cannot be built here). --cauchy K adds every loop
under a Cauchy(K) loss, as performSCLoopClosure does with K = 1 (profiles/r11/posegraph_robust.json); without it every factor is plain. --solve-form one | grid
takes the one-workgroup or the grid form of the linear solve (in the grid form the factorisation and PCG lie between HIP events); --repeats R runs every optimise on
R fresh graphs after an untimed one and records the medians, every repeat and the spread (profiles/r14/posegraph_grid.json: the parent's build, one, grid)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pgo_twin as tw  # noqa: E402
from rolo_amd.backend import PoseGraph  # noqa: E402


def fill(g, spec, n_between=None, cauchy=None):
    n = len(spec["initial"])
    for X in spec["initial"]:
        g.addPose(tw.T_of(X))
    g.addPrior(0, tw.T_of(spec["initial"][0]), tw.PRIOR_VARIANCES)
    for f, (i, j, T, v) in enumerate(spec["betweens"][:n_between]):
        if cauchy is None or f < n - 1:     # the odometry chain comes first and is always plain
            g.addBetween(i, j, T, v)
        else:
            g.addBetween(i, j, T, v, cauchy=cauchy)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "posegraph.json"))
    ap.add_argument("--sizes", default="1000,10000,60000")
    ap.add_argument("--loops", default="1,10,100")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-solve-max", type=int, default=60000, help="largest N whose first system is also solved on the host")
    ap.add_argument("--cauchy", type=float, default=None, help="every loop under a Cauchy loss with this constant")
    ap.add_argument("--repeats", type=int, default=1, help="above 1: each optimise is run on this many fresh graphs after one untimed one; the row holds the medians, "
                    "every repeat, and the spread (max - min) of the device total")
    ap.add_argument("--solve-form", default=None, choices=PoseGraph.SOLVE_FORMS if hasattr(PoseGraph, "SOLVE_FORMS") else None,
                    help="the form of the linear solve (PoseGraph.setSolveForm); without it the library's AUTO decides")
    a = ap.parse_args()
    rows = []
    for N in [int(x) for x in a.sizes.split(",")]:
        base = tw.circuit(N, 0, seed=N)
        # the zero-loop per-key-frame call
        g = PoseGraph()
        if a.solve_form: g.setSolveForm(a.solve_form)
        n0 = N - a.reps
        for X in base["initial"][:n0]:
            g.addPose(tw.T_of(X))
        g.addPrior(0, tw.T_of(base["initial"][0]), tw.PRIOR_VARIANCES)
        for i, j, T, v in base["betweens"][:n0 - 1]:
            g.addBetween(i, j, T, v)
        g.optimize()
        ms, wall, states = [], [], []
        for k in range(n0, N):
            t0 = time.perf_counter()
            g.addPose(tw.T_of(base["initial"][k]))
            g.addBetween(*base["betweens"][k - 1])
            r = g.optimize()
            wall.append(1e3 * (time.perf_counter() - t0)); ms.append(g.lastMs().astype(np.float64)); states.append((r["state"], r["iterations"], r["trials"]))
        g.close()
        key = dict(ms_linearise_factor_pcg_retract=[float(x) for x in np.median(np.array(ms), axis=0)], wall_ms=float(np.median(wall)), exits=sorted(set(states)))
        print(N, "per key frame", key, flush=True)
        for loops in [int(x) for x in a.loops.split(",")]:
            spec = tw.circuit(N, loops, seed=N)
            rep_ms, rep_wall = [], []
            for rep in range(a.repeats + (1 if a.repeats > 1 else 0)):
                if rep: g.close()
                g = PoseGraph()
                if a.solve_form: g.setSolveForm(a.solve_form)
                fill(g, spec, cauchy=a.cauchy)
                n, f, c = g.size()
                host = None
                if N <= a.host_solve_max and rep == 0:
                    lin = g.linearize()
                    t0 = time.perf_counter()
                    tw.Graph.solve_direct(lin, 1e-5)
                    host = time.perf_counter() - t0
                t0 = time.perf_counter()
                r = g.optimize()
                rep_wall.append(1e3 * (time.perf_counter() - t0)); rep_ms.append([float(x) for x in g.lastMs()])
            if a.repeats > 1: rep_ms, rep_wall = rep_ms[1:], rep_wall[1:]     # the first graph of a size and loop count is the warm-up
            totals = [sum(m) for m in rep_ms]
            row = dict(poses=n, factors=f, chords=c, state=PoseGraph.STATES[r["state"]], iterations=r["iterations"], trials=r["trials"], pcg_iterations=r["pcg_iterations"],
                       initial_cost=r["initial_cost"], final_cost=r["final_cost"], ms_linearise_factor_pcg_retract=[float(x) for x in np.median(np.array(rep_ms), axis=0)],
                       wall_ms=float(np.median(rep_wall)), device_total_ms=float(np.median(totals)), device_total_spread_ms=float(max(totals) - min(totals)),
                       repeats_ms=rep_ms if a.repeats > 1 else None,
                       pcg_per_trial=[t["pcg_iterations"] for t in g.trace()], host_direct_solve_s=host, keyframe_call=key, cauchy=a.cauchy,
                       solve_form=a.solve_form, solve_form_used=g.solveForm()[1] if a.solve_form else None)
            g.close()
            rows.append(row)
            print(row, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(dict(tool="profiles/tools/posegraph_time.py", note="device ms per optimise; host_direct_solve_s is scipy spsolve of the first system on the host, for scale only",
                       rows=rows), fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
