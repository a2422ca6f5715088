"""GPU: forced LM iterations answered from the kept cost (lm_step.hpp rot_step_t, ROLO_LM_KEEP_COST) change no observable bit.

With fixed_iterations > 0 the rotation stage, once a trial is rejected although the step has converged, repeats that very trial until the iterations are used up. The step
takes those repeats itself instead of asking for one pass each. Every case below runs the library in two child processes, ROLO_LM_KEEP_COST=1 and =0 (the parent form:
every repeat is a pass), and compares as hashes of the raw bytes: the fp64 pose, the translation, n_outer / n_passes / n_cost_only / converged / lm_failed of both stages,
the number of trace records and every field of every record. rolo_ctx_counters' "kept_trials" says that the shortcut did (or did not) fire.
(The trace count past TRACE_CAP is not readable through the C ABI — rolo_get_trace returns min(count, TRACE_CAP); n_passes advances with it, one per record of a stage,
and is compared.)

Inputs: os1-64 with every 8th column (8 192 points), UNIFORM leaf 1.0 m — the oracle, single-threaded and therefore repeatable, takes well over five
converged-but-rejected iterations of 20 on it with both LM optimisers (checked below on the CPU) — and, for the two sizes of the resident kernel (256 workgroups of one point
per thread on an idle device, 64 of four per thread on a busy one), the bench's own 131 072-point pair."""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO3, LM6, GN = 2, 1, 0   # rolo_hip.h ROLO_OPT_*
FORMS = (0, 1, 2)        # pass + controller launches, one launch per trial, the resident kernel


def trace_cap():
    m = re.search(r"constexpr int TRACE_CAP = (\d+);", open(os.path.join(ROOT, "rolo_amd", "csrc", "rolo_internal.hpp")).read())
    return int(m.group(1))


_CHILD = r"""
import sys, json, hashlib, struct
import numpy as np
sys.path.insert(0, sys.argv[1])
from rolo_amd import synth
from rolo_amd.rotvgicp import RotVGICP
G = -np.asarray(synth.PREV_STEP_T); L0 = G * 0.97
clouds = {}
def cloud(name):
    if name not in clouds:
        clouds[name] = synth.dense_pair("os1-64", col_stride=8)[:2] + (1.0,) if name == "small" else synth.dense_pair("os1-128")[:2] + (0.5,)
    return clouds[name]
def sha(b): return hashlib.sha256(b).hexdigest()
out = {}
for c in json.loads(sys.argv[2]):
    src, tgt, leaf = cloud(c.get("cloud", "small"))
    g = RotVGICP(); g.setResolution(leaf); g.setOptimizerType(c["opt"]); g.setFixedIterations(c["fixed"]); g.setFusedLm(c["fused"]); g.setUseGraph(bool(c.get("graph", 0)))
    if "hint" in c: g.setLoadHint(c["hint"])
    frames = []
    for k in range(c.get("frames", 1)):
        if c.get("align"):
            g.setInputTarget(tgt); g.setInputSource(src)
            g.align(None); Td = g.final_transformation_d.copy(); t = np.zeros(3)
            stats = [g.last_stats]
        else:
            g.setInputTarget(tgt.copy()); g.setInputSource(src.copy())
            g.register_async(None, np.zeros(3), G, L0); Tf, Td, t = g.register_wait()
            stats = [g.last_stats, g.last_translation_stats]
        tr = g.trace()
        rec = b"".join(struct.pack("<4i5d", r["stage"], r["outer"], r["trial"], r["accepted"], r["y0"], r["yi"], r["rho"], r["lam"], r["dnorm"]) for r in tr)
        frames.append(dict(T=sha(np.ascontiguousarray(Td, np.float64).tobytes()), t=sha(np.ascontiguousarray(t, np.float64).tobytes()),
                           stats=[[s.n_outer, s.n_passes, s.n_cost_only, s.converged, s.lm_failed] for s in stats], n_trace=len(tr), trace=sha(rec),
                           rot=[[r["outer"], r["trial"], r["accepted"]] for r in tr if r["stage"] == 0][:64]))
    cnt = g.counters()
    out[c["name"]] = dict(frames=frames, kept=cnt["kept_trials"], topup=cnt["topup_frames"], replays=cnt["graph_replays"], captures=cnt["graph_captures"], n_frames=cnt["frames"])
    g.close()
print(json.dumps(out))
"""


def run_ab(cases, **env):
    """the cases with ROLO_LM_KEEP_COST=1 and =0, one child process each: (on, off), name -> result"""
    res = []
    for keep in ("1", "0"):
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(cases)], env=dict(os.environ, ROLO_LM_KEEP_COST=keep, **env), capture_output=True, text=True,
                           timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        res.append(json.loads(r.stdout.strip().splitlines()[-1]))
    return res


def same_observables(on, off, name):
    a, b = on[name]["frames"], off[name]["frames"]
    assert len(a) == len(b)
    for k, (fa, fb) in enumerate(zip(a, b)):
        for f in ("T", "t", "stats", "n_trace", "trace", "rot"):
            assert fa[f] == fb[f], (name, k, f, fa, fb)
    assert off[name]["kept"] == 0, (name, off[name])


def case(name, **kw):
    d = dict(name=name, opt=SO3, fixed=20, fused=0); d.update(kw)
    return d


def main_cases():
    cs = []
    for f in FORMS:
        cs.append(case(f"so3_f{f}", fused=f))
        cs.append(case(f"so3_f{f}_graph", fused=f, graph=1, frames=5))   # eager, eager (the hints move the schedule), captured, replayed, replayed
        cs.append(case(f"cut3_f{f}", fused=f, fixed=3))
        cs.append(case(f"free_f{f}", fused=f, fixed=0))
        cs.append(case(f"cap_f{f}", fused=f, fixed=trace_cap() + 100))
        cs.append(case(f"lm6_f{f}", fused=f, opt=LM6))
        cs.append(case(f"gn_f{f}", fused=f, opt=GN))
    for f in (0, 2):
        cs.append(case(f"align_f{f}", fused=f, align=1, frames=2))       # the synchronous driver (its own hint update)
    for hint in (0, 1):
        cs.append(case(f"big_f2_h{hint}", fused=2, hint=hint, cloud="big"))
        cs.append(case(f"big_f2_h{hint}_graph", fused=2, hint=hint, cloud="big", graph=1, frames=5))
    return cs


@pytest.fixture(scope="module")
def main_ab():
    return run_ab(main_cases())


def test_oracle_takes_converged_but_rejected_iterations_on_the_input():
    """the precondition, on the CPU: the oracle (one thread: a repeatable summation order) ends at least five of the 20 forced iterations converged-but-rejected"""
    from oracle import pyorc
    from rolo_amd import synth
    src, tgt, _ = synth.dense_pair("os1-64", col_stride=8)
    for opt in (pyorc.OPT_SO3_LM, pyorc.OPT_LM):
        o = pyorc.Reg(pyorc.default_params(voxel_type=pyorc.VOXEL_UNIFORM, voxel_resolution=1.0, fixed_iterations=20, optimizer=opt, num_threads=1))
        o.set_target(tgt); o.set_source(src)
        rc, _, _, it, _ = o.align(None)
        acc = [r["accepted"] for r in o.trace() if r["stage"] == 0]
        assert rc == 0 and it == 20 and sum(1 for a in acc if a == 2) >= 5, (opt, acc)


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("fused", FORMS)
def test_every_launch_form(main_ab, fused, graph):
    on, off = main_ab
    name = f"so3_f{fused}" + ("_graph" if graph else "")
    same_observables(on, off, name)
    acc = [r[2] for r in off[name]["frames"][0]["rot"]]
    n_rep = sum(1 for x, y in zip(acc, acc[1:]) if x == 2 and y == 2)
    assert n_rep >= 5, acc                                                    # the run of repeats is there on the device too
    assert on[name]["kept"] == n_rep * len(on[name]["frames"]), (on[name]["kept"], n_rep)   # ... and every one of them was answered from the kept cost
    for r in (on[name], off[name]):
        assert r["topup"] == 0, r                                             # the first schedule held every launch the frame needed
        if graph:
            assert r["captures"] >= 1 and r["replays"] >= 2 and r["n_frames"] == 5, r


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("hint", [0, 1])
def test_resident_kernel_both_sizes(main_ab, hint, graph):
    on, off = main_ab
    name = f"big_f2_h{hint}" + ("_graph" if graph else "")
    same_observables(on, off, name)
    assert on[name]["kept"] > 0 and on[name]["topup"] == 0 and off[name]["topup"] == 0
    if graph:
        assert on[name]["replays"] >= 2 and off[name]["replays"] >= 2


@pytest.mark.parametrize("fused", (0, 2))
def test_synchronous_driver(main_ab, fused):
    on, off = main_ab
    same_observables(on, off, f"align_f{fused}")
    assert on[f"align_f{fused}"]["kept"] > 0


@pytest.mark.parametrize("fused", FORMS)
def test_shortcut_never_fires(main_ab, fused):
    on, off = main_ab
    for name in (f"cut3_f{fused}", f"free_f{fused}"):
        same_observables(on, off, name)
        assert on[name]["kept"] == 0, on[name]
    cut = [r[2] for r in on[f"cut3_f{fused}"]["frames"][0]["rot"]]
    assert len(cut) >= 3 and 2 not in cut[:-1], cut                           # cut off before it converged
    free = [r[2] for r in on[f"free_f{fused}"]["frames"][0]["rot"]]
    assert free.count(2) <= 1 and 2 not in free[:-1], free                    # convergence-driven: a converged rejection ends the stage


@pytest.mark.parametrize("fused", FORMS)
def test_trace_cap(main_ab, fused):
    on, off = main_ab
    name = f"cap_f{fused}"
    same_observables(on, off, name)
    cap = trace_cap()
    f = on[name]["frames"][0]
    assert f["n_trace"] == cap and f["stats"][0][0] == cap + 100 and f["stats"][0][1] > cap   # the trace filled up during the repeats, the counts went on
    assert on[name]["kept"] > cap - 64


@pytest.mark.parametrize("fused", FORMS)
def test_other_optimisers(main_ab, fused):
    on, off = main_ab
    same_observables(on, off, f"lm6_f{fused}")
    assert on[f"lm6_f{fused}"]["kept"] > 0
    same_observables(on, off, f"gn_f{fused}")
    assert on[f"gn_f{fused}"]["kept"] == 0                                    # Gauss-Newton rejects nothing
    assert all(r[2] == 1 for r in on[f"gn_f{fused}"]["frames"][0]["rot"])


def test_edges_zero_and_one_repeat(main_ab):
    """fixed_iterations such that the first converged-but-rejected trial is the last forced iteration (the shortcut's exit with nothing left to repeat), and one more
    (exactly one repeat); the value is read from each form's own trace of the =0 run (the forms sum their rows in different shapes: the first such trial may differ)"""
    _, off = main_ab
    cases, first = [], {}
    for f in FORMS:
        rot = off[f"so3_f{f}"]["frames"][0]["rot"]
        o = next(r[0] for r in rot if r[2] == 2)
        first[f] = o
        cases += [case(f"zero_f{f}", fused=f, fixed=o + 1), case(f"one_f{f}", fused=f, fixed=o + 2)]
    on, off = run_ab(cases)
    for f in FORMS:
        for name, reps in ((f"zero_f{f}", 0), (f"one_f{f}", 1)):
            same_observables(on, off, name)
            acc = [r[2] for r in off[name]["frames"][0]["rot"]]
            assert acc.count(2) == reps + 1 and acc[-(reps + 1):] == [2] * (reps + 1), (first[f], acc)
            assert on[name]["kept"] == reps, on[name]


def test_with_speculative_linearisation_off():
    """ROLO_LM_SPEC_LIN=0: the repeated pass would also have run its (B) half — into the correspondence buffer that is not current and the Mahalanobis cache — and
    nothing observable comes of it"""
    cases = [case(f"spec0_f{f}", fused=f) for f in FORMS] + [case(f"spec0_lm6_f{f}", fused=f, opt=LM6) for f in FORMS]
    on, off = run_ab(cases, ROLO_LM_SPEC_LIN="0")
    for c in cases:
        same_observables(on, off, c["name"])
        assert on[c["name"]]["kept"] > 0
        assert on[c["name"]]["frames"][0]["stats"][0][2] == 0                 # no cost-only passes in either
