"""GPU: the translation stage's trials answered from the sums of its own linearisation (lm_step.hpp trans_step, trans_model.hpp, ROLO_LM_TRANS_MODEL).

Within the stage a trial's cost is a quadratic in the translation; the step that has just unpacked a linearisation takes the trials that follow itself and asks for a pass
only to linearise again after an accepted trial. Every case below runs the library in two child processes, ROLO_LM_TRANS_MODEL=1 and =0 (the parent form: every trial is
a pass), and compares
  identical:  the rotation stage (fp64 pose and every byte of its trace records), n_outer / n_passes / n_cost_only / converged / lm_failed of both stages, the trace
              count, and stage / outer / trial / accepted / y0 of every record;
  yi          within 1e-12 relative (150 x what the model differs from the oracle's compute_t_error on the CPU, tests/test_trans_model.py; seven orders under the
              smallest |rho| of the inputs, which that file asserts),
  rho         within 1e-9 absolute,  lambda and |d| within 1e-9 relative,  the translation within 1e-12 m.
rolo_ctx_counters' "model_trials" says that the model did (or did not) answer.

Inputs: os1-64 with every 8th column (8 192 points, UNIFORM leaf 1.0 m), the VLP-16 pair on the POLAR grid, the 4 096-point pair of tests/golden/os64_uniform.npz (whose
stage, behind a convergence-driven rotation stage, opens with a rejected trial), and, for the two sizes of the resident kernel, the bench's own 131 072-point pair."""
import json
import os
import re
import subprocess
import sys

import numpy as np
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
        clouds[name] = {"small": lambda: synth.dense_pair("os1-64", col_stride=8)[:2] + (1.0,), "mid": lambda: tuple(np.load(sys.argv[1] + "/tests/golden/os64_uniform.npz")[k] for k in ("source", "target")) + (1.0,),
                        "vlp": lambda: synth.dense_pair("vlp16", col_stride=2)[:2] + (None,), "big": lambda: synth.dense_pair("os1-128")[:2] + (0.5,)}[name]()
    return clouds[name]
def sha(b): return hashlib.sha256(b).hexdigest()
out = {}
for c in json.loads(sys.argv[2]):
    src, tgt, leaf = cloud(c.get("cloud", "small"))
    g = RotVGICP()
    if leaf is None: g.setPolarResolution(0.175, 0.175, 2.0)
    else: g.setResolution(leaf)
    g.setOptimizerType(c["opt"]); g.setFixedIterations(c["fixed"]); g.setFusedLm(c["fused"]); g.setUseGraph(bool(c.get("graph", 0))); g.setQ2Intended(bool(c.get("q2", 0)))
    if "nb" in c: g.setNeighborSearchMethod(c["nb"])
    if "hint" in c: g.setLoadHint(c["hint"])
    frames = []
    for k in range(c.get("frames", 1)):
        if c.get("sync"):
            g.setInputTarget(tgt); g.setInputSource(src)
            g.align(None); Td = g.final_transformation_d.copy()
            # the knobs computeTranslation reads when IT runs: the rotation stage before it is the one of the full solve
            if "trans_lm_max" in c: g.setLmMaxIterations(c["trans_lm_max"])
            if "trans_max_it" in c: g.setMaximumIterations(c["trans_max_it"])
            t = g.computeTranslation(np.zeros(3), G, L0)
        else:
            g.setInputTarget(tgt.copy()); g.setInputSource(src.copy())
            g.register_async(None, np.zeros(3), G, L0); Tf, Td, t = g.register_wait()
        stats = [g.last_stats, g.last_translation_stats]
        tr = g.trace()
        pk = lambda r: struct.pack("<4i5d", r["stage"], r["outer"], r["trial"], r["accepted"], r["y0"], r["yi"], r["rho"], r["lam"], r["dnorm"])
        frames.append(dict(T=sha(np.ascontiguousarray(Td, np.float64).tobytes()), t=[float(x) for x in t],
                           stats=[[s.n_outer, s.n_passes, s.n_cost_only, s.converged, s.lm_failed] for s in stats], n_trace=len(tr),
                           rot=sha(b"".join(pk(r) for r in tr if r["stage"] == 0)), n_rot=sum(1 for r in tr if r["stage"] == 0),
                           ident=sha(b"".join(struct.pack("<4id", r["stage"], r["outer"], r["trial"], r["accepted"], r["y0"]) for r in tr)),
                           tr=[[r["outer"], r["trial"], r["accepted"], r["y0"].hex(), r["yi"], r["rho"], r["lam"], r["dnorm"]] for r in tr if r["stage"] == 1]))
    cnt = g.counters()
    out[c["name"]] = dict(frames=frames, modelled=cnt["model_trials"], topup=cnt["topup_frames"], replays=cnt["graph_replays"], captures=cnt["graph_captures"], n_frames=cnt["frames"],
                          hint_trans=cnt["hint_trans"])
    g.close()
print(json.dumps(out))
"""


def run_ab(cases, **env):
    """the cases with ROLO_LM_TRANS_MODEL=1 and =0, one child process each: (on, off), name -> result"""
    res = []
    for model in ("1", "0"):
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(cases)], env=dict(os.environ, ROLO_LM_TRANS_MODEL=model, **env), capture_output=True, text=True,
                           timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        res.append(json.loads(r.stdout.strip().splitlines()[-1]))
    return res


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def same_solve(on, off, name):
    """the comparison of the module docstring; returns the flags of the first frame's translation stage ("A" accepted, "R" rejected, "C" rejected but converged)"""
    a, b = on[name]["frames"], off[name]["frames"]
    assert len(a) == len(b)
    worst = dict(yi=0.0, rho=0.0, lam=0.0, dnorm=0.0, t=0.0)
    for k, (fa, fb) in enumerate(zip(a, b)):
        for f in ("T", "stats", "n_trace", "rot", "n_rot", "ident"):
            assert fa[f] == fb[f], (name, k, f, fa[f], fb[f], fa["tr"], fb["tr"])
        assert len(fa["tr"]) == len(fb["tr"])
        for ra, rb in zip(fa["tr"], fb["tr"]):
            assert ra[:4] == rb[:4], (name, k, ra, rb)
            worst["yi"] = max(worst["yi"], rel(ra[4], rb[4])); worst["rho"] = max(worst["rho"], abs(ra[5] - rb[5]))
            worst["lam"] = max(worst["lam"], rel(ra[6], rb[6])); worst["dnorm"] = max(worst["dnorm"], rel(ra[7], rb[7]))
        worst["t"] = max(worst["t"], max(abs(x - y) for x, y in zip(fa["t"], fb["t"])))
    flags = "".join("RAC"[r[2]] for r in b[0]["tr"])
    print(name, flags, "modelled", on[name]["modelled"], "max rel dyi %.2e |drho| %.2e rel dlam %.2e rel d|d| %.2e |dt| %.2e" % (worst["yi"], worst["rho"], worst["lam"], worst["dnorm"], worst["t"]))
    assert worst["yi"] <= 1e-12 and worst["rho"] <= 1e-9 and worst["lam"] <= 1e-9 and worst["dnorm"] <= 1e-9 and worst["t"] <= 1e-12, (name, worst)
    assert off[name]["modelled"] == 0, (name, off[name]["modelled"])
    return flags


def case(name, **kw):
    d = dict(name=name, opt=SO3, fixed=20, fused=0); d.update(kw)
    return d


def main_cases():
    cs = []
    for f in FORMS:
        for cl in ("small", "vlp"):
            for q2 in (0, 1):
                for opt, tag in ((SO3, "so3"), (LM6, "lm6"), (GN, "gn")):
                    cs.append(case(f"{tag}_{cl}_q{q2}_f{f}", fused=f, opt=opt, cloud=cl, q2=q2))
        cs.append(case(f"graph_f{f}", fused=f, graph=1, frames=5))   # eager, eager (the hints move the schedule), captured, replayed, replayed
        cs.append(case(f"free_polar_f{f}", fused=f, fixed=0, cloud="vlp"))   # convergence-driven, POLAR grid
        cs.append(case(f"sync_f{f}", fused=f, sync=1, frames=3))     # rolo_align + rolo_compute_translation: the stage's own chain and its hint
        cs.append(case(f"nb7_f{f}", fused=f, nb=1))                  # DIRECT7: the generic bodies
        for m in range(1, 9):
            cs.append(case(f"lmmax{m}_f{f}", fused=f, sync=1, trans_lm_max=m))
        cs.append(case(f"mid_full_f{f}", fused=f, sync=1, fixed=0, cloud="mid"))   # convergence-driven: the translation stage behind it opens with a rejected trial
        for m in (1, 3):
            cs.append(case(f"mid_lmmax{m}_f{f}", fused=f, sync=1, fixed=0, trans_lm_max=m, cloud="mid"))
        for m in (0, 1, 2):
            cs.append(case(f"maxit{m}_f{f}", fused=f, sync=1, trans_max_it=m, q2=1))
    for hint in (0, 1):
        cs.append(case(f"big_f2_h{hint}", fused=2, hint=hint, cloud="big"))
    return cs


@pytest.fixture(scope="module")
def main_ab():
    return run_ab(main_cases())


@pytest.mark.parametrize("q2", (0, 1))
@pytest.mark.parametrize("cl", ("small", "vlp"))
@pytest.mark.parametrize("tag", ("so3", "lm6", "gn"))
@pytest.mark.parametrize("fused", FORMS)
def test_every_launch_form_optimiser_and_q2_variant(main_ab, fused, tag, cl, q2):
    on, off = main_ab
    name = f"{tag}_{cl}_q{q2}_f{fused}"
    flags = same_solve(on, off, name)
    assert len(flags) >= 2
    assert on[name]["modelled"] == len(flags), (flags, on[name]["modelled"])            # every trial of the stage was answered from the model
    st_on = on[name]["frames"][0]["stats"][1]
    assert st_on[1] > len(flags) - 1 and st_on[2] > 0                                  # ... and counted as the pass it replaced: n_passes, n_cost_only


@pytest.mark.parametrize("fused", FORMS)
def test_graph_frames_eager_captured_replayed(main_ab, fused):
    on, off = main_ab
    name = f"graph_f{fused}"
    flags = same_solve(on, off, name)
    assert on[name]["modelled"] == 5 * len(flags)
    for r in (on[name], off[name]):
        assert r["topup"] == 0 and r["captures"] >= 1 and r["replays"] >= 2 and r["n_frames"] == 5, r
    if fused != 2:   # the schedule is sized from the launches that ran (the resident kernel has none: its hint keys the graph and follows the solve's trials)
        assert on[name]["hint_trans"] < off[name]["hint_trans"], (on[name]["hint_trans"], off[name]["hint_trans"])


@pytest.mark.parametrize("fused", FORMS)
def test_convergence_driven_polar_and_direct7(main_ab, fused):
    on, off = main_ab
    for name in (f"free_polar_f{fused}", f"nb7_f{fused}"):
        flags = same_solve(on, off, name)
        assert on[name]["modelled"] == len(flags) > 0


@pytest.mark.parametrize("fused", FORMS)
def test_synchronous_drivers_own_chain(main_ab, fused):
    on, off = main_ab
    name = f"sync_f{fused}"
    flags = same_solve(on, off, name)
    assert on[name]["modelled"] == 3 * len(flags)


@pytest.mark.parametrize("fused", FORMS)
def test_lm_max_iterations_cuts_the_ladder(main_ab, fused):
    """computeTranslation with lm_max_iterations 1 .. 8 behind a full rotation stage, on a stage that runs A R R R R R R (R) C: "lm not converged" after an accept (1), inside the ladder (2 .. 7), not at all (long enough);
    and on a stage that opens with a rejected trial: on its first trial"""
    on, off = main_ab
    full = same_solve(on, off, f"so3_small_q0_f{fused}")
    assert full[0] == "A" and full[-1] == "C" and set(full[1:-1]) == {"R"}, full
    ladder = len(full) - 1   # trials of the second outer iteration
    failed = []
    for m in range(1, 9):
        name = f"lmmax{m}_f{fused}"
        flags = same_solve(on, off, name)
        st = on[name]["frames"][0]["stats"][1]
        failed.append(st[4])
        assert st[4] == (1 if m < ladder else 0), (m, flags, st)
        assert flags == (full[:1 + m] if m < ladder else full), (m, flags, full)
        assert on[name]["modelled"] == len(flags)
    assert failed[0] == 1 and 0 in failed
    full_mid = same_solve(on, off, f"mid_full_f{fused}")
    assert full_mid[:3] == "RRR" and on[f"mid_full_f{fused}"]["modelled"] == len(full_mid), full_mid
    for m in (1, 3):
        name = f"mid_lmmax{m}_f{fused}"
        flags = same_solve(on, off, name)
        assert flags == "R" * m and on[name]["frames"][0]["stats"][1][4] == 1 and on[name]["frames"][0]["stats"][1][0] == 1, (flags, on[name]["frames"][0]["stats"])
        assert on[name]["modelled"] == m


@pytest.mark.parametrize("fused", FORMS)
def test_max_iterations(main_ab, fused):
    on, off = main_ab
    for m in (0, 1, 2):
        name = f"maxit{m}_f{fused}"
        flags = same_solve(on, off, name)
        st = on[name]["frames"][0]["stats"][1]
        assert st[0] == min(m, st[0]) and flags.count("A") <= m, (m, flags, st)
        if m == 0:
            assert flags == "" and on[name]["modelled"] == 0 and on[name]["frames"][0]["t"] == [0.0, 0.0, 0.0]
        else:
            assert on[name]["modelled"] == len(flags) > 0


@pytest.mark.parametrize("hint", [0, 1])
def test_resident_kernel_both_sizes(main_ab, hint):
    """256 workgroups of one point per thread on an idle device, 64 of four per thread on a busy one, on the bench's own pair"""
    on, off = main_ab
    name = f"big_f2_h{hint}"
    flags = same_solve(on, off, name)
    assert on[name]["modelled"] == len(flags) >= 8 and on[name]["topup"] == 0 and off[name]["topup"] == 0


def test_trace_cap_inside_one_ladder(main_ab):
    """forced rotation iterations such that the rotation stage leaves TRACE_CAP - 4 records: the translation stage's ladder crosses the cap. Past it only the count and
    n_passes advance (the count beyond TRACE_CAP is not readable through the C ABI: rolo_get_trace returns min(count, TRACE_CAP))"""
    _, base = main_ab
    cap = trace_cap()
    cases = []
    for f in FORMS:
        n20 = base[f"so3_small_q0_f{f}"]["frames"][0]["n_rot"]   # 20 forced iterations leave this many records; every further one repeats a converged-but-rejected trial: one more
        cases.append(case(f"cap_f{f}", fused=f, fixed=20 + (cap - 4 - n20)))
    on, off = run_ab(cases)
    for f in FORMS:
        name = f"cap_f{f}"
        same_solve(on, off, name)
        full = len(base[f"so3_small_q0_f{f}"]["frames"][0]["tr"])
        fr = on[name]["frames"][0]
        assert fr["n_rot"] == cap - 4 and fr["n_trace"] == cap and len(fr["tr"]) == 4, (fr["n_rot"], fr["n_trace"], len(fr["tr"]))
        assert fr["stats"][1][1] == base[f"so3_small_q0_f{f}"]["frames"][0]["stats"][1][1]    # n_passes went on past the cap
        assert on[name]["modelled"] == full


def test_with_speculative_linearisation_off():
    """ROLO_LM_SPEC_LIN=0: every pass the model replaces would have carried both halves — the counts say so (no cost-only passes), the solve is the same"""
    cases = [case(f"spec0_f{f}", fused=f) for f in FORMS]
    on, off = run_ab(cases, ROLO_LM_SPEC_LIN="0")
    for c in cases:
        flags = same_solve(on, off, c["name"])
        assert on[c["name"]]["modelled"] == len(flags)
        assert on[c["name"]]["frames"][0]["stats"][1][2] == 0


def test_scripted_translation_is_driven_pass_by_pass():
    """rolo_debug_lm_script_translation names a cost per trial: the model answers none (counter 0) and the trace holds the script's costs, bit for bit"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from lm_scenarios import make_script, ROT_SCENARIOS, TRANS_SCENARIOS
    from rolo_amd import synth
    from rolo_amd.rotvgicp import RotVGICP
    G = -np.asarray(synth.PREV_STEP_T)
    for name in sorted(TRANS_SCENARIOS):
        params, outers = TRANS_SCENARIOS[name]
        script = make_script(6, outers, seed=11)
        g = RotVGICP(); g.setOptimizerType(SO3)
        assert g.script_align(make_script(3, ROT_SCENARIOS["iteration_cap_one"][1]), None) == 0
        for k, v in params.items():
            setattr(g._p, k, v)
        g._push()
        rc, _ = g.script_translation(script, np.array([0.01, -0.02, 0.005]), G, G * 0.97)
        assert rc == 0
        tr = [r for r in g.trace() if r["stage"] == 1]
        err_y = np.asarray(script[4], float)
        for r in tr:
            want = err_y[min(r["outer"], err_y.shape[0] - 1), min(r["trial"], err_y.shape[1] - 1)]
            assert r["yi"] == want or (np.isnan(r["yi"]) and np.isnan(want)), (name, r, want)
        assert g.counters()["model_trials"] == 0, name
        assert g.last_translation_stats.n_passes >= len(tr)
        g.close()
