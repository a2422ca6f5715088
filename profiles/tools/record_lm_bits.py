"""Records the LM chain's results in every launch form (register_async / register_wait, the batch wrapper, the stage-level evaluations, align + compute_translation) for
the cases of tests/lm_bits_cases.py into tests/golden/lm_forms_bits.npz: the double pose and the translation, the exit flags and counts, lm_form() and every trace
record, as the GPU gave them. tests/test_gpu_lm_bits.py holds every later build to these bytes.

    python profiles/tools/record_lm_bits.py --commit $(git rev-parse HEAD) [--out FILE]

Each environment of the cases runs in a child process of its own, twice in that process: nothing is written if the two runs differ. Record only at a commit whose LM
forms are known good (the form tests pass), and say which one: the file's `meta` carries it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lm_bits_cases as cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", cases.FILE))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("record_lm_bits.py needs a GPU")
    device = torch.cuda.get_device_name(0)
    rec, n_cases, n_trace, failed = {}, 0, 0, []
    for env in cases.ENVS:
        try:
            r = cases.run_child(env, runs=2)   # raises if the child's two runs differ
        except RuntimeError as e:
            print(e, flush=True); failed.append(env)
            continue
        n_cases += len(r["names"]); n_trace += int(r["trace_start"][-1])
        rec.update({cases.key(env, k): v for k, v in r.items()})
        print(env, len(r["names"]), "cases", int(r["trace_start"][-1]), "trace records", flush=True)
    if failed:
        raise SystemExit("nothing written: " + ", ".join(failed))
    meta = dict(recorded_at_commit=a.commit, device=device, what="the LM chain per case of tests/lm_bits_cases.py", environments={k: v for k, v in cases.ENVS.items()},
                cases=n_cases, trace_records=n_trace)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, meta=np.array(json.dumps(meta)), **rec)
    print(json.dumps(meta), os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
