"""Records the single loop ICP's results (rolo_loopicp_align + rolo_loopicp_get_trace) for the inputs of tests/loopicp_bits_cases.py into
tests/golden/loopicp_single_bits.npz: T, fitness, state, iterations, n_last, converged and every trace record's n, mse, sums and increment, as the GPU gave them.
tests/test_gpu_loopicp.py::test_single_form_bits_are_the_recorded_ones holds every later build to these bytes.

    python profiles/tools/record_loopicp_bits.py --commit $(git rev-parse HEAD) [--out FILE]

Record only at a commit whose single form is known good (the numpy twin's tests pass), and say which one: the file's `meta` carries it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loopicp_bits_cases as cases  # noqa: E402
from rolo_amd.backend import LoopIcp  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", cases.FILE))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("record_loopicp_bits.py needs a GPU")
    icp = LoopIcp()
    rec = cases.run(icp)
    again = cases.run(icp)
    icp.close()
    for k in rec:
        if not np.array_equal(cases.raw(rec[k]), cases.raw(again[k])):
            raise SystemExit("not reproducible from run to run: " + k)
    meta = dict(recorded_at_commit=a.commit, device=torch.cuda.get_device_name(0), what="LoopIcp.align + trace() per case of tests/loopicp_bits_cases.py",
                cases=len(rec["names"]), trace_records=int(rec["trace_start"][-1]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, meta=np.array(json.dumps(meta)), **rec)
    print(json.dumps(meta), os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
