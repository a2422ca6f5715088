"""GPU: the LM chain in its three launch forms (pass + controller launches, one launch per trial, the resident kernel) against the bytes recorded on an MI355X at the
commit the record's meta names (tests/golden/lm_forms_bits.npz, profiles/tools/record_lm_bits.py; cases and layout: lm_bits_cases.py).

The form tests compare with the oracle at 1e-8 to 1e-10: a sum taken in another order, or a product that stopped being fused into its addition, passes them. Here the
double pose, the translation, the exits and counts and every trace record's y0, yi, rho, lambda and |d| are compared byte for byte, per environment of switches (one
child process each: the switches are read once per process)."""
import os

import numpy as np
import pytest

import lm_bits_cases as rec

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("env", list(rec.ENVS))
def test_lm_forms_give_the_recorded_bits(golden_dir, env):
    want = np.load(os.path.join(golden_dir, rec.FILE))
    print(str(want["meta"]))
    got = rec.run_child(env)
    mine = {k.split("/", 1)[1]: want[k] for k in want.files if k.startswith(env + "/")}
    assert sorted(got) == sorted(mine)
    assert got["names"].tolist() == mine["names"].tolist() and len(got["names"]) == rec.N_CASES[env]
    diff = rec.differences(got, mine)
    if diff:
        first = diff[0][1][0] if isinstance(diff[0][1], list) else 0
        case = int(np.searchsorted(got["trace_start"], first, side="right")) - 1 if diff[0][0].startswith("trace_") else first
        raise AssertionError(("arrays and their first rows that differ", diff, "first case", str(got["names"][min(case, len(got["names"]) - 1)])))
