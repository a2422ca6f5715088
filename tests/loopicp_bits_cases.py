"""The single loop ICP's recorded bits (tests/golden/loopicp_single_bits.npz): the inputs, which are those of tests/test_gpu_loopicp_batch.py's "batch equals
single" comparisons, and the record's layout. Shared by the recorder (profiles/tools/record_loopicp_bits.py) and tests/test_gpu_loopicp.py."""
import numpy as np

from rolo_amd.backend import loop_icp_params
from test_gpu_loopicp_batch import SIZES, mixed_batch, motion, xyzi

f32 = np.float32
FILE = "loopicp_single_bits.npz"


def cases():
    """(name, source, target, params, guess) in a fixed order"""
    for nt in (65, 5000):   # test_batch_equals_single_bit_for_bit
        rng = np.random.default_rng(100 + nt)
        tgt = rng.uniform(-10, 10, (nt, 3)).astype(f32)
        srcs = [rng.uniform(-10, 10, (n, 3)).astype(f32) for n in SIZES]
        guesses = np.stack([motion((0.01 * b, -0.02, 0.03 * b), (0.1 * b, -0.2, 0.05)).astype(f32) for b in range(len(SIZES))])
        guesses[2] = np.eye(4, dtype=f32)
        for with_guess in (False, True):
            for b, s in enumerate(srcs):
                yield "sizes nt %d guess %d ns %d" % (nt, with_guess, len(s)), s, tgt, loop_icp_params(4.0, max_iterations=30), guesses[b] if with_guess else None
    tgt, srcs = mixed_batch()   # test_mixed_exits_in_one_batch, test_mixed_exits_with_an_iteration_limit
    for limit in (None, 3):
        for b, s in enumerate(srcs):
            yield "mixed limit %s candidate %d" % (limit, b), s, tgt, loop_icp_params(2.0) if limit is None else loop_icp_params(2.0, max_iterations=limit), None


def run(icp):
    """every case through LoopIcp.align + trace(): the record's arrays (the trace records of all cases one after another, case k's at trace_start[k] : trace_start[k + 1])"""
    names, T, fit, ints, start, tn, tmse, tsums, tinc = [], [], [], [], [0], [], [], [], []
    for name, src, tgt, P, guess in cases():
        r = icp.align(xyzi(src), xyzi(tgt), P, guess)
        tr = icp.trace()
        names.append(name); T.append(r["T"]); fit.append(r["fitness"])
        ints.append([r["state"], r["iterations"], r["n_last"], int(r["converged"])])
        for x in tr:
            tn.append(x["n"]); tmse.append(x["mse"]); tsums.append(x["sums"]); tinc.append(x["increment"].reshape(16))
        start.append(len(tn))
    return dict(names=np.array(names), T=np.array(T, f32).reshape(-1, 4, 4), fitness=np.array(fit, np.float64), state_iterations_nlast_converged=np.array(ints, np.int32),
                trace_start=np.array(start, np.int64), trace_n=np.array(tn, np.int32), trace_mse=np.array(tmse, np.float64),
                trace_sums=np.array(tsums, np.float64).reshape(-1, 17), trace_increment=np.array(tinc, f32).reshape(-1, 16))


def raw(a):
    """an array as its bytes: a NaN equals itself, a negative zero differs from a positive one"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.kind in "fiu" else a
