"""GPU: the batched loop ICP (rolo_loopicp_align_batch, rolo_amd/csrc/loopicp.hip) — B sources against one target with every candidate's association in one
launch per iteration — against the single form (rolo_loopicp_align) bit for bit, and against the numpy twin (tests/icp_twin.py) as tests/test_gpu_loopicp.py
holds the single form. A candidate's bits may depend on nothing but its own source, the target, the settings and its guess: not on its place in the batch, its
neighbours, or how long they iterate."""
import ctypes as C

import numpy as np
import pytest

import icp_twin as T
from rolo_amd._lib import lib, LoopIcpResult, LoopIcpTraceRec
from rolo_amd.backend import LoopIcp, loop_icp_params
from test_icp_twin import CASES, moved_pair, motion, room

pytestmark = pytest.mark.gpu

f32 = np.float32
BAR_M, BAR_RAD = 1e-4, 1e-5   # BASELINE.json
EINVAL = -1


def xyzi(xyz):
    return np.concatenate([np.asarray(xyz, f32)[:, :3], np.zeros((len(xyz), 1), f32)], axis=1)


@pytest.fixture(scope="module")
def icp():
    h = LoopIcp()
    yield h
    h.close()


@pytest.fixture(scope="module")
def single():
    """the single form runs in a context of its own: what it leaves behind cannot help the batch"""
    h = LoopIcp()
    yield h
    h.close()


def bits(res, trace):
    """everything the issue compares: T, fitness, state, iterations, n_last, converged and every trace record's n, mse, sums and increment"""
    return (res["T"].tobytes(), np.float64(res["fitness"]).tobytes(), res["state"], res["iterations"], res["n_last"], res["converged"], res["n_source"], res["n_target"],
            [(x["n"], np.float64(x["mse"]).tobytes(), x["sums"].tobytes(), x["increment"].tobytes()) for x in trace])


def run_single(single, src, tgt, P, guess=None):
    r = single.align(xyzi(src), xyzi(tgt), P, guess)
    return bits(r, single.trace())


def run_batch(icp, srcs, tgt, P, guesses=None):
    rs = icp.alignBatch([xyzi(s) for s in srcs], xyzi(tgt), P, guesses)
    assert len(rs) == len(srcs)
    return [bits(r, icp.traceBatch(b)) for b, r in enumerate(rs)]


def assert_same(got, want, what=""):
    assert np.array_equal(np.frombuffer(got[0], f32), np.frombuffer(want[0], f32)), what                    # T
    assert np.array_equal(np.frombuffer(got[1], np.uint64), np.frombuffer(want[1], np.uint64)), what      # fitness, as bits
    assert got[2:8] == want[2:8], (what, got[2:8], want[2:8])
    assert len(got[8]) == len(want[8]), (what, len(got[8]), len(want[8]))
    for k, (a, b) in enumerate(zip(got[8], want[8])):
        assert a == b, (what, "trace record", k)


SIZES = (3, 63, 64, 65, 256, 257, 2000)


@pytest.mark.parametrize("with_guess", [False, True])
@pytest.mark.parametrize("nt", [65, 5000])
def test_batch_equals_single_bit_for_bit(icp, single, nt, with_guess):
    """seven sources of 3 .. 2000 points (below a wavefront, at and around one, at and around a workgroup, eight workgroups) in one batch"""
    rng = np.random.default_rng(100 + nt)
    tgt = rng.uniform(-10, 10, (nt, 3)).astype(f32)
    srcs = [rng.uniform(-10, 10, (n, 3)).astype(f32) for n in SIZES]
    guesses = None
    if with_guess:
        guesses = np.stack([motion((0.01 * b, -0.02, 0.03 * b), (0.1 * b, -0.2, 0.05)).astype(f32) for b in range(len(SIZES))])
        guesses[2] = np.eye(4, dtype=f32)   # an identity among them: the single form does not move that source
    P = loop_icp_params(4.0, max_iterations=30)
    got = run_batch(icp, srcs, tgt, P, guesses)
    iters = []
    for b, s in enumerate(srcs):
        want = run_single(single, s, tgt, P, None if guesses is None else guesses[b])
        assert_same(got[b], want, "ns %d nt %d" % (len(s), nt))
        iters.append(want[3])
    print("nt", nt, "guess", with_guess, "iterations", iters, "ms", icp.batchLastMs())


def mixed_batch():
    tgt = room(1500, 9, 0.01)
    src, _, _ = moved_pair(n_tgt=1500, n_src=400, seed=9)
    far = (room(300, 4) + np.array([500.0, 0.0, 0.0], f32)).astype(f32)
    long_src, _, _ = moved_pair(n_tgt=1500, n_src=700, seed=9, M=motion((0.03, -0.02, 0.08), (0.4, -0.3, 0.1)))
    # equal to the target: out after one iteration; ordinary; wholly beyond the cap; empty; a larger motion: many iterations
    return tgt, [tgt, src, far, src[:0], long_src]


def test_mixed_exits_in_one_batch(icp, single):
    tgt, srcs = mixed_batch()
    P = loop_icp_params(2.0)
    got = run_batch(icp, srcs, tgt, P)
    want = [run_single(single, s, tgt, P) for s in srcs]
    for b in range(len(srcs)):
        assert_same(got[b], want[b], "candidate %d" % b)
    states, iters = [w[2] for w in want], [w[3] for w in want]
    print("states", states, "iterations", iters)
    assert states[0] == T.TRANSFORM and iters[0] == 1
    assert states[2] == T.NO_CORRESPONDENCES and iters[2] == 0 and len(want[2][8]) == 2      # the refused association and the fitness pass
    assert states[3] == T.NO_CORRESPONDENCES and len(want[3][8]) == 0                         # empty: no association at all
    assert iters[1] > 1 and iters[4] > 1 and iters[4] != iters[1]   # of the test's own inputs: three different times to leave the loop
    # a finished candidate's fitness is that of its own final cloud: the twin's final cloud of candidate 1, associated once more
    tw = T.icp(srcs[1], tgt, max_correspondence_distance=2.0)
    fit = np.frombuffer(got[1][1], np.float64)[0]
    assert abs(fit - tw["fitness"]) <= 1e-6 * tw["fitness"] + 1e-12


def test_mixed_exits_with_an_iteration_limit(icp, single):
    """max_iterations = 3 ends the long candidates at ITERATIONS while the one that equals the target left after one"""
    tgt, srcs = mixed_batch()
    P = loop_icp_params(2.0, max_iterations=3)
    got = run_batch(icp, srcs, tgt, P)
    want = [run_single(single, s, tgt, P) for s in srcs]
    for b in range(len(srcs)):
        assert_same(got[b], want[b], "candidate %d" % b)
    assert want[4][2] == T.ITERATIONS and want[4][3] == 3 and want[0][3] == 1


def test_composition_and_run_to_run(icp):
    """candidate b gives the same bits alone, first, last and between others; the same batch twice gives the same bits"""
    tgt, srcs = mixed_batch()
    P = loop_icp_params(2.0)
    a, b, c = srcs[1], srcs[4], srcs[0]
    alone = run_batch(icp, [a], tgt, P)[0]
    first = run_batch(icp, [a, b, c], tgt, P)
    last = run_batch(icp, [b, c, a], tgt, P)
    between = run_batch(icp, [b, a, c], tgt, P)
    assert_same(first[0], alone, "first"); assert_same(last[2], alone, "last"); assert_same(between[1], alone, "between")
    again = run_batch(icp, [b, a, c], tgt, P)
    for k in range(3):
        assert_same(again[k], between[k], "second run, candidate %d" % k)


@pytest.mark.parametrize("state", sorted(CASES))
def test_a_mixed_batch_equals_the_twin(icp, state):
    """test_icp_twin's CASES are settings, and a batch has one set of them: under each case's settings one batch of its constructed pair, a second source with a
    larger motion, a cloud beyond any cap and the target itself, each candidate held to the twin as tests/test_gpu_loopicp.py holds the single form"""
    kw = CASES[state]
    noise = 0.0 if state == T.ABS_MSE else 0.01
    src, tgt, _ = moved_pair(noise=noise)
    src2 = moved_pair(noise=noise, M=motion((0.02, 0.01, 0.05), (0.3, -0.2, 0.1)))[0]
    far = (room(300, 4) + np.array([500.0, 0.0, 0.0], f32)).astype(f32)
    srcs = [src, src2, far, tgt]
    rs = icp.alignBatch([xyzi(s) for s in srcs], xyzi(tgt), loop_icp_params(**kw))
    for b, s in enumerate(srcs):
        want = T.icp(s, tgt, **kw)
        got, tr = rs[b], icp.traceBatch(b)
        print("candidate", b, "state", got["state"], want["state"], "iterations", got["iterations"], want["iterations"], "margin", want["margin"])
        if b == 0:
            assert want["margin"] > 1e-3 and want["state"] == state   # of the test's own inputs, as test_gpu_loopicp.py asserts it
        if want["margin"] > 1e-3:
            assert got["state"] == want["state"] and got["iterations"] == want["iterations"] and got["converged"] == want["converged"]
            assert [x["n"] for x in tr] == [x["n"] for x in want["trace"]]
            dt = np.linalg.norm(got["T"][:3, 3].astype(np.float64) - want["T"][:3, 3])
            dr = T.rot_angle(got["T"][:3, :3].astype(np.float64) @ want["T"][:3, :3].astype(np.float64).T)
            print("pose against the twin: %.3g m %.3g rad" % (dt, dr))
            assert dt <= BAR_M and dr <= BAR_RAD, (b, dt, dr)


def test_batch_of_one_and_of_the_limit(icp, single):
    rng = np.random.default_rng(77)
    tgt = rng.uniform(-5, 5, (900, 3)).astype(f32)
    P = loop_icp_params(3.0, max_iterations=4)
    one = rng.uniform(-5, 5, (70, 3)).astype(f32)
    assert_same(run_batch(icp, [one], tgt, P)[0], run_single(single, one, tgt, P), "B = 1")
    B = LoopIcp.MAX_BATCH
    assert B == 256
    srcs = [rng.uniform(-5, 5, (70, 3)).astype(f32) for _ in range(B)]
    got = run_batch(icp, srcs, tgt, P)
    for b in (0, 1, 100, B - 2, B - 1):
        assert_same(got[b], run_single(single, srcs[b], tgt, P), "B = 256, candidate %d" % b)
    assert len({g[0] for g in got}) == B   # 256 different clouds, 256 different poses


def test_empty_batch_and_bad_arguments(icp):
    assert icp.alignBatch([], np.zeros((10, 4), f32)) == []
    L, h = lib(), icp.reg._h
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    src = np.zeros((8, 4), f32); tgt = np.ones((8, 4), f32)
    ns = np.array([4, 4], np.int32)
    P = loop_icp_params(1.0)
    out = (LoopIcpResult * 2)()
    s, t, n = src.ctypes.data_as(fp), tgt.ctypes.data_as(fp), ns.ctypes.data_as(ip)
    call = L.rolo_loopicp_align_batch
    assert call(h, s, n, 2, t, 8, C.byref(P), None, out) == 0
    assert call(h, None, None, 0, None, 0, C.byref(P), None, None) == 0          # B == 0 touches nothing
    assert call(None, s, n, 2, t, 8, C.byref(P), None, out) == EINVAL
    assert call(h, None, n, 2, t, 8, C.byref(P), None, out) == EINVAL
    assert call(h, s, None, 2, t, 8, C.byref(P), None, out) == EINVAL
    assert call(h, s, n, 2, None, 8, C.byref(P), None, out) == EINVAL
    assert call(h, s, n, 2, t, 8, None, None, out) == EINVAL
    assert call(h, s, n, 2, t, 8, C.byref(P), None, None) == EINVAL
    assert call(h, s, n, -1, t, 8, C.byref(P), None, out) == EINVAL
    assert call(h, s, n, 257, t, 8, C.byref(P), None, out) == EINVAL
    assert call(h, s, n, 2, t, -1, C.byref(P), None, out) == EINVAL
    assert call(h, s, n, 2, t, (1 << 26) + 1, C.byref(P), None, out) == EINVAL
    neg = np.array([4, -1], np.int32)
    assert call(h, s, neg.ctypes.data_as(ip), 2, t, 8, C.byref(P), None, out) == EINVAL
    big = np.array([1 << 26, 1], np.int32)                                        # the sum passes the limit; no point is read
    assert call(h, s, big.ctypes.data_as(ip), 2, t, 8, C.byref(P), None, out) == EINVAL
    rec = (LoopIcpTraceRec * 4)()
    assert L.rolo_loopicp_get_trace_batch(h, -1, rec, 4) == EINVAL
    assert L.rolo_loopicp_get_trace_batch(h, 2, rec, 4) == EINVAL                 # the last batch had two candidates
    assert L.rolo_loopicp_get_trace_batch(h, 0, None, 4) == EINVAL
    assert L.rolo_loopicp_get_trace_batch(None, 0, rec, 4) == EINVAL
    assert L.rolo_loopicp_batch_last_ms(h, None) == EINVAL and L.rolo_loopicp_batch_last_ms(None, None) == EINVAL
    # an empty target: every candidate NO_CORRESPONDENCES, as the single form
    rs = icp.alignBatch([src, src[:0]], tgt[:0], P)
    assert [r["state"] for r in rs] == [T.NO_CORRESPONDENCES] * 2 and not any(r["converged"] for r in rs)


def trace_bits(trace):
    return bits(dict(T=np.zeros(16, f32), fitness=0.0, state=0, iterations=0, n_last=0, converged=0, n_source=0, n_target=0), trace)[8]


def test_one_context_serves_both_call_kinds():
    """align, alignBatch, align, associate in ONE context, whose scratch, events and control records the call kinds share: every result is a fresh context's,
    the single form's records survive a batch call and the batch's survive a single call"""
    rng = np.random.default_rng(78)
    tgt = rng.uniform(-5, 5, (900, 3)).astype(f32)
    one = rng.uniform(-5, 5, (70, 3)).astype(f32)
    srcs = [rng.uniform(-5, 5, (n, 3)).astype(f32) for n in (3, 257, 2000)]
    P = loop_icp_params(3.0, max_iterations=6)
    Tm = motion((0.01, -0.02, 0.03), (0.1, -0.2, 0.05)).astype(f32)
    h, fresh = LoopIcp(), LoopIcp()
    try:
        want = run_single(fresh, one, tgt, P)
        want_i, want_d = fresh.associate(xyzi(one), xyzi(tgt), Tm, 3.0)
        want_sums = fresh.trace()[-1]["sums"].tobytes()
        first = run_single(h, one, tgt, P)
        assert_same(first, want, "first align")
        batch = run_batch(h, srcs, tgt, P)
        assert trace_bits(h.trace()) == first[8]                      # read after the batch call: still the first align's
        second = run_single(h, one, tgt, P)
        assert_same(second, want, "align after a batch")
        for b in range(len(srcs)):                                    # the batch's records are unchanged by the later align
            assert trace_bits(h.traceBatch(b)) == batch[b][8], b
            fresh2 = LoopIcp()                                        # each candidate against a context that has seen nothing else
            try:
                assert_same(batch[b], run_single(fresh2, srcs[b], tgt, P), "candidate %d" % b)
            finally:
                fresh2.close()
        got_i, got_d = h.associate(xyzi(one), xyzi(tgt), Tm, 3.0)
        assert np.array_equal(got_i, want_i) and got_d.tobytes() == want_d.tobytes()
        assert len(h.trace()) == 1 and h.trace()[-1]["sums"].tobytes() == want_sums
        for b in range(len(srcs)):                                    # ... nor by the association
            assert trace_bits(h.traceBatch(b)) == batch[b][8], b
        assert len(first[8]) >= 2 and all(len(g[8]) >= 2 for g in batch)   # of the test's own inputs: every alignment associated at least twice
    finally:
        h.close(); fresh.close()


def test_times_keep_their_meaning():
    """lastMs: set-up, iterations, fitness pass, whole call of the last align; batchLastMs: set-up, iterations with the fitness passes, 0, whole call. The 1 %
    is slack for the float rounding of the event times, not a performance bound."""
    rng = np.random.default_rng(79)
    tgt = rng.uniform(-5, 5, (900, 3)).astype(f32)
    src = rng.uniform(-5, 5, (300, 3)).astype(f32)
    P = loop_icp_params(3.0, max_iterations=5)
    h = LoopIcp()
    try:
        r = h.align(xyzi(src), xyzi(tgt), P)
        ms = h.lastMs().astype(np.float64)
        print("single", r["iterations"], "iterations, ms", ms)
        assert ms.shape == (4,) and np.all(np.isfinite(ms)) and np.all(ms > 0)
        assert ms[0] + ms[1] + ms[2] <= ms[3] * 1.01
        h.align(xyzi(src[:0]), xyzi(tgt), P)
        assert np.array_equal(h.lastMs(), np.zeros(4, f32))
        h.alignBatch([xyzi(src), xyzi(src[:100])], xyzi(tgt), P)
        bms = h.batchLastMs().astype(np.float64)
        print("batch ms", bms)
        assert np.all(np.isfinite(bms)) and bms[2] == 0 and bms[0] > 0 and bms[1] > 0 and bms[3] > 0
        assert bms[0] + bms[1] <= bms[3] * 1.01
        assert np.array_equal(h.lastMs(), np.zeros(4, f32))   # the batch call left the single form's times alone
    finally:
        h.close()
