"""CPU: the constructed rings of tests/front_rings.py. For every case the C++ oracle and the independent numpy twin agree bit for bit on all five outputs of the feature
stage, the hand-written `expect_paths` agree with a restatement of the kernel's eligibility rule, and the case reaches what its purpose says — so that the GPU module
(tests/test_gpu_front_rings.py) compares the kernel with an answer that two statements share, on inputs that are known to sit where they claim to."""
import functools

import numpy as np
import pytest

import front_rings as R
from oracle import pyorc, twin_front

F = np.float32
OUTPUTS = ("curvature", "picked", "label", "corner", "surface")
NAMES = list(R.CASES)


@functools.lru_cache(maxsize=None)
def oracle(name):
    c = R.CASES[name]
    return pyorc.extract_features(pyorc.front_params(**R.params(c)), c["proj"])


def twin(c, edge=None, surf=None):
    return twin_front.extract_features(c["proj"], c["n_scan"], F(c["edge_threshold"] if edge is None else edge), F(c["surf_threshold"] if surf is None else surf),
                                       F(c["odometry_surf_leaf_size"]))


def ring_sectors(c, r):
    return [(sp, ep) for sp, ep in R.sectors(int(c["proj"]["start_ring"][r]), int(c["proj"]["end_ring"][r])) if sp < ep]


def scan_lengths(c, label):
    """points of every ring's surface scan: the cells of its non-empty sectors that are not corners"""
    return [sum(int((label[sp:ep + 1] <= 0).sum()) for sp, ep in ring_sectors(c, r)) for r in range(c["n_scan"])]


def corner_candidates(c, r):
    """per non-empty sector of ring r: cells the occlusion / parallel-beam marks left free whose curvature is above the edge threshold, by the twin's count"""
    marks = twin(c, edge=np.inf, surf=-np.inf)   # nothing is picked: `picked` is markOccludedPoints alone
    assert not marks["label"].any()
    free = (marks["picked"] == 0) & (marks["curvature"] > F(c["edge_threshold"]))
    return [int(free[sp:ep + 1].sum()) for sp, ep in ring_sectors(c, r)]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_and_twin_agree_bit_for_bit(name):
    c = R.CASES[name]
    eo, et = oracle(name), twin(c)
    for k in OUTPUTS:
        assert eo[k].shape == et[k].shape, k
        assert np.array_equal(eo[k], et[k]), k
    assert np.isfinite(eo["curvature"]).all()


def test_the_table_keeps_its_shapes_small():
    for c in R.CASES.values():
        H = c["horizon_scan"]
        assert c["n_scan"] <= 16 and H in (1024, 2048, 4096) and c["purpose"]
        assert H < 4096 or c["n_scan"] <= 4
        assert H != 2048 or max(c["pops"]) > 1024 or c["name"] == "steps_fast"   # (215 random column steps need the room)
        assert set(c["expect_paths"]) <= set(range(c["n_scan"])) and c["expect_paths"]
        p = c["proj"]
        assert np.array_equal(p["start_ring"] - 4, np.cumsum(c["pops"]) - c["pops"]) and np.array_equal(p["end_ring"] + 6, np.cumsum(c["pops"]))


def rule(c, r):
    """(attempted, word of a ring that goes stage by stage): the eligibility rule of extract_kernel, restated from the kernel and not from front_rings.py"""
    s, e = int(c["proj"]["start_ring"][r]), int(c["proj"]["end_ring"][r])
    edge, surf = F(c["edge_threshold"]), F(c["surf_threshold"])
    sec = R.sectors(s, e)
    seg = 2
    while seg < max(ep - sp for sp, ep in sec):
        seg *= 2
    attempted = bool(surf > 0 and edge >= surf and seg >= 64 and e - s >= 12 and all(ep > sp for sp, ep in sec))
    assert max(ep - sp for sp, ep in sec) < (c["horizon_scan"] > 2048 and 1024 or 512)   # SEGMAX is never the reason
    assert sec[5][1] < c["proj"]["n"] - 5                                                   # nor the tail rule
    if s < 5 and attempted:
        assert sec[0][1] >= 5
    word = 0
    for j, (sp, ep) in enumerate(sec):
        serial = sp < 5 and not (surf > 0 and edge >= 0)
        word |= (R.SEC_EMPTY if sp >= ep else R.SEC_SERIAL if serial else R.SEC_PARALLEL) << (2 + 2 * j)
    return attempted, word


@pytest.mark.parametrize("name", NAMES)
def test_expected_paths_follow_the_eligibility_rule(name):
    c = R.CASES[name]
    label = oracle(name)["label"]
    for r, want in c["expect_paths"].items():
        attempted, staged = rule(c, r)
        corners = [int((label[sp:ep + 1] == 1).sum()) for sp, ep in ring_sectors(c, r)]
        if not attempted:
            assert want == (R.RING_NONE | staged), (r, want)
        elif R.ring_level(want) == R.RING_APPLIED:
            assert want == R.APPLIED and max(corners) <= 20
            assert max(corners) < 20 or max(corner_candidates(c, r)) == 20   # 20 labelled: all there were, not the first 20 of more
        else:
            assert want == (R.RING_CAPPED | staged), (r, want)
            cand = corner_candidates(c, r)
            assert max(cand) >= 21 and any(k == 20 and m >= 21 for k, m in zip(corners, cand)), (r, corners, cand)


def test_paths_cover_every_value():
    lds = [w for c in R.CASES.values() if c["horizon_scan"] <= 2048 for w in c["expect_paths"].values()]
    big = [w for c in R.CASES.values() if c["horizon_scan"] > 2048 for w in c["expect_paths"].values()]
    assert {R.ring_level(w) for w in lds} == {R.RING_NONE, R.RING_CAPPED, R.RING_APPLIED}
    assert {R.ring_level(w) for w in big} == {R.RING_NONE, R.RING_CAPPED, R.RING_APPLIED}
    assert {R.sector_level(w, 0) for w in lds} == {R.SEC_NOT_STAGED, R.SEC_EMPTY, R.SEC_PARALLEL, R.SEC_SERIAL}
    later = {R.sector_level(w, j) for w in lds for j in range(1, 6)}
    # the serial walk cannot be reached in a later sector through validated arrays (front_rings.py, module docstring)
    assert later == {R.SEC_NOT_STAGED, R.SEC_EMPTY, R.SEC_PARALLEL}
    assert R.SEC_SERIAL in {R.sector_level(w, 0) for w in big}


# ---- each case reaches what it is there for ------------------------------------------------------------------------------------
def test_populations():
    c = R.CASES["pops_small"]
    assert c["pops"][1:12] == [0, 1, 11, 12, 13, 17, 18, 19, 20, 21, 22] and c["pops"][12:14] == [208, 209]
    longest = lambda r: max(ep - sp for sp, ep in R.sectors(int(c["proj"]["start_ring"][r]), int(c["proj"]["end_ring"][r])))   # noqa: E731
    assert (longest(12), longest(13)) == (32, 33)
    assert [len(ring_sectors(c, r)) for r in range(1, 12)] == [0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 6]
    h = R.CASES["head_small"]
    assert h["proj"]["start_ring"][2] == 4 and R.sectors(4, int(h["proj"]["end_ring"][2]))[0] == (4, 4)   # ep_0 = 4 < 5
    assert [R.CASES[k]["proj"]["n"] for k in ("cloud_n3", "cloud_n10", "cloud_n11", "cloud_n12")] == [3, 10, 11, 12]
    assert [int((oracle(k)["curvature"] != 0).sum()) for k in ("cloud_n3", "cloud_n10", "cloud_n11", "cloud_n12")] == [0, 0, 1, 2]
    assert R.CASES["full_1024"]["pops"] == [1023, 1024, 1024] and R.CASES["full_2048"]["pops"] == [2047, 2048] and R.CASES["big_noise"]["pops"] == [4096, 4095]
    sec = R.sectors(4, 4096 - 6)
    assert max(ep - sp for sp, ep in sec) > 512   # only the scratch form holds such a sector


def test_constant_range_ties_every_key():
    for name in ("const", "const_16", "big_const"):
        c, eo = R.CASES[name], oracle(name)
        assert not eo["curvature"].any() and not np.signbit(eo["curvature"]).any() and eo["corner"].shape[0] == 0
        picks = np.nonzero(eo["label"][:c["pops"][0]] == -1)[0]
        # ties fall back on the index, and the head ring's stale {0, 0} entry leads: point 0, then every sixth cell through all six sectors
        assert picks[0] == 0 and np.all(np.diff(picks) == 6) and picks[-1] >= c["pops"][0] - 7 - 5


def test_ramps_order_rank_against_position():
    up, down = oracle("ramp_up")["curvature"], oracle("ramp_down")["curvature"]
    short = slice(1024 + 5, 1424 - 5)      # the ring of 400: exact order
    assert np.all(np.diff(up[short][5:]) > 0) and np.all(np.diff(down[short][:-5]) < 0)
    long_ = np.arange(105, 1000)            # the ring of 1024: the order up to rounding
    for cv, sign in ((up, 1), (down, -1)):
        rank = np.argsort(np.argsort(cv[long_], kind="stable"))
        assert sign * np.corrcoef(rank, long_)[0, 1] > 0.999
    for name in ("ramp_up_cap", "ramp_down_cap"):
        assert oracle(name)["corner"].shape[0] > 60


def test_plateau_sits_exactly_on_the_threshold():
    at, below = oracle("plateau_at"), oracle("plateau_below")
    assert set(np.unique(at["curvature"][40:-40])) == {F(0), F(0.0625), F(6.25)}
    assert F(R.EDGE_BELOW_PLATEAU) < F(0.0625) and np.nextafter(F(R.EDGE_BELOW_PLATEAU), F(1)) == F(0.0625)
    # the counts both CPU statements give on these deterministic arrays (oracle here; the twin is held equal to it case by case above)
    assert at["corner"].shape[0] == 0 and below["corner"].shape[0] == 1414
    assert twin(R.CASES["plateau_below"])["corner"].shape[0] == 1414
    assert np.all(below["curvature"][below["label"] == 1] == F(0.0625))
    assert oracle("plateau_fast_at")["corner"].shape[0] == 0 and oracle("plateau_fast_below")["corner"].shape[0] == 203


def test_cap_cases_strike_the_cap():
    for name, r in (("saw_cap", 0), ("saw_cap", 1), ("saw_21", 1), ("big_cap", 0), ("big_cap", 1), ("ramp_up_cap", 0), ("saw_cap_staged", 0), ("thr_edge_neg", 0), ("thr_edge_neg", 1),
                    ("big_edge_neg", 0)):
        assert max(corner_candidates(R.CASES[name], r)) >= 21, name
    lab = oracle("saw_cap_staged")["label"]
    assert max(int((lab[sp:ep + 1] == 1).sum()) for sp, ep in ring_sectors(R.CASES["saw_cap_staged"], 0)) == 20
    assert corner_candidates(R.CASES["saw_20"], 1)[1] == 20 and oracle("saw_20")["corner"].shape[0] == 20
    assert corner_candidates(R.CASES["saw_21"], 1)[1] == 21 and oracle("saw_21")["corner"].shape[0] == 20


def test_depth_jumps_sit_one_float_either_side_of_the_constant():
    d = {k: float(F(hi - lo)) for k, (lo, hi) in R.JUMPS.items()}
    assert d["jump_1"] < 0.3 < d["jump_half"] < d["jump_4"]
    assert F(d["jump_half"]) == F(0.3) and not d["jump_half"] > float(F(0.3))       # above the double 0.3, not above the float
    for k in R.JUMPS:
        assert oracle(k)["curvature"][304] < 1e-10 and R.CASES[k]["proj"]["start_ring"][1] == 304   # the first candidate of ring 1 is an ordinary surface cell
    marks = {k: oracle(k + "_marks")["picked"] for k in R.JUMPS}
    assert not marks["jump_1"].any()
    for k in ("jump_4", "jump_half"):
        assert np.array_equal(np.nonzero(marks[k])[0], np.arange(299, 305))          # 299 .. 304, across the ring border at 300
    assert not np.array_equal(oracle("jump_1")["picked"], oracle("jump_4")["picked"])
    assert np.array_equal(np.nonzero(oracle("drop_half_marks")["picked"])[0], np.arange(293, 299)) and R.CASES["drop_half"]["proj"]["end_ring"][0] - 1 == 293
    d = oracle("drop_half")   # the surface picks beside the border are 288 and 304, reaching 293 and 299: cells 294 .. 298 are picked by the marks alone
    assert d["label"][288] == -1 and d["label"][304] == -1 and not d["label"][289:304].any() and d["picked"][294:299].all()
    assert not oracle("jump_1")["picked"][294:299].any()
    assert not np.array_equal(oracle("jump_1")["label"], oracle("jump_half")["label"]) and oracle("jump_1")["label"][304] == -1 and oracle("jump_4")["label"][304] == 0


def test_parallel_beam_sits_one_float_either_side():
    assert float(F(R.BEAM_BELOW - F(10))) < 0.02 * 10.0 < float(F(R.BEAM_ABOVE - F(10))) and np.nextafter(R.BEAM_BELOW, F(11)) == R.BEAM_ABOVE
    assert not oracle("beam_below")["picked"].any()
    assert np.array_equal(np.nonzero(oracle("beam_above")["picked"])[0], [150, 300])


def test_thresholds_and_the_stale_head_entry():
    eq, inv, s0, neg, both = (oracle(k) for k in ("thr_equal", "thr_inverted", "thr_surf0", "thr_edge_neg", "thr_both_neg"))
    c = R.CASES["thr_inverted"]
    cv = inv["curvature"]
    assert ((cv > F(c["edge_threshold"])) & (cv < F(c["surf_threshold"]))).sum() > 20       # cells that are both kinds of candidate
    assert not (s0["label"] == -1).any() and (s0["label"] == 1).any()
    assert eq["label"][0] == -1          # sane thresholds: the stale {0, 0} entry makes point 0 the best surface candidate
    assert neg["label"][0] == 1 and both["label"][0] == 1 and neg["curvature"][0] == 0   # edge < 0: it is a corner, although point 0 has no curvature of its own
    assert any(np.array_equal(row, R.CASES["thr_edge_neg"]["proj"]["extracted"][0]) for row in neg["corner"][:20])   # ... the last of sector 0's walk, k = sp
    assert not (both["label"] == -1).any()
    for c0 in (0, 10, 11, 500):
        assert R.CASES["col0_%d" % c0]["proj"]["point_col_ind"][0] == c0 and oracle("col0_%d" % c0)["label"][0] == 1


def test_column_steps_and_borders():
    for name in ("steps_staged", "steps_serial", "steps_fast"):
        p = R.CASES[name]["proj"]
        steps = np.diff(p["point_col_ind"])
        for r in np.cumsum(R.CASES[name]["pops"])[:-1]:
            steps[r - 1] = 1   # (the step over a ring border is not one of the draw)
        assert set(steps) == set(R.STEPS), name
    for name in ("steps_staged", "steps_serial"):   # depth jumps beside steps of 9 (marks) and 10 (none)
        p = R.CASES[name]["proj"]
        jump = np.abs(np.diff(p["point_range"])) > 0.3
        assert (jump & (np.diff(p["point_col_ind"]) == 9)).any() and (jump & (np.diff(p["point_col_ind"]) == 10)).any()
    for name, pop in (("border_sparse", 60), ("border_dense", 250)):
        p = R.CASES[name]["proj"]
        for b in (pop, 2 * pop):
            assert 0 < p["point_col_ind"][b] - p["point_col_ind"][b - 1] < 10 and abs(float(p["point_range"][b] - p["point_range"][b - 1])) > 0.3
            marks = twin(R.CASES[name], edge=np.inf, surf=-np.inf)["picked"]
            assert marks[b - 1] == 1 or marks[b] == 1   # the jump between the last cell of a ring and the first of the next marks one side


def test_voxel_cases():
    total = lambda name: sum(scan_lengths(R.CASES[name], oracle(name)["label"]))   # noqa: E731
    assert scan_lengths(R.CASES["vox_own_cell"], oracle("vox_own_cell")["label"]) == [1024, 1025, 1026]
    assert oracle("vox_own_cell")["surface"].shape[0] == 1024 + 1025 + 1026
    assert scan_lengths(R.CASES["vox_scan_1_2"], oracle("vox_scan_1_2")["label"]) == [2, 1] and oracle("vox_scan_1_2")["surface"].shape[0] == 3
    assert scan_lengths(R.CASES["vox_one_cell"], oracle("vox_one_cell")["label"]) == [2038, 290] and oracle("vox_one_cell")["surface"].shape[0] == 2
    # pass-through: the scan comes back as it went in, and the cell-count product is where PCL's int64 still holds it
    c, eo = R.CASES["vox_pass"], oracle("vox_pass")
    assert eo["surface"].shape[0] == total("vox_pass") == 1014 + 290
    scan0 = c["proj"]["extracted"][4:1018]
    assert np.array_equal(eo["surface"][:1014], scan0)
    inv = F(1.0) / F(c["odometry_surf_leaf_size"])
    span = ((scan0[:, :3].max(0) - scan0[:, :3].min(0)) * inv).astype(np.int64) + 1
    assert 2 ** 31 < int(span[0]) * int(span[1]) * int(span[2]) < 2 ** 63
    lat = R.CASES["vox_lattice"]["proj"]["extracted"]
    assert (lat[:, :3] < 0).any() and np.array_equal(lat[:, 0], np.round(lat[:, 0] / F(0.4)).astype(F) * F(0.4))
    assert 1 < oracle("vox_lattice")["surface"].shape[0] <= 2 * 7 * 5 * 3
    assert total("vox_dense") > 1.2 * oracle("vox_dense")["surface"].shape[0]   # runs of several points
    for name in ("vox_dense", "vox_pass", "const"):
        assert len(np.unique(R.CASES[name]["proj"]["extracted"][:, 3])) > 100    # the intensity column varies
