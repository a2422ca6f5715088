"""CPU: the constructions of tests/voxel_cases.py pinned through the oracle and the probe simulation — every planted point lands in its voxel, the chain really crosses the
table's end, the key-range clouds touch exactly 2^20 - 1 and -2^20, and the oracle's own map of every case equals the exact reference: keys and counts, means bit for bit
(float32 addends sum exactly in its serial fp64 sum at these counts), covariances within m * 2^-53 * max|c| (m the voxel's count: one rounding per addend of a serial sum)."""
import numpy as np
import pytest

from oracle import pyorc
import voxel_cases as V


def oracle_map(tgt, voxel_type=pyorc.VOXEL_UNIFORM, leaf=1.0, polar=V.POLAR_RES):
    o = pyorc.Reg(pyorc.default_params(voxel_type=voxel_type, voxel_resolution=leaf, polar_resolution=polar))
    o.set_target(tgt); o.set_source(tgt)
    assert o.compute_covariances() == 0 and o.build_voxelmap() == 0
    return o


def check_oracle_against_exact(tgt, voxel_type=pyorc.VOXEL_UNIFORM, leaf=1.0):
    o = oracle_map(tgt, voxel_type, leaf)
    keys = pyorc.voxel_keys(tgt, voxel_type, leaf, V.POLAR_RES)
    cov = o.target_covs()
    ek, ec, em, ev = V.exact_map(tgt, keys, cov)
    k, c, m, v = V.sort_map(*o.voxels())
    assert np.array_equal(k, ek) and np.array_equal(c, ec)
    assert np.array_equal(m, em)
    bound = ec[:, None, None] * 2.0 ** -53 * np.abs(cov[:, :3, :3]).max()
    assert np.all(np.abs(v - ev) <= bound)
    return ek, ec


def test_the_restated_table():
    k = np.array([[0, 0, 0], [V.KEY_MAX, V.KEY_MIN, 5], [-1, 2, -3]])
    assert np.array_equal(V.unpack(V.pack(k)), k)
    assert int(V.pack([V.KEY_MIN] * 3)) == 0 and int(V.pack([V.KEY_MAX] * 3)) == (1 << 63) - 1
    with pytest.raises(AssertionError):
        V.pack([1 << 20, 0, 0])
    with pytest.raises(AssertionError):
        V.pack([0, -(1 << 20) - 1, 0])
    # splitmix64's finaliser on known words (Vigna's reference: mix(0) = 0; the first output of a splitmix64 stream seeded 0 is the finaliser of the golden-ratio increment)
    assert int(V.hash_key(np.uint64(0))) == 0
    assert int(V.hash_key(np.uint64(0x9e3779b97f4a7c15))) == 0xe220a8397b1dcdaf & 0xffffffff
    assert [V.mask_of(n) for n in (1, 510, 512, 513, 1024, 1025)] == [1023, 1023, 1023, 2047, 2047, 4095]
    # the set of taken slots does not depend on the order of the inserts
    rng = np.random.default_rng(1)
    keys = rng.integers(-5, 5, size=(600, 3))
    assert set(V.occupied(keys, 1023)) == set(V.occupied(keys[::-1], 1023)) == set(V.occupied(keys[rng.permutation(600)], 1023))


@pytest.mark.parametrize("polar", [False, True])
def test_the_chain_wraps(polar):
    sc = V.polar_chain_scene() if polar else V.chain_scene()
    ch = sc["chain"]
    assert ch.mask == V.mask_of(sc["tgt"].shape[0]) == 1023 and sc["tgt"].shape[0] == V.CHAIN_N
    table = V.occupied(sc["voxels"], ch.mask)
    assert {1021, 1022, 1023, 0, 1, 2, 3, 4, 5, 6, 7, 8} <= set(table) and 9 not in table and 1020 not in table
    assert len(table) == 17
    # every chain voxel is at home in the last three slots, nine of them found only past the wrap; the ghosts miss at slot 9, three of them after crossing the end
    assert set(int(h) for h in V.home(ch.voxels, ch.mask)) == {1021, 1022, 1023}
    walks = [V.probe_length(k, table, ch.mask) for k in ch.voxels]
    assert all(hit for _, _, hit in walks) and sum(w for _, w, _ in walks) >= 9 and max(n for n, _, _ in walks) >= 10
    gw = [V.probe_length(g, table, ch.mask) for g in ch.ghosts]
    assert not any(hit for _, _, hit in gw) and sum(w for _, w, _ in gw) >= 3 and max(n for n, _, _ in gw) == 13
    # the planted points are where they were meant to be, ghosts included, and no ghost shares a voxel with the map
    vt = pyorc.VOXEL_POLAR if polar else pyorc.VOXEL_UNIFORM
    kt = pyorc.voxel_keys(sc["tgt"], vt, 1.0, V.POLAR_RES)
    assert np.array_equal(kt, np.repeat(sc["voxels"], 30, axis=0))
    kg = pyorc.voxel_keys(sc["ghost_pts"], vt, 1.0, V.POLAR_RES)
    assert np.array_equal(kg, ch.ghosts) and not (set(map(tuple, kg)) & set(map(tuple, kt)))
    check_oracle_against_exact(sc["tgt"], vt, 1.0)


@pytest.mark.parametrize("shift", [-1000, -60000])
def test_shifted_chain_scenes(shift):
    sc = V.chain_scene(shift)
    assert np.all(sc["tgt"][:, :3] < 0) and V.is_exact(sc["tgt"])
    check_oracle_against_exact(sc["tgt"])


def test_key_range_scene():
    sc = V.key_range_scene()
    tgt = sc["tgt"]
    k = pyorc.voxel_keys(tgt, pyorc.VOXEL_UNIFORM, sc["leaf"])
    assert np.array_equal(k, V.range_keys(tgt))
    assert k[:, 0].max() == V.KEY_MAX == 2 ** 20 - 1 and k[:, 0].min() == V.KEY_MIN == -2 ** 20
    assert k[sc["idx_hi"], 0] == V.KEY_MAX and k[sc["idx_lo"], 0] == V.KEY_MIN
    for x, want in zip(sc["first_out"], (2 ** 20, -2 ** 20 - 1)):
        assert float(np.float32(x)) == x
        p = np.array([[x, 0.0, 0.0, 0.0]], np.float32)
        assert V.range_keys(p)[0, 0] == want
        inner = np.nextafter(np.float32(x), np.float32(0.0))
        assert V.range_keys(np.array([[inner, 0, 0, 0]], np.float32))[0, 0] == (V.KEY_MAX if x > 0 else V.KEY_MIN)   # ... and it is the FIRST float outside
    assert V.is_exact(tgt)
    check_oracle_against_exact(tgt, leaf=sc["leaf"])


@pytest.mark.parametrize("n", [255, 256, 257, 511, 512])
def test_one_voxel_clouds_sit_just_under_the_headroom(n):
    p = V.one_voxel_cloud(n)
    assert V.is_exact(p)
    h = V.headroom(p)
    # n * max * scale < 2^62 by the contract; at n = 2^k - 1 the cloud uses all but 1 / 2^k of it, at 2^k half
    assert h < 1.0
    assert h > {255: 0.99, 256: 0.49, 257: 0.5, 511: 0.99, 512: 0.49}[n]
    ek, ec = check_oracle_against_exact(p, leaf=64.0)
    assert len(ek) == 1 and ec[0] == n


def test_tiny_far_and_sub_half_clouds():
    p = V.tiny_and_far_cloud()
    assert p.shape[0] == 512 and not V.is_exact(p)
    assert V.quantum_pos(512, V.maxabs(p)) == 2.0 ** -42
    ek, ec = check_oracle_against_exact(p)
    assert len(ek) == 2 and tuple(ek[0]) == (-1, -1, -1)
    q = V.sub_half_cloud()
    assert V.quantum_pos(q.shape[0], V.maxabs(q)) == 2.0 ** -(62 - 9)   # max(e, -1): the scale stops growing below 0.5
    check_oracle_against_exact(q, leaf=0.125)


def test_quanta():
    assert V.quantum_pos(510, 24.3) == 2.0 ** -(62 - 9 - 5) and V.quantum_pos(512, 1023.9) == 2.0 ** -42 and V.quantum_pos(512, 1024.0) == 2.0 ** -41
    assert V.quantum_pos(100, 0.6) == V.quantum_pos(100, 0.3) == V.quantum_pos(100, 0.0) == 2.0 ** -(62 - 7)
    assert V.quantum_cov(510) == 2.0 ** -52 and V.quantum_cov(512) == 2.0 ** -51
    assert np.array_equal(V.lowest_bit(np.array([0.0, 1.0, 0.75, -6.0, 2.0 ** -40 * 3])), [0.0, 1.0, 0.25, 2.0, 2.0 ** -40])


@pytest.mark.parametrize("distinct,groups,interleave", [(127, 1, False), (128, 1, False), (129, 1, False), (256, 1, False), (2, 1, True), (129, 4, False)])
def test_lds_table_clouds(distinct, groups, interleave):
    cloud, leaf = V.lds_cloud(distinct, interleave=interleave, groups=groups)
    assert cloud.shape[0] == 256 * groups
    k = pyorc.voxel_keys(cloud, pyorc.VOXEL_UNIFORM, leaf)
    if interleave:
        assert np.array_equal(k[0::2], np.repeat(k[:1], 128, axis=0)) and np.array_equal(k[1::2], np.repeat(k[1:2], 128, axis=0)) and not np.array_equal(k[0], k[1])
    else:   # a voxel's points are adjacent: every key is one run
        change = np.any(k[1:] != k[:-1], axis=1)
        assert int(change.sum()) + 1 == distinct * groups
    check_oracle_against_exact(cloud, leaf=leaf)


@pytest.mark.parametrize("neighbor", [pyorc.DIRECT1, pyorc.DIRECT7])
def test_oracle_registers_the_chain_scene(neighbor):
    """the registration scene of the lookup tests is a well-posed problem: the oracle converges in a few iterations on most of the 510 points"""
    sc = V.chain_scene()
    src = V.rotated_source(sc["tgt"])
    o = pyorc.Reg(pyorc.default_params(voxel_type=pyorc.VOXEL_UNIFORM, voxel_resolution=1.0, neighbor_search=neighbor))
    o.set_target(sc["tgt"]); o.set_source(src)
    _, H, _ = o.so3_linearize(np.eye(4))
    n_corr = len(np.unique(o.correspondences()[0]))
    print("cond(H) = %.2f, %d of %d source points with a correspondence" % (np.linalg.cond(H), n_corr, src.shape[0]))
    assert np.linalg.cond(H) < 10 and 350 <= n_corr <= 510
    rc, _, Td, it, conv = o.align()
    assert rc == 0 and conv and 1 <= it <= 5
    R = V.rpy_deg_to_R(*V.ROT_DEG)
    assert np.abs(Td[:3, :3] @ R - np.eye(3)).max() < 2e-3   # the rotation is undone (to what the points that changed voxel allow)
