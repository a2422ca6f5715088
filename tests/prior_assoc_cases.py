"""The ground-prior association's scene, shared by tests/test_prior_assoc.py (CPU: the twin alone gives the intended verdicts) and tests/test_gpu_prior_assoc.py
(device): a bumpy ground from tests/prior_cases.py (its `curve` ground with seeded ripples on top, so that no direction is left for the ICP to slide along), twelve
key poses, and five history entries — one outside the radius, one from other terrain, one with a planted roll, two good ones."""
import functools

import numpy as np

import icp_twin as T
import prior_cases as pc
from rolo_amd import synth

f32 = np.float32
PATCH = 2.0            # groundPatchSize
DENSITY = 200.0        # points / m^2: about 800 in the target patch, 400 in a source
SOURCE_NOISE = 0.003   # m, on every source coordinate: the good entries' fitness is about 3 x 0.003^2, above the 1e-6 floor of the noise score
WEIGHT = 0.05          # priorFactorWeight of the tests: the factor's roll / pitch / z variances come out near the odometry's 1e-6, so an optimise visibly moves the pose


def bumpy(seed):
    """prior_cases' curved ground over [-6, 6]^2 with three seeded ripples (amplitude 0.08 .. 0.15 m, wavelength 0.9 .. 2 m)"""
    g = pc.ground("curve", seed=seed, n=int(DENSITY * (2 * pc.HALF) ** 2))
    rng = np.random.default_rng(1000 + seed)
    x, y = g[:, 0].astype(np.float64), g[:, 1].astype(np.float64)
    z = g[:, 2].astype(np.float64)
    for _ in range(3):
        amp, lam, th, ph = rng.uniform(0.08, 0.15), rng.uniform(0.9, 2.0), rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
        z = z + amp * np.sin(2 * np.pi * (np.cos(th) * x + np.sin(th) * y) / lam + ph)
    g[:, 2] = z.astype(f32)
    g[:, 3] = 0
    return g


def cut(cloud, size=PATCH):
    h = 0.5 * size
    return cloud[(np.abs(cloud[:, 0]) <= h) & (np.abs(cloud[:, 1]) <= h)]


def motion(rpy, t):
    M = np.eye(4); M[:3, :3] = synth.rpy_to_R(*rpy); M[:3, 3] = t
    return M


def source_of(patch, M, seed):
    """every second point of `patch` with noise, moved by M^-1: the ICP's answer is about M"""
    rng = np.random.default_rng(seed)
    p = patch[::2, :3].astype(np.float64) + rng.normal(0, SOURCE_NOISE, (len(patch[::2]), 3))
    out = np.zeros((len(p), 4), f32)
    out[:, :3] = ((p - M[:3, 3]) @ M[:3, :3]).astype(f32)
    return out


def key_pose(k):
    """roll, pitch, yaw, x, y, z of key k: a gentle left turn, 0.4 m per key"""
    return np.array([0.002 * k, -0.001 * k, 0.01 * k, 0.4 * k, 0.02 * k, 0.01 * k], f32)


N_KEYS = 12
KEY_TIMES = [0.5 * k for k in range(N_KEYS)]
ENTRY_NAMES = ("outside", "other_terrain", "rolled", "good", "good_after")
# entry -> (latest key when it arrives, prior pose relative to that key: roll pitch yaw x y z, the motion its patch carries)
ENTRIES = {
    "outside": (10, (0.0, 0.0, 0.0, 5.0, 0.5, 0.0), motion((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))),
    "other_terrain": (10, (0.001, 0.002, 0.0, 0.3, 0.0, 0.0), motion((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))),
    "rolled": (10, (0.002, -0.001, 0.01, 0.35, 0.05, 0.01), motion((0.2, 0.01, 0.02), (0.03, -0.02, 0.02))),   # 0.2 rad: past any tolerance of a few degrees
    "good": (10, (0.004, -0.003, 0.005, 0.05, -0.02, 0.01), motion((0.012, -0.02, 0.03), (0.05, -0.04, 0.03))),
    "good_after": (11, (0.003, -0.002, 0.004, 0.04, -0.01, 0.0), motion((0.01, -0.015, 0.02), (0.04, -0.03, 0.02))),
}


@functools.lru_cache(maxsize=None)
def scene():
    """(target patch, {entry: source patch}): the target is the ground around the current key pose, in its frame"""
    target = cut(bumpy(3))
    other = cut(bumpy(8))
    sources = {}
    for k, name in enumerate(ENTRY_NAMES):
        base = other if name == "other_terrain" else target
        sources[name] = source_of(base, ENTRIES[name][2], 50 + k)
    return target, sources


@functools.lru_cache(maxsize=None)
def twin_results():
    """{entry: icp_twin.icp(source, target) under the closer's settings}, computed once"""
    target, sources = scene()
    return {name: T.icp(sources[name], target, max_correspondence_distance=PATCH, max_iterations=100, transformation_epsilon=1e-6, euclidean_fitness_epsilon=1e-6)
            for name in ENTRY_NAMES if name != "outside"}


class Keys:
    """what GroundPriorCloser needs of a key map, on the host"""
    def __init__(self, n=0):
        self.poses, self.times = [], []
        for k in range(n):
            self.add(k)

    def add(self, k):
        self.poses.append(key_pose(k)); self.times.append(KEY_TIMES[k])


def feed(closer, keys_add):
    """the twelve key poses arrive one by one (keys_add(k) stores key k); each entry arrives with the key it names. Returns the handler's answers"""
    target, sources = scene()
    told = []
    for k in range(N_KEYS):
        keys_add(k)
        for name in ENTRY_NAMES:
            if ENTRIES[name][0] == k:
                told.append(closer.priorInfoHandler(KEY_TIMES[k] + 0.001, ENTRIES[name][1], sources[name]))
    closer.setGroundCloud(target)
    return told
