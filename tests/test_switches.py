"""CPU: the table of switches the library reads from the environment (rolo_amd/csrc/switches.hpp) gives, for every switch, what the hand-written parse it replaced
gave: the default with a clean environment, an accepted value as given, a rejected value clamped as before. The expected values below were taken from those parses
(`static const ... = [] { getenv ... }()` in api.hip, passes.hip, knn_cov.hip, scan2map.hip and odometry.hip), not from the header."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFAULTS = {
    "ROLO_VOXEL_FUSE": "1", "ROLO_KNN_MOMENTS": "1", "ROLO_KNN_SUB": "-1", "ROLO_POLAR_EXACT": "1",
    "ROLO_LM_FUSED": "-1", "ROLO_LM_THREADS": "512", "ROLO_LM_PPT": "1", "ROLO_LM_SPEC_LIN": "1", "ROLO_PASS_NRM": "1", "ROLO_PASS_XCD": "1", "ROLO_STAMP": "0",
    "ROLO_LM_PERSIST_WGS": "0", "ROLO_LM_PERSIST_BUSY_THREADS": "512", "ROLO_LM_PERSIST_ADMIT_US": "1000", "ROLO_LM_PERSIST_TIMEOUT_MS": "200",
    "ROLO_LM_PERSIST_INTERLEAVE": "1", "ROLO_LM_PERSIST_MCACHE": "1", "ROLO_LM_PERSIST_BATCH": "2", "ROLO_CTRL_GENERIC": "0",
    "ROLO_CU_PARTITION": "0", "ROLO_ODOM_FRONT_PRIORITY": "1",
    "ROLO_S2M_PACKETS": "1", "ROLO_S2M_STATS": "-",
    "ROLO_PEER_TIMEOUT_MS": "10000", "ROLO_PEER_MEM": "-", "ROLO_ODOM_EARLY_SOURCE": "0/1",   # (the last: unset leaves the caller's default, whichever it is)
}
# switch -> (value set, value read): one accepted non-default value each
ACCEPTED = {
    "ROLO_VOXEL_FUSE": ("0", "0"), "ROLO_KNN_MOMENTS": ("0", "0"), "ROLO_KNN_SUB": ("2", "2"), "ROLO_POLAR_EXACT": ("0", "0"),
    "ROLO_LM_FUSED": ("1", "1"), "ROLO_LM_THREADS": ("1024", "1024"), "ROLO_LM_PPT": ("16", "16"), "ROLO_LM_SPEC_LIN": ("0", "0"), "ROLO_PASS_NRM": ("0", "0"),
    "ROLO_PASS_XCD": ("0", "0"), "ROLO_STAMP": ("1", "1"),
    "ROLO_LM_PERSIST_WGS": ("64", "64"), "ROLO_LM_PERSIST_BUSY_THREADS": ("256", "256"), "ROLO_LM_PERSIST_ADMIT_US": ("0", "0"), "ROLO_LM_PERSIST_TIMEOUT_MS": ("50", "50"),
    "ROLO_LM_PERSIST_INTERLEAVE": ("0", "0"), "ROLO_LM_PERSIST_MCACHE": ("0", "0"), "ROLO_LM_PERSIST_BATCH": ("4", "4"), "ROLO_CTRL_GENERIC": ("1", "1"),
    "ROLO_CU_PARTITION": ("4", "4"), "ROLO_ODOM_FRONT_PRIORITY": ("0", "0"),
    "ROLO_S2M_PACKETS": ("0", "0"), "ROLO_S2M_STATS": ("/tmp/walk.csv", "/tmp/walk.csv"),
    "ROLO_PEER_TIMEOUT_MS": ("250.5", "250.5"), "ROLO_PEER_MEM": ("coarse", "coarse"), "ROLO_ODOM_EARLY_SOURCE": ("1", "1/1"),
}
# values outside what a switch accepts, in two rounds (two of the switches have a rejected value on either side)
REJECTED = [
    {"ROLO_LM_THREADS": ("768", "512"), "ROLO_LM_PPT": ("0", "1"),
     "ROLO_LM_PERSIST_BATCH": ("3", "2"), "ROLO_LM_PERSIST_BUSY_THREADS": ("128", "512"), "ROLO_CU_PARTITION": ("3", "0"), "ROLO_LM_PERSIST_ADMIT_US": ("-5", "1000"),
     "ROLO_LM_PERSIST_TIMEOUT_MS": ("0", "200"), "ROLO_LM_PERSIST_WGS": ("7", "0"), "ROLO_KNN_SUB": ("3", "-1"), "ROLO_ODOM_EARLY_SOURCE": ("0", "0/0")},
    {"ROLO_LM_PPT": ("17", "1"), "ROLO_LM_PERSIST_WGS": ("257", "0"), "ROLO_LM_PERSIST_TIMEOUT_MS": ("-3", "200"), "ROLO_LM_FUSED": ("-4", "-4")},
]


def _table(exe, env):
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(line.split(" ", 1) for line in r.stdout.splitlines())


def test_switch_table(tmp_path):
    exe = str(tmp_path / "switches_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rolo_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "switches_test.cpp"), "-o", exe], check=True)
    assert sorted(ACCEPTED) == sorted(DEFAULTS)
    assert _table(exe, {}) == DEFAULTS
    assert _table(exe, {k: v[0] for k, v in ACCEPTED.items()}) == {k: v[1] for k, v in ACCEPTED.items()}
    for round_ in REJECTED:
        assert _table(exe, {k: v[0] for k, v in round_.items()}) == {**DEFAULTS, **{k: v[1] for k, v in round_.items()}}
