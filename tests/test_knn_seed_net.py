"""CPU: the sorting / merging networks that build the neighbour search's seed lists (rolo_amd/csrc/knn_seed_net.hpp) with integer min / max in place of the
device's v_min_f64 / v_max_f64: sort8 and sort4 on every 0-1 input, the chunk merges on every pair of ascending 0-1 lists (21 x 9, 21 x 5), the bitonic cleaner in
both directions, and a few thousand random lists of distinct keys with +inf padding against std::sort + truncate (tests/cpp/seed_net_test.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seed_networks_sort_and_merge(tmp_path):
    exe = str(tmp_path / "seed_net_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rolo_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "seed_net_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all held" in r.stdout, r.stdout + r.stderr
    assert "sort8 0-1 inputs: 256" in r.stdout and "merge8 0-1 pairs: 189" in r.stdout, r.stdout
