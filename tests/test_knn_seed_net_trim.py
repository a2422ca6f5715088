"""CPU: the trimmed seed networks of the neighbour search (rolo_amd/csrc/knn_seed_net.hpp) with integer min / max in place of the device's v_min_f64 / v_max_f64:
merge_chunk without a sort of the tail on every pair of ascending 0-1 lists (21 x 9, 21 x 5), first_two_chunks (the first seed leaf, into a list of sentinels) on every
pair of ascending 0-1 chunks and against merge_chunk applied twice, random lists of distinct keys with +inf padding and lists with ties against std::sort + truncate,
and the number of min / max calls of each form: 88 for a chunk of 8, 76 for a chunk of 4, 64 for the first leaf's merge (tests/cpp/seed_net_trim_test.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_trimmed_seed_networks(tmp_path):
    exe = str(tmp_path / "seed_net_trim_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rolo_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "seed_net_trim_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all held" in r.stdout, r.stdout + r.stderr
    assert "merge_chunk<8> 0-1 pairs: 189" in r.stdout and "merge_chunk<4> 0-1 pairs: 105" in r.stdout and "first_two_chunks 0-1 pairs: 81" in r.stdout, r.stdout
    assert "merge_chunk<8> min/max calls: 88" in r.stdout and "merge_chunk<4> min/max calls: 76" in r.stdout and "first_two_chunks min/max calls: 64" in r.stdout, r.stdout
