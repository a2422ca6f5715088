"""CPU: the box tests of the tree walks (rolo_amd/csrc/knn_box_pair.hpp) compiled for the host: box_d2_pair, both child boxes of a node at once, equals the scalar
box_d2 bit for bit on random boxes and queries, degenerate boxes, queries inside, on faces and at corners, and padding boxes; the one-compare reach test with the
clamped bound equals (d <= bd) && (d < INFINITY) over d in {0, denormal, 1, FLT_MAX, +inf} x bd in {-1, 0, 1, FLT_MAX, +inf} (tests/cpp/box_pair_test.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_box_pair_and_clamped_compare(tmp_path):
    exe = str(tmp_path / "box_pair_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rolo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "box_pair_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all held" in r.stdout, r.stdout + r.stderr
    assert "box pairs: 760000" in r.stdout and "clamped compare table: 25" in r.stdout, r.stdout
