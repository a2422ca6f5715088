"""Writes tests/golden/cov_cases.npz: the constructed cluster clouds of tests/cov_cases.py (two clouds per k = 20, 7, 33, 100, source and target), owner and class per
point, one block of expected matrices per distinct exact covariance (fractions + mpmath at 60 digits, the six rules as functions of the exact matrix) and the bars: per
rule the oracle's largest deviation from the exact matrix over the W and T2 clusters of all k, relative to the largest |entry|.

CPU only; needs mpmath and the built oracle. tests/test_cov_cases.py rebuilds every array and compares the bytes. Run from the repository root:
    python tests/golden/make_golden_cov_cases.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))


def main():
    import cov_cases as cc
    d = cc.build_fixture()
    np.savez_compressed(cc.GOLDEN, **d)
    print("wrote", cc.GOLDEN, os.path.getsize(cc.GOLDEN), "bytes;", d["block_exp"].shape[0], "expected blocks")
    for r, v in zip(cc.RULES, d["oracle_dev"]):
        print("oracle deviation %-20s %.3e" % (r, v))


if __name__ == "__main__":
    main()
