#!/usr/bin/env python3
"""Measure the wideband blanker's default threshold (include/ext/mercury_wideband_blanker.h, profiles/wideband_blanker.md): over 2^22
samples of white Gaussian CF64 noise per D in {1, 4, 64}, at the default block of each, the highest p / med_b with med_b the level the
host twin reports; the greatest of them times 1.5, rounded up. Also the same at B = 64, which the default block never is. No GPU."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mercury_amd import host_wblank_process, wblank_block  # noqa: E402

SEEDS = {1: 20260001, 4: 20260004, 64: 20260064}


def noise(seed, n):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def highest(x, D, block=0):
    """the highest p / med_b over the blocks the twin reports (all but the last, which waits for its successor)"""
    B = wblank_block(D, block)
    _, reports = host_wblank_process(x, D, block=block, threshold=1e300)
    level = reports["level"][1:]
    p = (x.real * x.real + x.imag * x.imag).reshape(-1, B)[: level.size]
    return float((p.max(axis=1) / level).max())


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--log2n", type=int, default=22)
    args = ap.parse_args()
    rows = []
    for D, seed in SEEDS.items():
        x = noise(seed, 1 << args.log2n)
        rows.append({"D": D, "seed": seed, "block": wblank_block(D), "highest": highest(x, D), "highest_at_64": highest(x, D, 64)})
        print(json.dumps(rows[-1]))
    top = max(r["highest"] for r in rows)
    print(json.dumps({"greatest": top, "times_1.5": 1.5 * top, "default_threshold": math.ceil(1.5 * top),
                      "greatest_at_64": max(r["highest_at_64"] for r in rows)}))


if __name__ == "__main__":
    main()
