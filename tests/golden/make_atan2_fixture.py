#!/usr/bin/env python3
"""Writes tests/golden/atan2_cr.json: (y, x, atan2(y, x) rounded to nearest) as hexadecimal doubles, the expected value from 300-bit
arithmetic (mpmath).  Small rotations (the usual argument of the quaternion tangent), general arguments over y >= 0, wide magnitude ranges,
and arguments on which a math library's atan2 is known to round the other way.  usage: python tests/golden/make_atan2_fixture.py"""
import json
import math
import os

import mpmath as mp
import numpy as np

HARD = [("0x1.5a1913dfe5c8p-3", "0x1.ee8df193434p-1"), ("0x1.9c517b9a8fc4p-2", "0x1.8dbafea94eap-1"), ("0x1.6f010b5d5fdp-3", "-0x1.e87645a5506p-4"),
        ("0x1.66f05547eaec4p-12", "0x1.5766bd968946bp-8"), ("0x1.ac97a7cefc9p-3", "0x1.ddfc1ecae9a8p-2"), ("0x1.e1047cf92dap-5", "0x1.00d2fc92c5dp-1"),
        ("0x1.9d1b39e7f51p-4", "0x1.ab11f62bee2p-1"), ("0x1.e47d8399238cp-10", "0x1.c0d94b0b9b2ap-7")]


def main():
    mp.mp.prec = 300
    rng = np.random.default_rng(0)
    pts = [(rng.uniform(0, 1e-2), rng.uniform(0.9, 1.0)) for _ in range(700)] + [(rng.uniform(0, 1), rng.uniform(-1, 1)) for _ in range(700)]
    pts += [(math.exp(rng.uniform(-40, 5)), math.exp(rng.uniform(-20, 20)) * rng.choice([-1, 1])) for _ in range(600)]
    pts += [(rng.uniform(0, 1e-6), 1.0 - rng.uniform(0, 1e-12)) for _ in range(200)]
    pts += [(float.fromhex(y), float.fromhex(x)) for y, x in HARD]
    rows = []
    for y, x in pts:
        y, x = float(y), float(x)
        rows.append([y.hex(), x.hex(), float(mp.atan2(mp.mpf(y), mp.mpf(x))).hex()])
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "atan2_cr.json")
    with open(out, "w") as f:
        json.dump(dict(precision_bits=300, hard=len(HARD), points=rows), f, separators=(",", ":"))
    print(len(rows), "points ->", out)


if __name__ == "__main__":
    main()
