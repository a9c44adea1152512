#!/usr/bin/env python3
"""Host wall time of one mjpc_hip_inverse_fd call against one mjpc_hip_transition_fd call at the same window length on the A1: the two
derivative fan-outs of the reference (mjd_inverseFD per configuration in mjpc/direct/, mjd_transitionFD per knot in the planners).

usage: tools/time_inverse_fd.py [--model quadruped] [--T 32] [--calls 5] [--passes 2] [--centered] [--only inverse_fd|transition_fd|inverse_batch]
The window is the model's default state with seeded nudges, controls and accelerations (tests/transition_cases.py's rule).  One-sided,
eps = 1e-6, inverse_fd with discrete = 1 (what direct/ sets).  Prints one line per pass and path: median (min - max) in ms, and the
number of evaluations of a call.  With --only one path runs alone, for a profiler run of its own, e.g.
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/time_inverse_fd.py --only inverse_fd
whose kernel statistics hold ifd_assemble_kernel, the inverse kernel and ifd_difference_kernel.  A build that has no inverse calls
(an older revision) times transition_fd alone.  DESIGN section 8l holds the recorded figures."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mujoco_mpc_amd.modelgen import REGISTRY       # noqa: E402
from mujoco_mpc_amd.planner import HipBackend      # noqa: E402


def window(m, d, T, seed=0):
    rng = np.random.default_rng(seed)
    nq, nv, na, nu = m["nq"], m["nv"], m["na"], m["nu"]
    X = np.tile(np.asarray(d["state"], float), (T, 1))
    for j in range(m["njnt"]):                      # plain coordinates only: quaternions stay unit
        if int(m["jnt_type"][j]) >= 2:
            X[1:, int(m["jnt_qposadr"][j])] += 0.01 * rng.standard_normal(T - 1)
    X[1:, nq:nq + nv] += 0.05 * rng.standard_normal((T - 1, nv))
    if na:
        X[1:, nq + nv:] += 0.05 * rng.standard_normal((T - 1, na))
    return X, rng.uniform(-0.3, 0.3, (T, nu)), rng.uniform(-2.0, 2.0, (T, nv)), 0.05 + 0.01 * np.arange(T)


def stats(ts):
    ts = sorted(ts)
    return f"{1e3 * ts[len(ts) // 2]:.3f} ({1e3 * ts[0]:.3f} - {1e3 * ts[-1]:.3f}) ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="quadruped"); ap.add_argument("--T", type=int, default=32); ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--passes", type=int, default=2); ap.add_argument("--centered", action="store_true"); ap.add_argument("--only", default="")
    a = ap.parse_args()
    m, task, d = REGISTRY[a.model]()
    mocap = np.asarray(d["mocap"], float) if len(d["mocap"]) else None
    X, U, A, Tm = window(m, d, a.T)
    nv, nd, nu = m["nv"], 2 * m["nv"] + m["na"], m["nu"]
    be = HipBackend(m, task, max_samples=256, max_horizon=2)
    k = 2 if a.centered else 1
    paths = {"transition_fd": (lambda: be.transition_fd(X, U, Tm, mocap=mocap, eps=1e-6, centered=a.centered), a.T * (1 + k * (nd + nu)))}
    if hasattr(be, "inverse_fd"):
        paths["inverse_fd"] = (lambda: be.inverse_fd(X, U, A, Tm, mocap=mocap, discrete=True, eps=1e-6, centered=a.centered), a.T * (1 + 3 * k * nv))
        paths["inverse_batch"] = (lambda: be.inverse_batch(np.tile(X, (1 + 3 * nv, 1)), np.tile(U, (1 + 3 * nv, 1)), np.tile(A, (1 + 3 * nv, 1)),
                                                            np.tile(Tm, 1 + 3 * nv), mocap=mocap, discrete=True), a.T * (1 + 3 * nv))
    if a.only:
        paths = {a.only: paths[a.only]}
    for fn, _ in paths.values():                    # warm-up: code objects, buffers
        o = fn(); fn()
        assert not o["failure"].any(), o["failure"]
    for p in range(a.passes):
        for name, (fn, evals) in paths.items():     # the paths alternate inside a pass
            ts = []
            for _ in range(a.calls):
                t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
            print(f"pass {p + 1} {a.model} T={a.T} {'centred' if a.centered else 'one-sided'} {name}: {stats(ts)}, {evals} evaluations", flush=True)
    be.close()


if __name__ == "__main__":
    main()
