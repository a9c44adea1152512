#!/usr/bin/env python3
"""Host wall time of one derivative iteration of the gradient planner: mjpc_hip_trajectory_gradient (fused: one download) against the
composed path (mjpc_hip_transition_fd with its four matrices downloaded, mjpc_hip_cost_derivatives with hessians = 0, the host
Gradient::Compute), alternating in one process, through the C ABI with preallocated arrays.  Also times mjpc_hip_cost_derivatives
with and without Hessians on the matrices of the same trajectory.

usage: tools/time_trajectory_gradient.py [--model quadruped|humanoid_track|...] [--T 36] [--centered] [--calls 5] [--passes 2]
                                         [--only fused|composed|cost|cost0|cost1]      (one path alone: for a profiler run)
Prints one line per pass and path: median (min - max) in ms.  DESIGN section 8f holds the recorded figures."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mujoco_mpc_amd import capi, derivatives                       # noqa: E402
from mujoco_mpc_amd.modelgen import REGISTRY                       # noqa: E402
from mujoco_mpc_amd.planner import HipBackend                      # noqa: E402


def scattered(m, d, T, seed=0):
    """the default state with plain coordinates, velocities and controls scattered; distinct times"""
    rng = np.random.default_rng(seed)
    nq, nv, na, nu = m["nq"], m["nv"], m["na"], m["nu"]
    X = np.tile(np.asarray(d["state"], float), (T, 1))
    quat = np.zeros(nq, bool)
    for j in range(m["njnt"]):
        ty, qa = int(m["jnt_type"][j]), int(m["jnt_qposadr"][j])
        if ty == 0:
            quat[qa + 3:qa + 7] = True
        elif ty == 1:
            quat[qa:qa + 4] = True
    X[1:, :nq][:, ~quat] += 0.01 * rng.standard_normal((T - 1, int((~quat).sum())))
    X[1:, nq:] += 0.05 * rng.standard_normal((T - 1, nv + na))
    return X, rng.uniform(-0.3, 0.3, (T, nu)), 0.05 + m["timestep"] * np.arange(T)


def stats(ts):
    ts = 1e3 * np.asarray(ts)
    return "%.3f ms (%.3f - %.3f)" % (np.median(ts), ts.min(), ts.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="quadruped"); ap.add_argument("--T", type=int, default=36); ap.add_argument("--centered", action="store_true")
    ap.add_argument("--calls", type=int, default=5); ap.add_argument("--passes", type=int, default=2); ap.add_argument("--only", default="")
    a = ap.parse_args()
    m, task, d = REGISTRY[a.model]()
    be = HipBackend(m, task, max_samples=4096, max_horizon=2)
    lib = be.lib
    T, ds, nd, nu, nr = a.T, m["nq"] + m["nv"] + m["na"], 2 * m["nv"] + m["na"], m["nu"], task["num_residual"]
    X, U, Tm = scattered(m, d, T)
    mocap = np.asarray(d["mocap"], float) if len(d["mocap"]) else None
    res = be.step_batch(X, U, Tm, mocap=mocap)["residual"]
    dp = capi.c_double_p
    P = lambda v: v.ctypes.data_as(dp)                              # noqa: E731
    pmo = P(mocap) if mocap is not None else None
    A = np.zeros((T, nd, nd)); B = np.zeros((T, nd, nu)); Cm = np.zeros((T, nr, nd)); Dm = np.zeros((T, nr, nu)); fail = np.zeros(T, np.int32)
    cr = np.zeros((T, nr)); cx = np.zeros((T, nd)); cu = np.zeros((T, nu)); cxx = np.zeros((T, nd, nd)); cuu = np.zeros((T, nu, nu)); cxu = np.zeros((T, nd, nu))
    k = np.zeros((T, nu)); Vx = np.zeros((T, nd)); Qx = np.zeros((T - 1, nd)); Qu = np.zeros((T - 1, nu)); dV = np.zeros(2)
    pf = fail.ctypes.data_as(capi.c_int_p)
    eps, cen = 1e-6, int(a.centered)

    def fused():
        assert lib.mjpc_hip_trajectory_gradient(be.h, T, P(X), P(U), P(Tm), P(res), pmo, None, eps, cen, P(k), P(Vx), P(Qx), P(Qu), P(dV), pf) == 0

    def composed():
        assert lib.mjpc_hip_transition_fd(be.h, T, P(X), P(U), P(Tm), pmo, None, eps, cen, 1, P(A), P(B), P(Cm), P(Dm), pf) == 0
        assert lib.mjpc_hip_cost_derivatives(be.h, T, P(res), P(Cm), P(Dm), 1, 0, P(cr), P(cx), P(cu), None, None, None) == 0
        return derivatives.gradient_compute(A, B, cx, cu)

    def cost(h):
        assert lib.mjpc_hip_cost_derivatives(be.h, T, P(res), P(Cm), P(Dm), 1, h, P(cr), P(cx), P(cu), P(cxx), P(cuu), P(cxu)) == 0

    def timed(fn, *args):
        t0 = time.perf_counter(); fn(*args); return time.perf_counter() - t0

    composed(); fused()                                            # warm-up, and the matrices for cost()
    assert not fail.any(), "a failed evaluation: not a timing state"
    host = composed()
    assert np.array_equal(host["Qu"], Qu) and np.array_equal(host["Vx"], Vx)
    print(f"{a.model} T={T} {'centred' if cen else 'one-sided'} nd+nu={nd + nu} nr={nr}")
    for p in range(a.passes):
        if a.only in ("", "fused"):
            print(f"pass {p + 1} fused     {stats([timed(fused) for _ in range(a.calls)])}")
        if a.only in ("", "composed"):
            print(f"pass {p + 1} composed  {stats([timed(composed) for _ in range(a.calls)])}")
        if a.only in ("", "cost", "cost0"):
            print(f"pass {p + 1} cost derivatives, gradients only {stats([timed(cost, 0) for _ in range(a.calls)])}")
        if a.only in ("", "cost", "cost1"):
            print(f"pass {p + 1} cost derivatives, with Hessians  {stats([timed(cost, 1) for _ in range(a.calls)])}")
    be.close()


if __name__ == "__main__":
    main()
