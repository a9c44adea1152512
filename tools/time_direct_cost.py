#!/usr/bin/env python3
"""Host wall time of the direct optimiser's window cost, gradient and band Hessian on the A1:
  (a) cost_derivatives    mjpc_hip_direct_cost_derivatives: everything on the device, nothing downloaded in between
  (b) fd_assemble_host    the route without it: mjpc_hip_inverse_fd with all six blocks downloaded, then DirectCost::AssembleHost
  (c) cost_nwin1 / 8      mjpc_hip_direct_cost, one and eight candidate windows in one call
and the algebra alone on given arrays (assemble on the device, assemble_host, fd_assemble = inverse_fd then the device's assemble).

usage: tools/time_direct_cost.py [--model quadruped] [--T 32] [--calls 5] [--passes 2] [--only cost_derivatives|fd_assemble_host|cost_nwin1|cost_nwin8|assemble|assemble_host|fd_assemble]
The window is tools/time_inverse_fd.py's (the model's default state with seeded nudges), one-sided, eps = 1e-6, discrete = 1.  The sensors
are the task's cost terms (one sensor per term, its rows the term's, quadratic norm, acceleration stage), every dof's velocity blocks
are -1/h and 1/h (a quaternion dof's dense 3 x 3 block costs the kernels the same: they contract over all nv), the residuals are the
inverse evaluation's own rows and forces.  Prints one line per pass and path: median (min - max) in ms.  With --only one path runs alone,
for a profiler run of its own, e.g.
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/time_direct_cost.py --only cost_derivatives
whose kernel statistics hold the dc_* kernels, the inverse kernel and the two ifd_* kernels.  DESIGN section 8m holds the recorded figures."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mujoco_mpc_amd import capi                          # noqa: E402
from mujoco_mpc_amd.derivatives import DirectCost       # noqa: E402
from mujoco_mpc_amd.modelgen import REGISTRY             # noqa: E402
from mujoco_mpc_amd.planner import HipBackend            # noqa: E402
from time_inverse_fd import stats, window                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="quadruped"); ap.add_argument("--T", type=int, default=32); ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--passes", type=int, default=2); ap.add_argument("--only", default="")
    a = ap.parse_args()
    m, task, d = REGISTRY[a.model]()
    mocap = np.asarray(d["mocap"], float) if len(d["mocap"]) else None
    T, nv, nr, h = a.T, m["nv"], task["num_residual"], float(m["timestep"])
    X, U, A, Tm = window(m, d, T)
    be = HipBackend(m, task, max_samples=256, max_horizon=2)
    dim = [int(v) for v in task["dim_norm_residual"][:task["num_term"]]]
    assert sum(dim) == nr
    spec = dict(sensor_dim=dim, sensor_stage=[2] * len(dim), sensor_norm=[0] * len(dim), sensor_norm_parameter=np.zeros((len(dim), 2)),
                noise_sensor=np.ones(len(dim)), noise_process=np.ones(nv))
    s = capi.direct_settings(timestep=h, **spec)
    host = DirectCost(nv, nr, h, **spec)
    fd = lambda: be.inverse_fd(X, U, A, Tm, mocap=mocap, discrete=True, eps=1e-6)      # noqa: E731
    o = fd()
    assert not o["failure"].any(), o["failure"]
    ev = be.inverse_batch(X, U, A, Tm, mocap=mocap, discrete=True)
    V0 = np.tile(-np.eye(nv) / h, (T, 1, 1)); V1 = np.tile(np.eye(nv) / h, (T, 1, 1))
    blocks = lambda o: (ev["residual"], ev["qfrc_inverse"], o["DfDq"], o["DfDv"], o["DfDa"], o["DsDq"], o["DsDv"], o["DsDa"], V0, V1)      # noqa: E731
    # the window calls: the window's configurations alone go up (velocities and accelerations are the device's own, so the rows differ from
    # the seeded ones above: same sizes, same work); measurements zero
    nq = m["nq"]
    Q, ys, yf = X[:, :nq], np.zeros((T, nr)), np.zeros((T, nv))
    Q8 = np.tile(Q, (8, 1, 1))
    paths = {"cost_derivatives": lambda: be.direct_cost_derivatives(s, Q, None, U, Tm, ys, yf, mocap=mocap, eps=1e-6),          # (a)
             "fd_assemble_host": lambda: host.assemble_host(*blocks(fd())),                                                      # (b) the parent's route
             "cost_nwin1": lambda: be.direct_cost(s, Q, None, U, Tm, ys, yf, mocap=mocap),                                       # (c)
             "cost_nwin8": lambda: be.direct_cost(s, Q8, None, U, Tm, ys, yf, mocap=mocap),
             "assemble": lambda: be.direct_assemble(s, *blocks(o)), "assemble_host": lambda: host.assemble_host(*blocks(o)),
             "fd_assemble": lambda: be.direct_assemble(s, *blocks(fd()))}
    if a.only:
        paths = {a.only: paths[a.only]}
    got = {name: fn() for name, fn in paths.items()}          # warm-up: code objects, buffers
    if "assemble" in got and "assemble_host" in got:
        assert all(np.array_equal(got["assemble"][k], got["assemble_host"][k]) for k in ("cost", "gradient", "hessian_band")), "device and host differ"
    for p in range(a.passes):
        for name, fn in paths.items():          # the paths alternate inside a pass
            ts = []
            for _ in range(a.calls):
                t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
            print(f"pass {p + 1} {a.model} T={T} nv={nv} ns={nr} {name}: {stats(ts)}", flush=True)
    be.close()


if __name__ == "__main__":
    main()
