#!/usr/bin/env python3
"""Host wall time of one state-estimator update: mjpc_hip::Unscented::Update and mjpc_hip::Kalman::Update (mujoco_mpc_amd/estimators.py:
one mjpc_hip_unscented_moments, or two mjpc_hip_linearize_step, plus the C++ filter algebra) against the same update composed from the
calls the engine had before them - step_batch over a sigma table built on the host with the moments summed on the host; transition_fd
plus step_batch per half-step - with the host part in vectorised numpy.  The paths alternate in one process.

usage: tools/time_estimators.py [--model quadruped|humanoid_track] [--calls 5] [--passes 2] [--only unscented|kalman|unscented_composed|kalman_composed]
                                [--imu-site torso] [--touch-sites FR,FL,RR,RL]
The measurement is the trunk's (root body's) position plus the joint positions behind the free joint; --imu-site / --touch-sites add
an IMU (gyro + accelerometer, 6 rows) and touch rows, which the step kernel fills in its late phase.  Prints one line per pass and
path: median (min - max) in ms.  With --only one path runs alone, for a profiler run of its own, e.g.
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/time_estimators.py --only unscented
whose kernel statistics hold ukf_sigma_kernel, the step kernel, ukf_mean_kernel and ukf_cov_kernel.  DESIGN section 8j holds the
recorded figures."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mujoco_mpc_amd import estimators as E                         # noqa: E402
from mujoco_mpc_amd.modelgen import REGISTRY                       # noqa: E402
from mujoco_mpc_amd.modelgen.residual_table import ResidualTable   # noqa: E402
from mujoco_mpc_amd.planner import HipBackend                      # noqa: E402
from time_trajectory_gradient import stats                         # noqa: E402


def quat_mul(a, b):
    return np.stack([a[:, 0] * b[:, 0] - a[:, 1] * b[:, 1] - a[:, 2] * b[:, 2] - a[:, 3] * b[:, 3],
                     a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0] + a[:, 2] * b[:, 3] - a[:, 3] * b[:, 2],
                     a[:, 0] * b[:, 2] - a[:, 1] * b[:, 3] + a[:, 2] * b[:, 0] + a[:, 3] * b[:, 1],
                     a[:, 0] * b[:, 3] + a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1] + a[:, 3] * b[:, 0]], axis=1)


def integrate(x, Cv, nq, nv):
    """rows x (+) Cv[r] for a model whose only quaternion is the free joint's at qpos 3:7 (dofs 3:6), vectorised over the rows"""
    S = np.tile(x, (Cv.shape[0], 1))
    S[:, :3] += Cv[:, :3]; S[:, 7:nq] += Cv[:, 6:nv]; S[:, nq:] += Cv[:, nv:]
    w = Cv[:, 3:6]; n = np.linalg.norm(w, axis=1)
    axis = np.where(n[:, None] > 1e-15, w / np.maximum(n, 1e-300)[:, None], [1.0, 0.0, 0.0])
    r = np.concatenate([np.cos(0.5 * n)[:, None], axis * np.sin(0.5 * n)[:, None]], axis=1)
    q = quat_mul(np.tile(x[3:7] / np.linalg.norm(x[3:7]), (Cv.shape[0], 1)), r)
    S[:, 3:7] = q / np.linalg.norm(q, axis=1)[:, None]
    return S


def tangent(Y, mean, nq, nv):
    """rows Y[r] (-) mean, same model shape"""
    D = np.empty((Y.shape[0], 2 * nv + Y.shape[1] - nq - nv))
    D[:, :3] = Y[:, :3] - mean[:3]; D[:, 6:nv] = Y[:, 7:nq] - mean[7:nq]; D[:, nv:] = Y[:, nq:] - mean[nq:]
    mc = np.tile(mean[3:7] * [1, -1, -1, -1], (Y.shape[0], 1))
    d = quat_mul(mc, Y[:, 3:7])
    s = np.linalg.norm(d[:, 1:], axis=1)
    ang = 2 * np.arctan2(s, d[:, 0]); ang = np.where(ang > np.pi, ang - 2 * np.pi, ang)
    D[:, 3:6] = d[:, 1:] / np.maximum(s, 1e-300)[:, None] * ang[:, None]
    return D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="quadruped"); ap.add_argument("--calls", type=int, default=5); ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--imu-site", default="", help="add late rows to the measurement: gyro and accelerometer of this site (6 rows) and one touch row per --touch-site")
    ap.add_argument("--touch-sites", default="", help="comma-separated sites, each with a spherical touch zone of radius 0.03")
    a = ap.parse_args()
    m, _, d = REGISTRY[a.model]()
    nq, nv, na, nu = m["nq"], m["nv"], m["na"], m["nu"]
    assert int(m["jnt_type"][0]) == 0 and na == 0 and nq == nv + 1, "the composed path's numpy is written for one free joint followed by hinges / slides"
    nd = 2 * nv
    t = ResidualTable(m)
    t.sum(t.pos("xbody", int(m["jnt_bodyid"][0]))); t.sum(t.qpos()[7:])
    if a.imu_site:                                                    # late rows: the step kernel runs its late phase
        t.sum(t.gyro(a.imu_site)); t.sum(t.accelerometer(a.imu_site))
    for s_ in filter(None, a.touch_sites.split(",")):
        t.sum(t.touch(s_, "sphere", (0.03,)))
    task = t.measurement(); ns = task["num_residual"]
    be = HipBackend(m, task, max_samples=256, max_horizon=2)
    mocap = np.asarray(d["mocap"], float) if len(d["mocap"]) else None
    x0 = np.asarray(d["state"], float); u = np.zeros(nu); h = m["timestep"]
    y = be.step_batch(x0[None], u[None], np.zeros(1), mocap=mocap)["residual"][0]
    ukf, ekf = E.Unscented(be), E.Kalman(be)
    for f in (ukf, ekf):
        f.SetShared(mocap=mocap)
    w = ukf.weights
    wm = np.full(2 * nd + 1, w["weight_sigma"]); wm[-1] = w["weight_mean0"]
    wc = np.full(2 * nd + 1, w["weight_sigma"]); wc[-1] = w["weight_covariance0"]
    Q, R = np.full(nd, 1e-4), np.full(ns, 1e-4)

    def unscented():
        ukf.Reset(x0, 0.0)
        assert ukf.Update(u, y) == E.OK

    def kalman():
        ekf.Reset(x0, 0.0)
        assert ekf.Update(u, y) == E.OK

    def unscented_composed():
        P = 1e-4 * np.eye(nd)
        Cv = (w["sigma_step"] * np.linalg.cholesky(P)).T
        S = np.vstack([integrate(x0, Cv, nq, nv), integrate(x0, -Cv, nq, nv), x0[None]])
        o = be.step_batch(S, np.tile(u, (len(S), 1)), np.zeros(len(S)), mocap=mocap)
        assert not o["failure"].any()
        Y, Z = o["next_states"], o["residual"]
        sm = wm @ Y; ym = wm @ Z
        K = 4.0 * np.einsum("j,ja,jb->ab", wc, Y[:, 3:7], Y[:, 3:7]) - wc.sum() * np.eye(4)
        v = np.linalg.eigh(K)[1][:, -1]
        sm[3:7] = -v if v @ Y[-1, 3:7] < 0 else v
        D = np.hstack([tangent(Y, sm, nq, nv), Z - ym])
        cov = (D.T * wc) @ D + np.diag(np.concatenate([Q, R]))
        G = np.linalg.solve(cov[nd:, nd:], cov[:nd, nd:].T).T
        corr = G @ (y - ym)
        Pn = cov[:nd, :nd] - G @ cov[:nd, nd:].T
        return integrate(sm, corr[None], nq, nv)[0], 0.5 * (Pn + Pn.T)

    def kalman_composed():
        P = 1e-4 * np.eye(nd); x = x0
        fd = be.transition_fd(x[None], u[None], np.zeros(1), mocap=mocap, eps=1e-6)
        st = be.step_batch(x[None], u[None], np.zeros(1), mocap=mocap)
        Cm = fd["C"][0]
        G = np.linalg.solve(Cm @ P @ Cm.T + np.diag(R), Cm @ P).T
        x = integrate(x, (G @ (y - st["residual"][0]))[None], nq, nv)[0]
        P = P - G @ Cm @ P
        fd = be.transition_fd(x[None], u[None], np.zeros(1), mocap=mocap, eps=1e-6)
        st = be.step_batch(x[None], u[None], np.zeros(1), mocap=mocap)
        A = fd["A"][0]
        P = A @ P @ A.T + np.diag(Q)
        return st["next_states"][0], 0.5 * (P + P.T)

    def timed(fn):
        t0 = time.perf_counter(); fn(); return time.perf_counter() - t0

    paths = (("unscented", unscented), ("unscented_composed", unscented_composed), ("kalman", kalman), ("kalman_composed", kalman_composed))
    for name, fn in paths:                                            # warm-up
        if a.only in ("", name):
            fn()
    if not a.only:                                                    # the composed paths compute the classes' update
        xs, Ps = unscented_composed()
        assert np.abs(ukf.state - xs).max() < 1e-6 and np.abs(ukf.covariance - Ps).max() < 1e-8
        xs, Ps = kalman_composed()
        assert np.abs(ekf.state - xs).max() < 1e-6 and np.abs(ekf.covariance - Ps).max() < 1e-8
    print(f"{a.model} nd={nd} ns={ns} sigma rows={2 * nd + 1} timestep={h}")
    for p in range(a.passes):
        for name, fn in paths:
            if a.only in ("", name):
                print(f"pass {p + 1} {name:19s} {stats([timed(fn) for _ in range(a.calls)])}")
    ukf.close(); ekf.close(); be.close()


if __name__ == "__main__":
    main()
