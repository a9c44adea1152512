"""Batches of distinct (state, ctrl, time) rows for the one-step / finite-difference tests (TEST INFRASTRUCTURE ONLY), shared by the
CPU tier (emulation, oracle) and the GPU tier, and the oracle's one-step function."""
import numpy as np

import transition_mirror as tm
from mujoco_mpc_amd.modelgen import REGISTRY, humanoid_track, particle
from spill_common import with_capacity


def model(name):
    if name == "particle_copystate":
        return particle(copystate=True)
    if name == "humanoid_spill":                      # the spill flavour's model of the spill tests
        return with_capacity(humanoid_track(), 64, 192)
    return REGISTRY[name]()                           # "quadruped": the A1 at its standing keyframe


def batch(name, n=5, seed=0, spread=1.0):
    """row 0: the model's default state; the others: plain coordinates, velocities and activations nudged (quaternions kept: still
    unit), distinct controls inside the ctrlrange's middle and distinct times"""
    m, task, d = model(name)
    dd = tm.dims(m, task)
    rng = np.random.default_rng(seed)
    X = np.tile(np.asarray(d["state"], float), (n, 1))
    nq, nv = dd["nq"], dd["nv"]
    for i in range(1, n):
        for qa, ax in tm.dofmap(m):
            if ax < 0:
                X[i, qa] += spread * 0.01 * rng.standard_normal()
        X[i, nq:nq + nv] += spread * 0.05 * rng.standard_normal(nv)
        if dd["na"]:
            X[i, nq + nv:] += spread * 0.05 * rng.standard_normal(dd["na"])
    U = rng.uniform(-0.3, 0.3, (n, dd["nu"]))
    T = 0.05 + 0.1 * np.arange(n)
    mocap = np.asarray(d["mocap"], float) if len(d["mocap"]) else None
    return m, task, mocap, X, U, T


def oracle_step(m, task, mocap):
    """(states, ctrl, time) -> (next, residual, failure) through Oracle.plan(N=1, H=2, P=1, candidate knots = ctrl), row by row"""
    import oracle_lib as ol
    o = ol.Oracle(m, task)
    nr = task["num_residual"]

    def step(S, U, T):
        S = np.atleast_2d(np.asarray(S, float)); n = S.shape[0]
        U = np.asarray(U, float).reshape(n, -1); T = np.asarray(T, float).reshape(n)
        nxt = np.zeros_like(S); res = np.zeros((n, nr)); fail = np.zeros(n, np.int32)
        for i in range(n):
            r = o.plan(S[i], mocap, T[i], np.array([0.0]), U[i:i + 1], 0, 1, 2, candidate_knots=U[i].reshape(1, 1, -1))
            nxt[i] = r["states"][0, 1]; res[i] = r["residual"][0, 0]; fail[i] = r["failure"][0]
        return nxt, res, fail
    return step


def nudge_case(m, U, eps=1e-4):
    """the model with the ctrlranges of its first four actuators rewritten around U[0]: actuator 0 sits at hi, 1 at lo, 2 inside,
    3 in a range narrower than eps (no nudge fits: a zero column); every row of U gets row 0's values there"""
    m = dict(m)
    assert m["nu"] >= 4
    rng = np.array(m["actuator_ctrlrange"], float).reshape(-1, 2).copy()
    lim = np.array(m["actuator_ctrllimited"]).ravel().copy()
    U = U.copy(); U[:, :4] = U[0, :4]
    u = U[0]
    rng[0] = (u[0] - 0.5, u[0]); rng[1] = (u[1], u[1] + 0.5); rng[2] = (u[2] - 0.5, u[2] + 0.5); rng[3] = (u[3] - 0.25 * eps, u[3] + 0.25 * eps)
    lim[:4] = 1
    m["actuator_ctrlrange"] = rng.reshape(np.asarray(m["actuator_ctrlrange"]).shape); m["actuator_ctrllimited"] = lim
    return m, U, eps
