"""Inputs of the feedback-rollout tests (TEST INFRASTRUCTURE ONLY), shared by the CPU tier (emulation, oracle loop) and the GPU tier: per
model a nominal rollout, the gains of a real backward pass over it (the host C++ iLQGBackwardPass on emulated derivatives: no GPU), the
candidates' steps and the start state, and the references every comparison uses (computed once per case)."""
import contextlib
import functools
import math

import numpy as np

import emu_cost_derivatives_lib as ec
import emu_lib
import emu_transition_lib as et
import riccati_mirror as rm
import transition_cases as tc
from mujoco_mpc_amd import derivatives as D

STEPS = np.array([1.0, 0.1, 0.01, 0.0])         # alpha per candidate; the feedback scales are the same values in reverse
T0 = 0.25                                        # start time of every case


def dims(m, task):
    nq, nv, na, nu = (int(m[k]) for k in ("nq", "nv", "na", "nu"))
    return dict(nq=nq, nv=nv, na=na, nu=nu, ds=nq + nv + na, nd=2 * nv + na, nr=int(task["num_residual"]))


def step_times(t0, h, H):
    """as the rollout accumulates them: time += h once per step"""
    out = np.zeros(H); t = float(t0)
    for i in range(H):
        out[i] = t
        t = t + float(h)
    return out


def ctrlrange(m):
    return np.asarray(m["actuator_ctrlrange"], float).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def case(name, H, seed=1):
    """model, task, mocap, x0; the nominal rollout (emulated, open loop, zero-order knots at the step times); K, k of the backward pass"""
    m, task, d = tc.model(name)
    dd = dims(m, task)
    rng = np.random.default_rng(seed)
    cr = ctrlrange(m)
    mocap = np.asarray(d["mocap"], float) if len(d["mocap"]) else None
    x0 = np.asarray(d["state"], float).copy()
    times = step_times(T0, float(m["timestep"]), H)
    mid, half = 0.5 * (cr[:, 0] + cr[:, 1]), 0.5 * (cr[:, 1] - cr[:, 0])
    u_nom = mid + 0.2 * half * rng.uniform(-1, 1, (H, dd["nu"]))
    nom = emu_lib.plan(m, task, x0, mocap, T0, times, u_nom, 0, 1, H, candidate_knots=u_nom[None])
    assert nom["failure"][0] == 0 and np.array_equal(nom["times"][0], times)
    xs, us, res = nom["states"][0], nom["actions"][0], nom["residual"][0]
    A, B, Cm, Dm, fail = et.transition_fd(m, task, xs, us, times, mocap, last_is_terminal=True, fill=0.0)
    assert not fail.any()
    cd = ec.cost_derivatives(m, task, dd["nd"], dd["nu"], res, Cm, Dm, last_is_terminal=True, fill=0.0)
    bp = D.ILQGBackwardPass(dd["nd"], dd["nu"], H)
    o = bp.riccati_host(A[:H - 1], B[:H - 1], cd["cx"], cd["cu"], cd["cxx"], cd["cxu"], cd["cuu"], us, cr)
    assert o["status"][0] == 1, o["status"]
    K = np.ascontiguousarray(o["K"], float).reshape(H, dd["nu"], dd["nd"]); k = np.ascontiguousarray(o["k"], float).reshape(H, dd["nu"])
    assert np.abs(K).max() > 0
    return dict(name=name, m=m, task=task, mocap=mocap, x0=x0, H=H, times=times, u_nom=u_nom, nominal=nom, xs=xs, us=us, K=K, k=k, dd=dd, cr=cr)


def displaced(c, scale=1.0, seed=5):
    """the start state moved off xbar[0] in its plain coordinates, velocities and activations (quaternions kept)"""
    import transition_mirror as tm
    rng = np.random.default_rng(seed)
    x = c["x0"].copy(); dd = c["dd"]
    for qa, ax in tm.dofmap(c["m"]):
        if ax < 0:
            x[qa] += scale * 0.01 * rng.standard_normal()
    x[dd["nq"]:] += scale * 0.02 * rng.standard_normal(dd["nv"] + dd["na"])
    return x


def time_policy(c, T=5, seed=3):
    """a policy on its own time grid: T knots, the first half a step AFTER the start of the rollout and the last half a step before its
    last policy step (steps fall before, between and after the knots); states / actions / gains cut from the nominal and perturbed (interpolated
    quaternions are then no longer unit: the renormalisation shows)"""
    rng = np.random.default_rng(seed)
    h = float(c["m"]["timestep"]); dd = c["dd"]
    spacing = (c["H"] - 3.0) / (T - 1)
    times = T0 + 0.5 * h + spacing * h * np.arange(T)
    idx = np.minimum(np.round(0.5 + spacing * np.arange(T)).astype(int), c["H"] - 1)
    states = c["xs"][idx] + 0.01 * rng.standard_normal((T, dd["ds"]))
    return dict(times=times, states=states, actions=c["us"][idx].copy(), K=c["K"][idx].copy(), k=c["k"][idx].copy())


class _RuleVector(np.ndarray):
    """a vector whose product with a matrix on its left follows the summation rule: `K @ v` with v of this type goes to the mirror's own
    sequential `_matvec` (Python tries the reflected operator of a subclass first) instead of numpy's BLAS product"""

    def __rmatmul__(self, K):
        return rm._matvec(np.asarray(K, float), np.asarray(self, float))


class _RuleMath:
    """the math module with atan2 replaced by csrc/atan2_cr.h (through the emulation library): the angle function the kernel and the
    host share, where glibc's own atan2 is a last place off in about 3 of 10^4 arguments"""

    def __getattr__(self, name):
        return getattr(math, name)

    @staticmethod
    def atan2(y, x):
        import emu_feedback_lib as ef
        return ef.atan2_cr(y, x)


@contextlib.contextmanager
def summation_rule():
    """riccati_mirror.policy_action AS IT STANDS, with the two operations of it that the mirror's own header rule does not cover brought
    under it for the duration: its gain product `K @ state_diff(...)` (numpy's `@`: BLAS order and fusing) runs through rm._matvec, and the
    angle of its quaternion tangent through atan2_cr.  Nothing else of the function is touched; outside the context it is what it was."""
    state_diff, mth = rm.state_diff, rm.math
    rm.state_diff = lambda *a, **k: state_diff(*a, **k).view(_RuleVector)
    rm.math = _RuleMath()
    try:
        yield
    finally:
        rm.state_diff, rm.math = state_diff, mth


def host_actions(c, out, pol, mode, representation, alpha, scale, use_feedback=True, with_improvement=True):
    """what iLQGPolicy::Action (C++ host), riccati_mirror.policy_action under the summation rule (summation_rule above) and the same function
    with numpy's own product and glibc's atan2 give at every recorded (state, time) of every candidate: [N][H-1][nu] each"""
    m = c["m"]; N, H = out["states"].shape[:2]
    host = np.zeros((N, H - 1, c["dd"]["nu"])); mirror = np.zeros_like(host); blas = np.zeros_like(host)
    for i in range(N):
        acts = pol["actions"] + pol["k"] * alpha[i] if with_improvement else pol["actions"]          # mju_addScl
        for t in range(H - 1):
            x = out["states"][i, t] if use_feedback else None
            if mode == 0:       # indexed: the policy of Trajectory::RolloutDiscrete, sampled zero-order at its own knot times
                tt, rep, times = out["times"][i, t], 0, c["times"]
            else:
                tt, rep, times = out["times"][i, t], representation, pol["times"]
            host[i, t] = D.ilqg_policy_action(m, times, pol["states"], acts, pol["K"], tt, x, rep, feedback_scaling=scale[i])
            with summation_rule():
                mirror[i, t] = rm.policy_action(m, times, pol["states"], acts, pol["K"], tt, x, rep, feedback_scaling=scale[i])
            blas[i, t] = rm.policy_action(m, times, pol["states"], acts, pol["K"], tt, x, rep, feedback_scaling=scale[i])
    return host, mirror, blas
