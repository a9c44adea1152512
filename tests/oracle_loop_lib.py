"""A closed loop over the C oracle (TEST INFRASTRUCTURE ONLY): one persistent OData, its warm start zeroed once as oracle_rollout does,
oracle_step per step and oracle_forward at the end, the action of every step computed in Python from the oracle's own state.  OData's
fields are reached through tests/emu/oracle_loop_shim.c, compiled here against oracle/oracle.h."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import oracle_lib as ol

ROOT = ol.ROOT
SHIM_SRC = os.path.join(ROOT, "tests", "emu", "oracle_loop_shim.c")
SHIM_SO = os.path.join(ROOT, "tests", "emu", "liboracle_loop_shim.so")
c_double_p = ol.c_double_p

_shim = None


def shim():
    global _shim
    if _shim is None:
        L = ol.lib()
        deps = [SHIM_SRC, os.path.join(ROOT, "oracle", "oracle.h"), os.path.join(ROOT, "include", "mjpc_hip.h")]
        with open(os.path.join(ROOT, "tests", "emu", ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if (not os.path.exists(SHIM_SO)) or any(os.path.getmtime(s) > os.path.getmtime(SHIM_SO) for s in deps):
                tmp = SHIM_SO + f".{os.getpid()}.tmp"
                subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-o", tmp, SHIM_SRC])
                os.replace(tmp, SHIM_SO)
        S = C.CDLL(SHIM_SO)
        S.shim_begin.argtypes = [C.c_void_p, C.c_void_p, c_double_p, c_double_p, c_double_p, C.c_double]; S.shim_begin.restype = None
        S.shim_set_ctrl.argtypes = [C.c_void_p, C.c_void_p, c_double_p]; S.shim_set_ctrl.restype = None
        S.shim_get_state.argtypes = [C.c_void_p, C.c_void_p, c_double_p]; S.shim_get_state.restype = None
        S.shim_get_time.argtypes = [C.c_void_p]; S.shim_get_time.restype = C.c_double
        S.shim_get_warning.argtypes = [C.c_void_p]; S.shim_get_warning.restype = C.c_int
        S.shim_get_residual.argtypes = [C.c_void_p, C.c_void_p, c_double_p]; S.shim_get_residual.restype = None
        L.oracle_make_data.restype = C.c_void_p; L.oracle_make_data.argtypes = [C.c_void_p]
        L.oracle_free_data.restype = None; L.oracle_free_data.argtypes = [C.c_void_p]
        L.oracle_step.restype = None; L.oracle_step.argtypes = [C.c_void_p, C.c_void_p]
        L.oracle_forward.restype = None; L.oracle_forward.argtypes = [C.c_void_p, C.c_void_p]
        _shim = S
    return _shim


def closed_loop(oracle, state, time, H, policy, mocap=None, userdata=None):
    """states [H][ds], actions [H][nu], times [H], residual [H][nr], costs [H], return, failure of the rollout in which step t < H-1
    applies policy(t, time_t, state_t) (already clamped).  Mirrors oracle_rollout."""
    S = shim(); L = ol.lib()
    m, task = oracle.model, oracle.task
    ds = m["nq"] + m["nv"] + m["na"]; nu = m["nu"]; nr = task["num_residual"]
    dp = lambda a: a.ctypes.data_as(c_double_p)
    x0 = np.ascontiguousarray(state, float)
    mc = np.ascontiguousarray(mocap if mocap is not None and len(mocap) else np.zeros(7 * max(m["nmocap"], 1)), float)
    ud = np.ascontiguousarray(userdata if userdata is not None else np.zeros(max(m["nuserdata"], 1)), float)
    d = L.oracle_make_data(oracle.h)
    try:
        S.shim_begin(oracle.h, d, dp(x0), dp(mc), dp(ud), float(time))
        states = np.zeros((H, ds)); actions = np.zeros((H, nu)); times = np.zeros(H); residual = np.zeros((H, nr)); costs = np.zeros(H)
        states[0] = x0; times[0] = time
        x = np.zeros(ds); r = np.zeros(max(nr, 1))
        for t in range(H - 1):
            a = np.ascontiguousarray(policy(t, times[t], states[t].copy()), float)
            actions[t] = a
            S.shim_set_ctrl(oracle.h, d, dp(a))
            L.oracle_step(oracle.h, d)
            S.shim_get_residual(oracle.h, d, dp(r)); residual[t] = r[:nr]
            if S.shim_get_warning(d):
                return dict(states=states, actions=actions, times=times, residual=residual, costs=costs, ret=1.0e6, failure=S.shim_get_warning(d))
            S.shim_get_state(oracle.h, d, dp(x)); states[t + 1] = x
            times[t + 1] = S.shim_get_time(d)
        if H > 1:
            actions[H - 1] = actions[H - 2]
        L.oracle_forward(oracle.h, d)
        S.shim_get_residual(oracle.h, d, dp(r)); residual[H - 1] = r[:nr]
        fail = S.shim_get_warning(d)
        for t in range(H):
            costs[t] = oracle.cost(residual[t])[0]
        ret = 1.0e6 if fail else costs.sum() / max(H, 1)
        return dict(states=states, actions=actions, times=times, residual=residual, costs=costs, ret=ret, failure=fail)
    finally:
        L.oracle_free_data(d)
