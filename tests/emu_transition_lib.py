"""Loader for the 1-lane emulation build of the one-step and finite-difference kernels (tests/emu/emu_transition.cpp; TEST INFRASTRUCTURE ONLY)."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import emu_lib
from mujoco_mpc_amd import capi

EMU_SO = os.path.join(emu_lib.EMU_DIR, "libmjpc_emu_transition.so")
c_double_p = emu_lib.c_double_p
c_int_p = emu_lib.c_int_p

_lib = None


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(emu_lib.ROOT, "mujoco_mpc_amd", "csrc")
        src = os.path.join(emu_lib.EMU_DIR, "emu_transition.cpp")
        srcs = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
        with open(os.path.join(emu_lib.EMU_DIR, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if (not os.path.exists(EMU_SO)) or any(os.path.getmtime(s_) > os.path.getmtime(EMU_SO) for s_ in srcs):
                tmp = EMU_SO + f".{os.getpid()}.tmp"
                subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", tmp, src])
                os.replace(tmp, EMU_SO)
        _lib = C.CDLL(EMU_SO)
        mt = [C.POINTER(capi.MjpcHipModel), C.POINTER(capi.MjpcHipTask)]
        _lib.emu_step_batch.argtypes = mt + [C.c_int] + [c_double_p] * 4 + [c_double_p, c_double_p, c_int_p]
        _lib.emu_transition_fd.argtypes = mt + [C.c_int] + [c_double_p] * 4 + [C.c_double, C.c_int, C.c_int] + [c_double_p] * 4 + [c_int_p]
    return _lib


def _dp(a):
    return a.ctypes.data_as(c_double_p)


def _in(a, shape):
    a = np.ascontiguousarray(np.asarray(a, np.float64).reshape(shape))
    return a if a.size else np.zeros(1)


def dims(model, task):
    nq, nv, na, nu = model["nq"], model["nv"], model["na"], model["nu"]
    return dict(nq=nq, nv=nv, na=na, nu=nu, ds=nq + nv + na, nd=2 * nv + na, nr=task["num_residual"])


def step_batch(model, task, states, ctrl, time, mocap=None):
    d = dims(model, task)
    states = _in(states, (-1, d["ds"])); n = states.shape[0]
    ctrl = _in(ctrl, (n, d["nu"])); time = _in(time, (n,))
    mocap = _in(mocap if mocap is not None else np.zeros(7 * model["nmocap"]), (-1,))
    cm = capi.CModel(model, task)
    nxt = np.full((n, d["ds"]), np.nan); res = np.full((n, max(d["nr"], 1)), np.nan); fail = np.full(n, -1, np.int32)
    rc = lib().emu_step_batch(C.byref(cm.c_model), C.byref(cm.c_task), n, _dp(states), _dp(ctrl), _dp(time), _dp(mocap), _dp(nxt), _dp(res),
                              fail.ctypes.data_as(c_int_p))
    assert rc == 0
    return nxt, res[:, :d["nr"]], fail


def transition_fd(model, task, x, u, time, mocap=None, eps=1e-6, centered=False, last_is_terminal=False, fill=np.nan):
    d = dims(model, task)
    x = _in(x, (-1, d["ds"])); T = x.shape[0]
    u = _in(u, (T, d["nu"])); time = _in(time, (T,))
    mocap = _in(mocap if mocap is not None else np.zeros(7 * model["nmocap"]), (-1,))
    cm = capi.CModel(model, task)
    nd, nu, nr = d["nd"], d["nu"], d["nr"]
    A = np.full((T, nd, nd), fill); B = np.full((T, nd, nu), fill); Cm = np.full((T, nr, nd), fill); D = np.full((T, nr, nu), fill)
    fail = np.full(T, -1, np.int32)
    rc = lib().emu_transition_fd(C.byref(cm.c_model), C.byref(cm.c_task), T, _dp(x), _dp(u), _dp(time), _dp(mocap), float(eps), int(centered),
                                 int(last_is_terminal), _dp(A), _dp(B), _dp(Cm), _dp(D), fail.ctypes.data_as(c_int_p))
    assert rc == 0
    return A, B, Cm, D, fail
