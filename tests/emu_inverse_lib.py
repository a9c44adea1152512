"""Loader for the 1-lane emulation build of the inverse-dynamics kernel and its finite-difference kernels (tests/emu/emu_inverse.cpp;
TEST INFRASTRUCTURE ONLY)."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import emu_lib
from emu_transition_lib import _dp, _in, dims
from mujoco_mpc_amd import capi

EMU_SO = os.path.join(emu_lib.EMU_DIR, "libmjpc_emu_inverse.so")
c_double_p = emu_lib.c_double_p
c_int_p = emu_lib.c_int_p

_lib = None


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(emu_lib.ROOT, "mujoco_mpc_amd", "csrc")
        src = os.path.join(emu_lib.EMU_DIR, "emu_inverse.cpp")
        srcs = [src, os.path.join(emu_lib.ROOT, "include", "mjpc_hip.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
        with open(os.path.join(emu_lib.EMU_DIR, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if (not os.path.exists(EMU_SO)) or any(os.path.getmtime(s_) > os.path.getmtime(EMU_SO) for s_ in srcs):
                tmp = EMU_SO + f".{os.getpid()}.tmp"
                subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", tmp, src])
                os.replace(tmp, EMU_SO)
        _lib = C.CDLL(EMU_SO)
        mt = [C.POINTER(capi.MjpcHipModel), C.POINTER(capi.MjpcHipTask)]
        _lib.emu_inverse_batch.argtypes = mt + [C.c_int] + [c_double_p] * 5 + [C.c_int] + [c_double_p] * 3 + [c_int_p]
        _lib.emu_inverse_fd.argtypes = mt + [C.c_int] + [c_double_p] * 5 + [C.c_int, C.c_double, C.c_int] + [c_double_p] * 6 + [c_int_p, c_double_p]
        _lib.emu_inv_step_batch.argtypes = mt + [C.c_int] + [c_double_p] * 4 + [c_double_p, c_double_p, c_int_p]
        _lib.emu_inv_transition_fd.argtypes = mt + [C.c_int] + [c_double_p] * 4 + [C.c_double, C.c_int, C.c_int] + [c_double_p] * 4 + [c_int_p]
        _lib.emu_inv_step_forces.argtypes = mt + [c_double_p, c_double_p, C.c_double, c_double_p, c_double_p, c_double_p]
        _lib.emu_inverse_error.restype = C.c_char_p
    return _lib


def _mocap(model, mocap):
    return _in(mocap if mocap is not None else np.zeros(7 * model["nmocap"]), (-1,))


def inverse_batch(model, task, states, ctrl, qacc, time, mocap=None, discrete=False, fill=np.nan):
    """(qfrc_inverse [n, nv], qfrc_constraint [n, nv], residual [n, nr], failure [n]); a refusal raises ValueError with the message and
    leaves nothing to return"""
    d = dims(model, task)
    states = _in(states, (-1, d["ds"])); n = states.shape[0]
    ctrl = _in(ctrl, (n, d["nu"])); time = _in(time, (n,)); qacc = _in(qacc, (n, d["nv"]))
    cm = capi.CModel(model, task)
    fi = np.full((n, d["nv"]), fill); fc = np.full((n, d["nv"]), fill); res = np.full((n, max(d["nr"], 1)), fill); fail = np.full(n, -1, np.int32)
    rc = lib().emu_inverse_batch(C.byref(cm.c_model), C.byref(cm.c_task), n, _dp(states), _dp(ctrl), _dp(qacc), _dp(time), _dp(_mocap(model, mocap)),
                                 int(bool(discrete)), _dp(fi), _dp(fc), _dp(res), fail.ctypes.data_as(c_int_p))
    if rc != 0:
        raise ValueError(lib().emu_inverse_error().decode())
    return fi, fc, res[:, :d["nr"]], fail


def slots(nv, centered):
    return 1 + (6 if centered else 3) * nv


def inverse_fd(model, task, x, u, qacc, time, mocap=None, discrete=False, eps=1e-6, centered=False, want=(1,) * 6, fill=np.nan):
    """dict(DfDq, DfDv, DfDa [T, nv, nv], DsDq, DsDv, DsDa [T, nr, nv], failure [T], table [T * E, ds + nu + 1 + nv]); want: which of the
    six blocks are asked for (the others are handed over as null and come back as None)"""
    d = dims(model, task)
    x = _in(x, (-1, d["ds"])); T = x.shape[0]
    u = _in(u, (T, d["nu"])); time = _in(time, (T,)); qacc = _in(qacc, (T, d["nv"]))
    cm = capi.CModel(model, task)
    nv, nr = d["nv"], d["nr"]
    names = ["DfDq", "DfDv", "DfDa", "DsDq", "DsDv", "DsDa"]
    blocks = [np.full((T, nv if k < 3 else nr, nv), fill) if want[k] else None for k in range(6)]
    ptr = [(_dp(b) if b is not None and b.size else (_dp(np.zeros(1)) if b is not None else None)) for b in blocks]
    fail = np.full(T, -1, np.int32)
    table = np.full((T * slots(nv, centered), d["ds"] + d["nu"] + 1 + nv), np.nan)
    rc = lib().emu_inverse_fd(C.byref(cm.c_model), C.byref(cm.c_task), T, _dp(x), _dp(u), _dp(qacc), _dp(time), _dp(_mocap(model, mocap)),
                              int(bool(discrete)), float(eps), int(bool(centered)), *ptr, fail.ctypes.data_as(c_int_p), _dp(table))
    if rc != 0:
        raise ValueError(lib().emu_inverse_error().decode())
    out = dict(zip(names, blocks)); out["failure"] = fail; out["table"] = table
    return out


def step_batch(model, task, states, ctrl, time, mocap=None):
    """the one-step kernel as compiled next to the inverse kernel: (next states, residual, failure)"""
    d = dims(model, task)
    states = _in(states, (-1, d["ds"])); n = states.shape[0]
    ctrl = _in(ctrl, (n, d["nu"])); time = _in(time, (n,))
    cm = capi.CModel(model, task)
    nxt = np.full((n, d["ds"]), np.nan); res = np.full((n, max(d["nr"], 1)), np.nan); fail = np.full(n, -1, np.int32)
    rc = lib().emu_inv_step_batch(C.byref(cm.c_model), C.byref(cm.c_task), n, _dp(states), _dp(ctrl), _dp(time), _dp(_mocap(model, mocap)), _dp(nxt),
                                  _dp(res), fail.ctypes.data_as(c_int_p))
    assert rc == 0
    return nxt, res[:, :d["nr"]], fail


def transition_fd(model, task, x, u, time, mocap=None, eps=1e-6, centered=False, last_is_terminal=False, fill=np.nan):
    """mjpc_hip_transition_fd as compiled next to the inverse kernel: (A, B, C, D, failure), emu_transition_lib.transition_fd's form"""
    d = dims(model, task)
    x = _in(x, (-1, d["ds"])); T = x.shape[0]
    u = _in(u, (T, d["nu"])); time = _in(time, (T,))
    cm = capi.CModel(model, task)
    nd, nu, nr = d["nd"], d["nu"], d["nr"]
    A = np.full((T, nd, nd), fill); B = np.full((T, nd, nu), fill); Cm = np.full((T, nr, nd), fill); D = np.full((T, nr, nu), fill)
    fail = np.full(T, -1, np.int32)
    rc = lib().emu_inv_transition_fd(C.byref(cm.c_model), C.byref(cm.c_task), T, _dp(x), _dp(u), _dp(time), _dp(_mocap(model, mocap)), float(eps),
                                     int(centered), int(last_is_terminal), _dp(A), _dp(B), _dp(Cm), _dp(D), fail.ctypes.data_as(c_int_p))
    assert rc == 0
    return A, B, Cm, D, fail


def step_forces(model, task, state, ctrl, time, mocap=None):
    """(qfrc_constraint, qacc) the forward step's solver leaves for one row"""
    d = dims(model, task)
    state = _in(state, (d["ds"],)); ctrl = _in(ctrl, (d["nu"],))
    cm = capi.CModel(model, task)
    fc = np.full(d["nv"], np.nan); qa = np.full(d["nv"], np.nan)
    rc = lib().emu_inv_step_forces(C.byref(cm.c_model), C.byref(cm.c_task), _dp(state), _dp(ctrl), float(time), _dp(_mocap(model, mocap)), _dp(fc), _dp(qa))
    assert rc == 0, rc
    return fc, qa
