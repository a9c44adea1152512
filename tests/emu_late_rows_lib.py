"""Loader for the 1-lane emulation build of the one-step kernel with its late-row phase (tests/emu/emu_late_rows.cpp; TEST INFRASTRUCTURE ONLY)."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import emu_lib
from emu_transition_lib import _dp, _in, dims
from mujoco_mpc_amd import capi

EMU_SO = os.path.join(emu_lib.EMU_DIR, "libmjpc_emu_late_rows.so")
c_double_p = emu_lib.c_double_p
c_int_p = emu_lib.c_int_p

_lib = None


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(emu_lib.ROOT, "mujoco_mpc_amd", "csrc")
        src = os.path.join(emu_lib.EMU_DIR, "emu_late_rows.cpp")
        srcs = [src, os.path.join(emu_lib.ROOT, "include", "mjpc_hip.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
        with open(os.path.join(emu_lib.EMU_DIR, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if (not os.path.exists(EMU_SO)) or any(os.path.getmtime(s_) > os.path.getmtime(EMU_SO) for s_ in srcs):
                tmp = EMU_SO + f".{os.getpid()}.tmp"
                subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", tmp, src])
                os.replace(tmp, EMU_SO)
        _lib = C.CDLL(EMU_SO)
        mt = [C.POINTER(capi.MjpcHipModel), C.POINTER(capi.MjpcHipTask)]
        _lib.emu_late_step_batch.argtypes = mt + [C.c_int] + [c_double_p] * 4 + [c_double_p, c_double_p, c_int_p]
        _lib.emu_late_blocks.argtypes = mt
        _lib.emu_late_error.restype = C.c_char_p
    return _lib


def step_batch(model, task, states, ctrl, time, mocap=None):
    """(next states, residual rows with the late rows filled, failure bits); a refused table raises ValueError with the library's message"""
    d = dims(model, task)
    states = _in(states, (-1, d["ds"])); n = states.shape[0]
    ctrl = _in(ctrl, (n, d["nu"])); time = _in(time, (n,))
    mocap = _in(mocap if mocap is not None else np.zeros(7 * model["nmocap"]), (-1,))
    cm = capi.CModel(model, task)
    nxt = np.full((n, d["ds"]), np.nan); res = np.full((n, max(d["nr"], 1)), np.nan); fail = np.full(n, -1, np.int32)
    rc = lib().emu_late_step_batch(C.byref(cm.c_model), C.byref(cm.c_task), n, _dp(states), _dp(ctrl), _dp(time), _dp(mocap), _dp(nxt), _dp(res),
                                   fail.ctypes.data_as(c_int_p))
    if rc != 0:
        raise ValueError(lib().emu_late_error().decode())
    return nxt, res[:, :d["nr"]], fail


def late_blocks(model, task):
    """number of late blocks host.h finds (0: the step kernel gets a null table); a refused table raises ValueError with the message"""
    cm = capi.CModel(model, task)
    n = lib().emu_late_blocks(C.byref(cm.c_model), C.byref(cm.c_task))
    if n < 0:
        raise ValueError(lib().emu_late_error().decode())
    return n
