"""Loader for the 1-lane emulation build of the unscented-moments kernels (tests/emu/emu_estimator.cpp; TEST INFRASTRUCTURE ONLY)."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import emu_lib
from emu_transition_lib import _dp, _in, dims
from mujoco_mpc_amd import capi

EMU_SO = os.path.join(emu_lib.EMU_DIR, "libmjpc_emu_estimator.so")
c_double_p = emu_lib.c_double_p
c_int_p = emu_lib.c_int_p

_lib = None


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(emu_lib.ROOT, "mujoco_mpc_amd", "csrc")
        src = os.path.join(emu_lib.EMU_DIR, "emu_estimator.cpp")
        srcs = [src, os.path.join(emu_lib.EMU_DIR, "emu_transition.cpp")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
        with open(os.path.join(emu_lib.EMU_DIR, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if (not os.path.exists(EMU_SO)) or any(os.path.getmtime(s_) > os.path.getmtime(EMU_SO) for s_ in srcs):
                tmp = EMU_SO + f".{os.getpid()}.tmp"
                subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", tmp, src])
                os.replace(tmp, EMU_SO)
        _lib = C.CDLL(EMU_SO)
        mp, tp = C.POINTER(capi.MjpcHipModel), C.POINTER(capi.MjpcHipTask)
        _lib.emu_ukf_sigma.argtypes = [mp] + [c_double_p] * 3 + [C.c_double, C.c_double] + [c_double_p] * 3
        _lib.emu_unscented_moments.argtypes = ([mp, tp, c_double_p, c_double_p, C.c_double, c_double_p, c_double_p, C.c_double] + [c_double_p] * 3
                                               + [C.c_int, C.c_int] + [c_double_p] * 7 + [c_int_p])
        _lib.emu_ukf_quat_mean.argtypes = [C.c_int] * 4 + [c_double_p, C.c_double, C.c_double, c_double_p]
        _lib.emu_ukf_quat_mean.restype = None
    return _lib


def sigma_table(model, task, x, L, u, sigma_step, time):
    d = dims(model, task); R = 2 * d["nd"] + 1
    cm = capi.CModel(model, task)
    st = np.full((R, d["ds"]), np.nan); ct = np.full((R, max(d["nu"], 1)), np.nan); tt = np.full(R, np.nan)
    rc = lib().emu_ukf_sigma(C.byref(cm.c_model), _dp(_in(x, (d["ds"],))), _dp(_in(L, (d["nd"], d["nd"]))), _dp(_in(u, (d["nu"],))), float(sigma_step),
                             float(time), _dp(st), _dp(ct), _dp(tt))
    assert rc == 0
    return st, ct[:, :d["nu"]], tt


def unscented_moments(model, task, x, L, sigma_step, weights, u, time, noise_process, noise_sensor, first, ns, mocap=None):
    d = dims(model, task); nd, ds = d["nd"], d["ds"]; R = 2 * nd + 1
    cm = capi.CModel(model, task)
    mocap = _in(mocap if mocap is not None else np.zeros(7 * model["nmocap"]), (-1,))
    o = dict(state_mean=np.full(ds, np.nan), sensor_mean=np.full(ns, np.nan), cov_ss=np.full((nd, nd), np.nan), cov_sy=np.full((nd, ns), np.nan),
             cov_yy=np.full((ns, ns), np.nan), sigma_next=np.full((R, ds), np.nan), diff=np.full((R, nd + ns), np.nan))
    fail = np.full(1, -1, np.int32)
    rc = lib().emu_unscented_moments(C.byref(cm.c_model), C.byref(cm.c_task), _dp(_in(x, (ds,))), _dp(_in(L, (nd, nd))), float(sigma_step),
                                     _dp(_in(weights, (3,))), _dp(_in(u, (d["nu"],))), float(time), _dp(mocap), _dp(_in(noise_process, (nd,))),
                                     _dp(_in(noise_sensor, (ns,))), int(first), int(ns), _dp(o["state_mean"]), _dp(o["sensor_mean"]), _dp(o["cov_ss"]),
                                     _dp(o["cov_sy"]), _dp(o["cov_yy"]), _dp(o["sigma_next"]), _dp(o["diff"]), fail.ctypes.data_as(c_int_p))
    assert rc == 0
    o["failure"] = int(fail[0])
    return o


def quat_mean(nq, nv, na, qa, next_state, w_cov0, w_sigma):
    out = np.full(4, np.nan)
    lib().emu_ukf_quat_mean(nq, nv, na, qa, _dp(_in(next_state, (-1,))), float(w_cov0), float(w_sigma), _dp(out))
    return out
