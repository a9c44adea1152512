"""Loader for the 1-lane emulation build of the spill flavour (tests/emu/emu_spill.cpp; TEST INFRASTRUCTURE ONLY)."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import emu_lib
from mujoco_mpc_amd import capi

EMU_SO = os.path.join(emu_lib.EMU_DIR, "libmjpc_emu_spill.so")
SPILL_NONE, SPILL_AUTO, SPILL_ALL = 0, 1, 2          # host.h build(..., spill_mode)

_lib = None


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(emu_lib.ROOT, "mujoco_mpc_amd", "csrc")
        src = os.path.join(emu_lib.EMU_DIR, "emu_spill.cpp")
        srcs = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
        asan = bool(os.environ.get("MJPC_EMU_ASAN"))      # memory-checked build, as for emu_lib
        so = EMU_SO[:-3] + "_asan.so" if asan else EMU_SO
        flags = ["-O1", "-g", "-fsanitize=address"] if asan else ["-O2"]
        with open(os.path.join(emu_lib.EMU_DIR, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if (not os.path.exists(so)) or any(os.path.getmtime(s_) > os.path.getmtime(so) for s_ in srcs):
                tmp = so + f".{os.getpid()}.tmp"
                subprocess.check_call(["g++"] + flags + ["-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", tmp, src])
                os.replace(tmp, so)
        _lib = C.CDLL(so)
        _lib.emu_spill_plan.argtypes = [C.POINTER(capi.MjpcHipModel), C.POINTER(capi.MjpcHipTask), C.POINTER(capi.MjpcHipPlanInput),
                                        C.POINTER(emu_lib.EmuOut), C.c_int, C.POINTER(C.c_int)]
    return _lib


def plan(model, task, state, mocap, time, knot_times, knot_values, interp, N, H, sigma=(0.1, 0.0), noise_eps=None, noise_sel=None,
         mode=SPILL_AUTO):
    """emu_lib.plan on the spill flavour's emulation; out["lds_doubles"], out["slab_doubles"] = the layout it ran with"""
    cm = capi.CModel(model, task)
    inp = capi.make_plan_input(cm, state, mocap, time, knot_times, knot_values, interp, N, H, sigma, noise_eps, noise_sel, 0, 0, 0, None)
    nl = inp.num_local
    ds = model["nq"] + model["nv"] + model["na"]; nu = model["nu"]; nr = task["num_residual"]; ntr = 3 * task["num_trace"]
    P = inp.num_spline_points
    out = dict(returns=np.zeros(nl), failure=np.zeros(nl, np.int32), states=np.zeros((nl, H, ds)),
               actions=np.zeros((nl, H, nu)), times=np.zeros((nl, H)), residual=np.zeros((nl, H, nr)),
               costs=np.zeros((nl, H)), trace=np.zeros((nl, H, max(ntr, 1))), knots=np.zeros((nl, P, nu)),
               diag=np.zeros((nl, 4), np.int32))
    o = emu_lib.EmuOut()
    for k in ["returns", "states", "actions", "times", "residual", "costs", "trace", "knots"]:
        setattr(o, k, out[k].ctypes.data_as(emu_lib.c_double_p))
    o.failure = out["failure"].ctypes.data_as(emu_lib.c_int_p); o.diag = out["diag"].ctypes.data_as(emu_lib.c_int_p)
    slab = C.c_int(0)
    rc = lib().emu_spill_plan(C.byref(cm.c_model), C.byref(cm.c_task), C.byref(inp), C.byref(o), mode, C.byref(slab))
    assert rc > 0
    out["lds_doubles"] = rc; out["slab_doubles"] = slab.value
    out["trace"] = out["trace"][:, :, :ntr]
    return out
