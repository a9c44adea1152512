"""Loader for the 1-lane emulation build of the feedback-policy rollout kernel (tests/emu/emu_feedback.cpp; TEST INFRASTRUCTURE ONLY)."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import emu_lib
from mujoco_mpc_amd import capi

EMU_SO = os.path.join(emu_lib.EMU_DIR, "libmjpc_emu_feedback.so")
c_double_p = emu_lib.c_double_p
c_int_p = emu_lib.c_int_p


class EmuFbOut(C.Structure):
    _fields_ = [("returns", c_double_p), ("failure", c_int_p), ("states", c_double_p), ("actions", c_double_p), ("times", c_double_p),
                ("residual", c_double_p), ("costs", c_double_p), ("trace", c_double_p), ("diag", c_int_p),
                ("xbar", c_double_p), ("ubar", c_double_p), ("kbar", c_double_p), ("Kbar", c_double_p)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(emu_lib.ROOT, "mujoco_mpc_amd", "csrc")
        src = os.path.join(emu_lib.EMU_DIR, "emu_feedback.cpp")
        srcs = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
        with open(os.path.join(emu_lib.EMU_DIR, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if (not os.path.exists(EMU_SO)) or any(os.path.getmtime(s_) > os.path.getmtime(EMU_SO) for s_ in srcs):
                tmp = EMU_SO + f".{os.getpid()}.tmp"
                subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", tmp, src])
                os.replace(tmp, EMU_SO)
        _lib = C.CDLL(EMU_SO)
        _lib.emu_plan_feedback.argtypes = [C.POINTER(capi.MjpcHipModel), C.POINTER(capi.MjpcHipTask), C.POINTER(capi.MjpcHipPlanInput),
                                           C.POINTER(capi.MjpcHipFeedbackPolicy), C.POINTER(EmuFbOut)]
        _lib.emu_atan2_cr.argtypes = [C.c_double, C.c_double]; _lib.emu_atan2_cr.restype = C.c_double
    return _lib


def atan2_cr(y, x):
    return lib().emu_atan2_cr(float(y), float(x))


def plan_feedback(model, task, state, time, horizon, times, states, actions, feedback_gain, action_step, feedback_scaling, action_improvement=None,
                  mode=capi.FEEDBACK_INDEXED, representation=1, use_feedback=True, mocap=None, candidate_offset=0):
    """Every candidate's rows [N][H][...] under the feedback policy, and the [H] tables the rollout read."""
    cm = capi.CModel(model, task)
    N = int(len(np.ravel(action_step))); H = int(horizon)
    inp = capi.make_plan_input(cm, state, mocap, time, np.zeros(1), np.zeros(model["nu"]), 0, N, H, candidate_offset=candidate_offset,
                               num_local=N - candidate_offset)
    pol = capi.make_feedback_policy(times, states, actions, feedback_gain, action_step, feedback_scaling, action_improvement=action_improvement,
                                    mode=mode, representation=representation, use_feedback=use_feedback)
    nl = N - candidate_offset
    ds = model["nq"] + model["nv"] + model["na"]; nu = model["nu"]; nr = task["num_residual"]; ntr = 3 * task["num_trace"]
    nd = 2 * model["nv"] + model["na"]
    out = dict(returns=np.zeros(nl), failure=np.zeros(nl, np.int32), states=np.zeros((nl, H, ds)), actions=np.zeros((nl, H, nu)),
               times=np.zeros((nl, H)), residual=np.zeros((nl, H, nr)), costs=np.zeros((nl, H)), trace=np.zeros((nl, H, max(ntr, 1))),
               diag=np.zeros((nl, 4), np.int32), xbar=np.full((H, ds), np.nan), ubar=np.full((H, nu), np.nan), kbar=np.full((H, nu), np.nan),
               Kbar=np.full((H, nu, nd), np.nan))
    o = EmuFbOut()
    for k, _ in EmuFbOut._fields_:
        setattr(o, k, out[k].ctypes.data_as(c_int_p if k in ("failure", "diag") else c_double_p))
    rc = lib().emu_plan_feedback(C.byref(cm.c_model), C.byref(cm.c_task), C.byref(inp), C.byref(pol), C.byref(o))
    assert rc > 0, rc
    out["trace"] = out["trace"][:, :, :ntr]
    return out
