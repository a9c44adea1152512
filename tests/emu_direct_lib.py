"""Loader for the 1-lane emulation build of the direct optimiser's window-cost kernels (tests/emu/emu_direct.cpp; TEST INFRASTRUCTURE
ONLY)."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import emu_lib
from mujoco_mpc_amd import capi

EMU_SO = os.path.join(emu_lib.EMU_DIR, "libmjpc_emu_direct.so")
c_double_p = emu_lib.c_double_p

OUTPUTS = ("cost", "gradient", "hessian_band", "block_sensor", "block_force", "norm_gradient_sensor", "norm_gradient_force", "residual_sensor",
           "residual_force")

_lib = None


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(emu_lib.ROOT, "mujoco_mpc_amd", "csrc")
        src = os.path.join(emu_lib.EMU_DIR, "emu_direct.cpp")
        srcs = [src, os.path.join(emu_lib.ROOT, "include", "mjpc_hip.h")] + [os.path.join(csrc, f) for f in ("direct_cost.h", "cost_derivatives.h", "spmd.h", "dmath.h")]
        with open(os.path.join(emu_lib.EMU_DIR, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if (not os.path.exists(EMU_SO)) or any(os.path.getmtime(s_) > os.path.getmtime(EMU_SO) for s_ in srcs):
                tmp = EMU_SO + f".{os.getpid()}.tmp"
                subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", tmp, src])
                os.replace(tmp, EMU_SO)
        _lib = C.CDLL(EMU_SO)
        _lib.emu_direct_assemble.argtypes = [C.c_int] * 3 + [C.POINTER(capi.MjpcHipDirectSettings)] + [c_double_p] * 19
    return _lib


def _dp(a):
    return (a if a.size else np.zeros(1)).ctypes.data_as(c_double_p)


def assemble(settings, residual_sensor, residual_force, DfDq, DfDv, DfDa, DsDq, DsDv, DsDa, dvdq0, dvdq1, fill=np.nan):
    """the kernels of mjpc_hip_direct_assemble played in one thread; the outputs start as `fill` (NaN): what is never written keeps it"""
    f64 = lambda a, *shape: np.ascontiguousarray(a, dtype=np.float64).reshape(*shape)      # noqa: E731
    DfDq = f64(DfDq, -1, *np.shape(DfDq)[-2:]); T, nv = DfDq.shape[0], DfDq.shape[-1]
    ns = settings.num_sensor_rows
    DsDq = f64(DsDq, T, -1, nv); nr = DsDq.shape[1]
    ins = [f64(residual_sensor, T, ns), f64(residual_force, T, nv), DfDq, f64(DfDv, T, nv, nv), f64(DfDa, T, nv, nv), DsDq, f64(DsDv, T, nr, nv),
           f64(DsDa, T, nr, nv), f64(dvdq0, T, nv, nv), f64(dvdq1, T, nv, nv)]
    shapes = [(3,), (T * nv,), (T * nv, 3 * nv), (T, ns, 3 * nv), (T, nv, 3 * nv), (T, ns), (T, nv), (T, ns), (T, nv)]
    o = {k: np.full(sh, fill) for k, sh in zip(OUTPUTS, shapes)}
    rc = lib().emu_direct_assemble(T, nv, nr, C.byref(settings), *[_dp(a) for a in ins], *[_dp(a) for a in o.values()])
    assert rc == 0, rc
    return o


def window(model, q, act=None, ctrl=None, time=None, h=None, blocks=True):
    """dc_window_kernel / dc_vblock_kernel played in one thread: q [nwin, T, nq] -> dict(x [nwin, T, ds], u, a [nwin, T, nv], time [nwin, T],
    dvdq0, dvdq1 [T, nv, nv] of window 0)"""
    import transition_mirror as tm
    nq, nv, na, nu = model["nq"], model["nv"], model["na"], model["nu"]
    q = np.ascontiguousarray(q, dtype=np.float64); q = q.reshape((1,) + q.shape) if q.ndim == 2 else q
    W, T = q.shape[:2]
    f = lambda a, n: np.ascontiguousarray(np.broadcast_to(np.zeros((1, T, n)) if a is None or n == 0 else np.asarray(a, float).reshape(-1, T, n), (W, T, n)))      # noqa: E731
    act, ctrl = f(act, na), f(ctrl, nu)
    time = np.ascontiguousarray(np.zeros(T) if time is None else time, dtype=np.float64)
    dofmap = np.ascontiguousarray(np.asarray(tm.dofmap(model), np.int32).ravel())
    o = dict(x=np.full((W, T, nq + nv + na), np.nan), u=np.full((W, T, nu), np.nan), a=np.full((W, T, nv), np.nan), time=np.full((W, T), np.nan),
             dvdq0=np.full((T, nv, nv), np.nan), dvdq1=np.full((T, nv, nv), np.nan))
    L = lib()
    L.emu_direct_window.argtypes = [C.c_int] * 6 + [C.c_double, C.POINTER(C.c_int)] + [c_double_p] * 10
    rc = L.emu_direct_window(W, T, nq, nv, na, nu, float(model["timestep"] if h is None else h), dofmap.ctypes.data_as(C.POINTER(C.c_int)), _dp(q), _dp(act),
                             _dp(ctrl), _dp(time), _dp(o["x"]), _dp(o["u"]), _dp(o["a"]), _dp(o["time"]), *([_dp(o["dvdq0"]), _dp(o["dvdq1"])] if blocks else [None, None]))
    assert rc == 0
    return o


def value(settings, T, nv, residual, qfrc, y_sensor, y_force, E=1):
    """dc_residual_kernel, dc_norm_kernel and dc_cost_kernel over the windows whose inverse evaluations are residual [nwin T E, nr], qfrc
    [nwin T E, nv] (slot 0 of every E the base) -> dict(cost [nwin, 3], rs [nwin, T, ns], rf [nwin, T, nv])"""
    residual = np.ascontiguousarray(residual, dtype=np.float64); qfrc = np.ascontiguousarray(qfrc, dtype=np.float64).reshape(-1, nv)
    nr, ns = residual.shape[1], settings.num_sensor_rows
    W = qfrc.shape[0] // (T * E)
    ys = np.ascontiguousarray(y_sensor, dtype=np.float64).reshape(T, ns); yf = np.ascontiguousarray(y_force, dtype=np.float64).reshape(T, nv)
    o = dict(cost=np.full((W, 3), np.nan), rs=np.full((W, T, ns), np.nan), rf=np.full((W, T, nv), np.nan))
    L = lib()
    L.emu_direct_value.argtypes = [C.c_int] * 5 + [C.POINTER(capi.MjpcHipDirectSettings)] + [c_double_p] * 7
    rc = L.emu_direct_value(W, T, nv, nr, E, C.byref(settings), _dp(residual), _dp(qfrc), _dp(ys), _dp(yf), _dp(o["rs"]), _dp(o["rf"]), _dp(o["cost"]))
    assert rc == 0, rc
    return o
