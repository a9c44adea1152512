"""Derivatives along a trajectory on the HIP engine: the C++ `mjpc_hip::ModelDerivatives`, `CostDerivatives` and `Gradient`
(csrc/planner.cc; mjpc/planners/model_derivatives.{h,cc}, cost_derivatives.{h,cc}, gradient/gradient.{h,cc}) driven through their
flat C view (include/mjpc_hip_planner_c.h).

ModelDerivatives: the evaluated knots go to the device in one mjpc_hip_transition_fd call; the knots `skip` leaves out are
interpolated on the host with the reference's weights.  CostDerivatives: one mjpc_hip_cost_derivatives call under the engine's
current cost table.  gradient_compute: the gradient planner's backward recursion on the host, bit-equal to the one
HipBackend.trajectory_gradient runs on the device behind the two.  What iLQG, the gradient planner and iLQS linearise around; the gradient
planner itself is cplanner.GradientPlanner, the host algorithms of iLQG and iLQS are not part of this package.  No CPU fallback: the step evaluations and the cost derivatives
are the engine's kernels.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi, cplanner
from .planner import HipBackend

_dp, _ip = capi.c_double_p, capi.c_int_p
_bound = False


def _lib():
    global _bound
    lib = cplanner.lib()          # installs the planner error handler: a refusal raises cplanner.PlannerError instead of aborting
    if not _bound:
        lib.mjpc_md_create.restype = C.c_void_p
        lib.mjpc_md_create.argtypes = [C.c_int] * 5
        lib.mjpc_md_destroy.argtypes = [C.c_void_p]; lib.mjpc_md_destroy.restype = None
        lib.mjpc_md_reset.argtypes = [C.c_void_p, C.c_int]; lib.mjpc_md_reset.restype = None
        lib.mjpc_md_compute.argtypes = [C.c_void_p, C.c_void_p, _dp, _dp, _dp, C.c_int, C.c_double, C.c_int, C.c_int, _dp, _dp]
        lib.mjpc_md_index_sets.argtypes = [C.c_void_p, C.c_int, C.c_int]; lib.mjpc_md_index_sets.restype = None
        lib.mjpc_md_interpolate.argtypes = [C.c_void_p]; lib.mjpc_md_interpolate.restype = None
        lib.mjpc_md_indices.argtypes = [C.c_void_p, _ip, _ip, _ip]; lib.mjpc_md_indices.restype = None
        lib.mjpc_md_blocks.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip]; lib.mjpc_md_blocks.restype = None
        lib.mjpc_cd_create.restype = C.c_void_p
        lib.mjpc_cd_create.argtypes = [C.c_int] * 4
        lib.mjpc_cd_destroy.argtypes = [C.c_void_p]; lib.mjpc_cd_destroy.restype = None
        lib.mjpc_cd_reset.argtypes = [C.c_void_p, C.c_int]; lib.mjpc_cd_reset.restype = None
        lib.mjpc_cd_compute.argtypes = [C.c_void_p, C.c_void_p, _dp, _dp, _dp, C.c_int, C.c_int]
        lib.mjpc_cd_blocks.argtypes = [C.c_void_p, C.c_int] + [_dp] * 6; lib.mjpc_cd_blocks.restype = None
        lib.mjpc_gd_gradient_compute.argtypes = [C.c_int] * 3 + [_dp] * 9
        _bound = True
    return lib


def _ptr(a):
    return (a if a.size else np.zeros(1)).ctypes.data_as(_dp)


def gradient_compute(A, B, cx, cu):
    """Gradient::Compute on the host (no GPU): A [T-1 or more, nd, nd], B [.., nd, nu], cx [T, nd], cu [T, nu] ->
    dict(k [T, nu], Vx [T, nd], Qx [T-1, nd], Qu [T-1, nu], dV [2], status)."""
    cx = np.ascontiguousarray(cx, dtype=np.float64); cu = np.ascontiguousarray(cu, dtype=np.float64)
    T, nd = cx.shape; nu = cu.shape[1]
    A = np.ascontiguousarray(A, dtype=np.float64).reshape(-1); B = np.ascontiguousarray(B, dtype=np.float64).reshape(-1)
    if T >= 2 and (A.size < (T - 1) * nd * nd or B.size < (T - 1) * nd * nu):
        raise ValueError("gradient_compute: A / B hold fewer than T - 1 blocks")
    o = dict(k=np.zeros((T, nu)), Vx=np.zeros((T, nd)), Qx=np.zeros((max(T - 1, 0), nd)), Qu=np.zeros((max(T - 1, 0), nu)), dV=np.zeros(2))
    rc = _lib().mjpc_gd_gradient_compute(nd, nu, T, _ptr(A), _ptr(B), _ptr(cx), _ptr(cu), *[_ptr(o[k]) for k in ("k", "Vx", "Qx", "Qu", "dV")])
    cplanner._check()
    o["status"] = rc
    return o


class CostDerivatives:
    """cr [T, nr], cx [T, nd], cu [T, nu], cxx [T, nd, nd], cuu [T, nu, nu], cxu [T, nd, nu] of a trajectory's residual r [T, nr] and its
    Jacobians rx [T, nr, nd], ru [T, nr, nu]; index T - 1 is the terminal knot (its ru is not read)."""

    def __init__(self, model: dict = None, task: dict = None, T=2, dims=None):
        if dims is None:
            dims = (2 * model["nv"] + model["na"], model["nu"], task["num_residual"])
        self.nd, self.nu, self.nr = (int(v) for v in dims)
        self.T = int(T)
        self.lib = _lib()
        self.h = C.c_void_p(self.lib.mjpc_cd_create(self.nd, self.nu, self.nr, self.T))

    def close(self):
        if getattr(self, "h", None):
            self.lib.mjpc_cd_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def compute(self, backend: HipBackend, r, rx, ru, hessians=True):
        r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1, self.nr); T = r.shape[0]
        rx = np.ascontiguousarray(rx, dtype=np.float64).reshape(T, self.nr, self.nd); ru = np.ascontiguousarray(ru, dtype=np.float64).reshape(T, self.nr, self.nu)
        rc = self.lib.mjpc_cd_compute(self.h, backend.h, _ptr(r), _ptr(rx), _ptr(ru), T, int(bool(hessians)))
        cplanner._check()
        if rc != 0:
            raise RuntimeError("CostDerivatives.compute failed: " + self.lib.mjpc_hip_last_error().decode())
        self.T = max(self.T, T)
        nd, nu, nr = self.nd, self.nu, self.nr
        o = dict(cr=np.zeros((T, nr)), cx=np.zeros((T, nd)), cu=np.zeros((T, nu)), cxx=np.zeros((T, nd, nd)), cuu=np.zeros((T, nu, nu)), cxu=np.zeros((T, nd, nu)))
        self.lib.mjpc_cd_blocks(self.h, T, *[_ptr(o[k]) for k in ("cr", "cx", "cu", "cxx", "cuu", "cxu")])
        return o


class ModelDerivatives:
    """A [T, nd, nd], B [T, nd, nu], C [T, nr, nd], D [T, nr, nu] of a nominal trajectory; nd = 2 nv + na, nr = num_residual.
    Dimensions come from (model, task), or are given one by one for host-only use (index sets / interpolation)."""

    def __init__(self, model: dict = None, task: dict = None, T=2, dims=None):
        if dims is None:
            nq, nv, na = model["nq"], model["nv"], model["na"]
            dims = (nq + nv + na, 2 * nv + na, model["nu"], task["num_residual"])
        self.ds, self.nd, self.nu, self.nr = (int(v) for v in dims)
        self.T = int(T)
        self.lib = _lib()
        self.h = C.c_void_p(self.lib.mjpc_md_create(self.ds, self.nd, self.nu, self.nr, self.T))

    def close(self):
        if getattr(self, "h", None):
            self.lib.mjpc_md_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _grow(self, T):
        if T > self.T:
            self.close()
            self.T = int(T)
            self.h = C.c_void_p(self.lib.mjpc_md_create(self.ds, self.nd, self.nu, self.nr, self.T))

    def compute(self, backend: HipBackend, x, u, h, tol=1e-6, mode=0, skip=0, mocap=None, userdata=None):
        """x [T, nq+nv+na], u [T, nu], h [T] knot times -> dict(A, B, C, D, failure, evaluate, interpolate).  Index T - 1 is the
        terminal knot (C only).  mode: 0 one-sided, 1 centred."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, self.ds); T = x.shape[0]
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(T, self.nu); h = np.ascontiguousarray(h, dtype=np.float64).reshape(T)
        self._grow(T)
        mo, ud, pmo, pud = backend._shared(mocap, userdata)
        u_ = u if u.size else np.zeros(1)
        rc = self.lib.mjpc_md_compute(self.h, backend.h, x.ctypes.data_as(_dp), u_.ctypes.data_as(_dp), h.ctypes.data_as(_dp), T, float(tol), int(mode),
                                      int(skip), pmo, pud)
        cplanner._check()
        if rc != 0:
            raise RuntimeError("ModelDerivatives.compute failed: " + self.lib.mjpc_hip_last_error().decode())
        return self.blocks(T)

    def index_sets(self, T, skip):
        """the evaluated and the interpolated indices of (T, skip), as two ascending int arrays (host only)"""
        self._grow(T)
        self.lib.mjpc_md_index_sets(self.h, int(T), int(skip))
        cplanner._check()
        return self._indices()

    def _indices(self):
        n = np.zeros(2, np.int32)
        self.lib.mjpc_md_indices(self.h, None, None, n.ctypes.data_as(_ip))
        ev = np.zeros(max(int(n[0]), 1), np.int32); it = np.zeros(max(int(n[1]), 1), np.int32)
        self.lib.mjpc_md_indices(self.h, ev.ctypes.data_as(_ip), it.ctypes.data_as(_ip), n.ctypes.data_as(_ip))
        return ev[:n[0]], it[:n[1]]

    def set_blocks(self, A, B, C_, D):
        """store the first T blocks (host only: the tests fill the evaluated ones before interpolate())"""
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (A, B, C_, D)]
        T = arrs[0].shape[0]
        self._grow(T)
        self.lib.mjpc_md_blocks(self.h, T, 1, *[(a if a.size else np.zeros(1)).ctypes.data_as(_dp) for a in arrs], None)

    def interpolate(self):
        self.lib.mjpc_md_interpolate(self.h)

    def blocks(self, T):
        nd, nu, nr = self.nd, self.nu, self.nr
        o = dict(A=np.zeros((T, nd, nd)), B=np.zeros((T, nd, nu)), C=np.zeros((T, nr, nd)), D=np.zeros((T, nr, nu)), failure=np.zeros(T, np.int32))
        keep = {k: (v if v.size else np.zeros(1)) for k, v in o.items()}
        self.lib.mjpc_md_blocks(self.h, int(T), 0, *[keep[k].ctypes.data_as(_dp) for k in "ABCD"], keep["failure"].ctypes.data_as(_ip))
        o["evaluate"], o["interpolate"] = self._indices()
        return o
