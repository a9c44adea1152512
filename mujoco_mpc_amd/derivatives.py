"""Derivatives along a trajectory on the HIP engine: the C++ `mjpc_hip::ModelDerivatives`, `CostDerivatives` and `Gradient`
(csrc/planner.cc; mjpc/planners/model_derivatives.{h,cc}, cost_derivatives.{h,cc}, gradient/gradient.{h,cc}) driven through their
flat C view (include/mjpc_hip_planner_c.h).

ModelDerivatives: the evaluated knots go to the device in one mjpc_hip_transition_fd call; the knots `skip` leaves out are
interpolated on the host with the reference's weights.  CostDerivatives: one mjpc_hip_cost_derivatives call under the engine's
current cost table.  gradient_compute: the gradient planner's backward recursion on the host, bit-equal to the one
HipBackend.trajectory_gradient runs on the device behind the two.  What iLQG, the gradient planner and iLQS linearise around; the gradient
planner itself is cplanner.GradientPlanner.  ILQGBackwardPass, boxqp and ilqg_policy_action are iLQG's backward pass (Riccati recursion, box-constrained
control solve, regularisation loop) and policy, on the host and on the device (HipBackend.ilqg_backward_pass / trajectory_ilqg); iLQG's feedback rollouts
and line search, and iLQS, are not part of this package.  InverseDerivatives: the six Jacobians of the inverse dynamics along a window (one
mjpc_hip_inverse_fd call), what the reference's direct optimiser and batch estimator linearise around; the optimiser itself is not part
of this package.  DirectCost: that optimiser's window cost, gradient and band Hessian from those blocks (mjpc_hip_direct_assemble, and
the same algebra on the host).  No CPU fallback: the step and inverse evaluations and the cost derivatives are the engine's kernels.
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
        lib.mjpc_id_create.restype = C.c_void_p
        lib.mjpc_id_create.argtypes = [C.c_int] * 6
        lib.mjpc_id_destroy.argtypes = [C.c_void_p]; lib.mjpc_id_destroy.restype = None
        lib.mjpc_id_set_row_stages.argtypes = [C.c_void_p, _ip]; lib.mjpc_id_set_row_stages.restype = None
        lib.mjpc_id_row_stages_from_table.argtypes = [C.c_void_p, C.POINTER(capi.MjpcHipTask)]
        lib.mjpc_id_row_stages.argtypes = [C.c_void_p, _ip]; lib.mjpc_id_row_stages.restype = None
        lib.mjpc_id_compute.argtypes = [C.c_void_p, C.c_void_p, _dp, _dp, _dp, _dp, C.c_int, C.c_double, C.c_int, C.c_int, _dp, _dp]
        lib.mjpc_id_blocks.argtypes = [C.c_void_p, C.c_int] + [_dp] * 6 + [_ip]; lib.mjpc_id_blocks.restype = None
        lib.mjpc_dc_create.restype = C.c_void_p
        lib.mjpc_dc_create.argtypes = [C.c_int] * 3
        lib.mjpc_dc_destroy.argtypes = [C.c_void_p]; lib.mjpc_dc_destroy.restype = None
        lib.mjpc_dc_set_sensors.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, _ip, _ip, _dp, _dp]; lib.mjpc_dc_set_sensors.restype = None
        lib.mjpc_dc_set_process_noise.argtypes = [C.c_void_p, _dp]; lib.mjpc_dc_set_process_noise.restype = None
        lib.mjpc_dc_set_mask.argtypes = [C.c_void_p, _ip, C.c_int]; lib.mjpc_dc_set_mask.restype = None
        lib.mjpc_dc_set_settings.argtypes = [C.c_void_p, _ip, C.c_double]; lib.mjpc_dc_set_settings.restype = None
        lib.mjpc_dc_assemble.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [_dp] * 10
        lib.mjpc_dc_set_window.argtypes = [C.c_void_p] + [C.c_int] * 4 + [_dp] * 6; lib.mjpc_dc_set_window.restype = None
        lib.mjpc_dc_set_fd.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int]; lib.mjpc_dc_set_fd.restype = None
        lib.mjpc_dc_cost.argtypes = [C.c_void_p, C.c_void_p, _dp, C.c_int, _dp, _dp, _dp, _ip]
        lib.mjpc_dc_cost_derivatives.argtypes = [C.c_void_p, C.c_void_p, _dp, _dp, _ip]
        lib.mjpc_dc_outputs.argtypes = [C.c_void_p] + [_dp] * 9; lib.mjpc_dc_outputs.restype = None
        lib.mjpc_cd_create.restype = C.c_void_p
        lib.mjpc_cd_create.argtypes = [C.c_int] * 4
        lib.mjpc_cd_destroy.argtypes = [C.c_void_p]; lib.mjpc_cd_destroy.restype = None
        lib.mjpc_cd_reset.argtypes = [C.c_void_p, C.c_int]; lib.mjpc_cd_reset.restype = None
        lib.mjpc_cd_compute.argtypes = [C.c_void_p, C.c_void_p, _dp, _dp, _dp, C.c_int, C.c_int]
        lib.mjpc_cd_blocks.argtypes = [C.c_void_p, C.c_int] + [_dp] * 6; lib.mjpc_cd_blocks.restype = None
        lib.mjpc_gd_gradient_compute.argtypes = [C.c_int] * 3 + [_dp] * 9
        lib.mjpc_ilqg_bp_create.restype = C.c_void_p
        lib.mjpc_ilqg_bp_create.argtypes = [C.c_int] * 3
        lib.mjpc_ilqg_bp_destroy.argtypes = [C.c_void_p]; lib.mjpc_ilqg_bp_destroy.restype = None
        lib.mjpc_ilqg_bp_reset.argtypes = [C.c_void_p, C.c_int]; lib.mjpc_ilqg_bp_reset.restype = None
        lib.mjpc_ilqg_bp_riccati_host.argtypes = [C.c_void_p, C.c_int] + [_dp] * 9 + [_ip, _dp, _dp, _dp, _ip]; lib.mjpc_ilqg_bp_riccati_host.restype = None
        lib.mjpc_ilqg_bp_riccati.argtypes = [C.c_void_p, C.c_int, C.c_double] + [_dp] * 9 + [_ip, _dp, _dp, _dp]
        lib.mjpc_ilqg_bp_compute.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [_dp] * 9 + [_ip, _dp, _dp, _dp, _ip]
        lib.mjpc_ilqg_bp_compute_fused.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [_dp] * 6 + [C.c_double, C.c_int, _ip, _dp, _dp, _dp, _ip, _ip]
        lib.mjpc_ilqg_bp_blocks.argtypes = [C.c_void_p, C.c_int] + [_dp] * 8; lib.mjpc_ilqg_bp_blocks.restype = None
        lib.mjpc_ilqg_bp_regularization.argtypes = [C.c_void_p, _dp, _dp]; lib.mjpc_ilqg_bp_regularization.restype = None
        lib.mjpc_ilqg_bp_scale_regularization.argtypes = [C.c_void_p] + [C.c_double] * 3; lib.mjpc_ilqg_bp_scale_regularization.restype = None
        lib.mjpc_ilqg_bp_update_regularization.argtypes = [C.c_void_p] + [C.c_double] * 4; lib.mjpc_ilqg_bp_update_regularization.restype = None
        lib.mjpc_ilqg_boxqp.argtypes = [C.c_int] + [_dp] * 6 + [_ip]
        lib.mjpc_ilqg_policy_action.argtypes = [C.c_int] * 5 + [_ip] * 3 + [_dp, C.c_int, C.c_int] + [_dp] * 4 + [C.c_double, _dp, C.c_double, _dp]
        lib.mjpc_ilqg_policy_action.restype = None
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


class InverseDerivatives:
    """DfDq, DfDv, DfDa [T, nv, nv] and DsDq, DsDv, DsDa [T, nr, nv] of the inverse dynamics along a window of T configurations
    (mjpc_hip::InverseDerivatives; Direct::InverseDynamicsDerivatives of the reference): one mjpc_hip_inverse_fd call, then the window's
    ends as the reference keeps them.  At t = 0 (evaluated at zero velocity and acceleration) only the position-stage rows of DsDq, at
    t = T - 1 (zero acceleration) only DsDq and DsDv without their acceleration-stage rows; every other block there is zero.  The row
    stages (0 position, 1 velocity, 2 acceleration) come from the task's residual table; without a table every row counts as
    acceleration stage until set_row_stages."""

    def __init__(self, model: dict, task: dict, T=2):
        nq, nv, na = model["nq"], model["nv"], model["na"]
        self.ds, self.nq, self.nv, self.nu, self.nr = nq + nv + na, nq, nv, model["nu"], task["num_residual"]
        self.T = int(T)
        self.lib = _lib()
        self.h = C.c_void_p(self.lib.mjpc_id_create(self.ds, nq, nv, self.nu, self.nr, self.T))
        self._cm = capi.CModel(model, task)
        self.lib.mjpc_id_row_stages_from_table(self.h, C.byref(self._cm.c_task))      # -1: not a table, the rows stay acceleration stage

    def close(self):
        if getattr(self, "h", None):
            self.lib.mjpc_id_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def row_stages(self):
        st = np.zeros(max(self.nr, 1), np.int32)
        self.lib.mjpc_id_row_stages(self.h, st.ctypes.data_as(_ip))
        return st[:self.nr]

    def set_row_stages(self, stage):
        st = np.ascontiguousarray(stage, dtype=np.int32).reshape(self.nr)
        self.lib.mjpc_id_set_row_stages(self.h, (st if st.size else np.zeros(1, np.int32)).ctypes.data_as(_ip))

    def compute(self, backend: HipBackend, x, u, a, h, tol=1e-6, mode=0, discrete=True, mocap=None, userdata=None):
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, self.ds); T = x.shape[0]
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(T, self.nu); a = np.ascontiguousarray(a, dtype=np.float64).reshape(T, self.nv)
        h = np.ascontiguousarray(h, dtype=np.float64).reshape(T)
        mo, ud, pmo, pud = backend._shared(mocap, userdata)
        rc = self.lib.mjpc_id_compute(self.h, backend.h, _ptr(x), _ptr(u), _ptr(a), _ptr(h), T, float(tol), int(mode), int(bool(discrete)), pmo, pud)
        cplanner._check()
        if rc != 0:
            raise RuntimeError("InverseDerivatives.compute failed: " + self.lib.mjpc_hip_last_error().decode())
        self.T = max(self.T, T)
        nv, nr = self.nv, self.nr
        names = ("DfDq", "DfDv", "DfDa", "DsDq", "DsDv", "DsDa")
        o = {k: np.zeros((T, nv if i < 3 else nr, nv)) for i, k in enumerate(names)}
        o["failure"] = np.zeros(T, np.int32)
        self.lib.mjpc_id_blocks(self.h, T, *[_ptr(o[k]) for k in names], o["failure"].ctypes.data_as(_ip))
        return o


class DirectCost:
    """The direct optimiser's window cost with its gradient [T nv] and Gauss-Newton Hessian in MuJoCo's lower band [T nv, 3 nv]
    (mjpc_hip::DirectCost; Direct::Cost of the reference) from the window's residuals, the six blocks of InverseDerivatives and the velocity
    blocks dv_t/dq_{t-1}, dv_t/dq_t.  assemble runs on the device (mjpc_hip_direct_assemble), assemble_host the same algebra on the host
    with the same bits.  The sensors are runs of rows of the residual: sensor_dim, sensor_stage (0 position, 1 velocity, 2 acceleration),
    sensor_norm (the cost table's norm types), sensor_norm_parameter [num_sensor, 2], noise_sensor; flags: the keywords of
    capi.direct_settings.  set_window / cost / cost_derivatives: the window the object owns, evaluated on the device (mjpc_hip_direct_cost,
    mjpc_hip_direct_cost_derivatives).  The band solve and the optimiser's loop are not part of this package."""

    FLAGS = ("sensor_flag", "force_flag", "time_scaling_sensor", "time_scaling_force", "first_step_position_sensors", "last_step_position_sensors",
             "last_step_velocity_sensors")

    def __init__(self, nv, nr, timestep, sensor_dim, sensor_stage, sensor_norm, sensor_norm_parameter, noise_sensor, noise_process=None,
                 sensor_first_row=0, sensor_mask=None, T=3, **flags):
        self.nv, self.nr, self.T = int(nv), int(nr), int(T)
        self.lib = _lib()
        self.h = C.c_void_p(self.lib.mjpc_dc_create(self.nv, self.nr, self.T))
        i32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.int32).ravel())      # noqa: E731
        f64 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel())      # noqa: E731
        dim, stage, norm, prm, noise = i32(sensor_dim), i32(sensor_stage), i32(sensor_norm), f64(sensor_norm_parameter), f64(noise_sensor)
        self.num_sensor, self.ns = int(dim.size), int(dim.sum())
        ip = lambda a: (a if a.size else np.zeros(1, np.int32)).ctypes.data_as(_ip)      # noqa: E731
        self.lib.mjpc_dc_set_sensors(self.h, int(sensor_first_row), self.num_sensor, ip(dim), ip(stage), ip(norm), _ptr(prm), _ptr(noise))
        if noise_process is not None:
            self.lib.mjpc_dc_set_process_noise(self.h, _ptr(f64(noise_process).reshape(self.nv)))
        if sensor_mask is not None:
            mk = i32(sensor_mask)
            self.lib.mjpc_dc_set_mask(self.h, ip(mk), mk.size // max(self.num_sensor, 1))
        defaults = dict(zip(self.FLAGS, (1, 1, 1, 1, 1, 0, 0)))
        unknown = set(flags) - set(defaults)
        if unknown:
            raise TypeError(f"DirectCost: unknown settings {sorted(unknown)}")
        defaults.update({k: int(bool(v)) for k, v in flags.items()})
        self.lib.mjpc_dc_set_settings(self.h, i32([defaults[k] for k in self.FLAGS]).ctypes.data_as(_ip), float(timestep))

    def close(self):
        if getattr(self, "h", None):
            self.lib.mjpc_dc_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _run(self, engine, residual_sensor, residual_force, DfDq, DfDv, DfDa, DsDq, DsDv, DsDa, dvdq0, dvdq1):
        nv, nr, ns = self.nv, self.nr, self.ns
        f64 = lambda a, *shape: np.ascontiguousarray(a, dtype=np.float64).reshape(*shape)      # noqa: E731
        DfDq = f64(DfDq, -1, nv, nv); T = DfDq.shape[0]
        ins = [f64(residual_sensor, T, ns), f64(residual_force, T, nv), DfDq, f64(DfDv, T, nv, nv), f64(DfDa, T, nv, nv), f64(DsDq, T, nr, nv),
               f64(DsDv, T, nr, nv), f64(DsDa, T, nr, nv), f64(dvdq0, T, nv, nv), f64(dvdq1, T, nv, nv)]
        rc = self.lib.mjpc_dc_assemble(self.h, engine, T, *[_ptr(a) for a in ins])
        cplanner._check()
        if rc != 0:
            raise RuntimeError("DirectCost.assemble failed: " + self.lib.mjpc_hip_last_error().decode())
        return self._outputs(T)

    def _outputs(self, T):
        nv, ns = self.nv, self.ns
        o = dict(cost=np.zeros(3), gradient=np.zeros(T * nv), hessian_band=np.zeros((T * nv, 3 * nv)), block_sensor=np.zeros((T, ns, 3 * nv)),
                 block_force=np.zeros((T, nv, 3 * nv)), norm_gradient_sensor=np.zeros((T, ns)), norm_gradient_force=np.zeros((T, nv)),
                 residual_sensor=np.zeros((T, ns)), residual_force=np.zeros((T, nv)))
        self.lib.mjpc_dc_outputs(self.h, *[_ptr(a) if a.size else None for a in o.values()])
        return o

    def set_window(self, model, q, act=None, ctrl=None, time=None, sensor_measurement=None, force_measurement=None, tol=1e-6, mode=0, discrete=True):
        """the window the object owns: q [T, nq] and, where given, act [T, na], ctrl [T, nu], time [T], sensor_measurement [T, ns],
        force_measurement [T, nv] (None: zeros); tol, mode, discrete: the finite differences of cost_derivatives and mjENBL_INVDISCRETE"""
        nq, na, nu = model["nq"], model["na"], model["nu"]
        q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, nq); T = self.window_T = q.shape[0]
        self.nq = nq
        arr = lambda a, n: None if a is None or n == 0 else np.ascontiguousarray(a, dtype=np.float64).reshape(T, n)      # noqa: E731
        ins = [q, arr(act, na), arr(ctrl, nu), arr(time, 1), arr(sensor_measurement, self.ns), arr(force_measurement, self.nv)]
        self.lib.mjpc_dc_set_window(self.h, T, nq, na, nu, *[None if a is None else _ptr(a) for a in ins])
        self.lib.mjpc_dc_set_fd(self.h, float(tol), int(mode), int(bool(discrete)))

    def cost(self, backend: HipBackend, q_windows=None, mocap=None, userdata=None):
        """DirectCost::Cost: the costs [nwin, 3] (cost, cost_sensor, cost_force) of candidate windows q_windows [nwin, T, nq] (None: the window
        itself) in one device call, and failure [nwin, T]"""
        T = self.window_T
        qw = None if q_windows is None else np.ascontiguousarray(q_windows, dtype=np.float64).reshape(-1, T, self.nq)
        W = 1 if qw is None else qw.shape[0]
        costs = np.zeros((W, 3)); fail = np.zeros((W, T), np.int32)
        mo, ud, pmo, pud = backend._shared(mocap, userdata)
        rc = self.lib.mjpc_dc_cost(self.h, backend.h, None if qw is None else _ptr(qw), W, pmo, pud, _ptr(costs), fail.ctypes.data_as(_ip))
        cplanner._check()
        if rc != 0:
            raise RuntimeError("DirectCost.cost failed: " + self.lib.mjpc_hip_last_error().decode())
        return dict(cost=costs, failure=fail)

    def cost_derivatives(self, backend: HipBackend, mocap=None, userdata=None):
        """DirectCost::CostDerivatives: the window's cost, gradient, band Hessian and blocks in one device call -> the dict of assemble plus
        failure [T]"""
        T = self.window_T
        fail = np.zeros(T, np.int32)
        mo, ud, pmo, pud = backend._shared(mocap, userdata)
        rc = self.lib.mjpc_dc_cost_derivatives(self.h, backend.h, pmo, pud, fail.ctypes.data_as(_ip))
        cplanner._check()
        if rc != 0:
            raise RuntimeError("DirectCost.cost_derivatives failed: " + self.lib.mjpc_hip_last_error().decode())
        o = self._outputs(T)
        o["failure"] = fail
        return o

    def assemble(self, backend: HipBackend, *arrays):
        """(residual_sensor [T, ns], residual_force [T, nv], DfDq, DfDv, DfDa [T, nv, nv], DsDq, DsDv, DsDa [T, nr, nv], dvdq0, dvdq1 [T, nv, nv])
        -> dict(cost [3], gradient, hessian_band, block_sensor, block_force, norm_gradient_sensor, norm_gradient_force, residual_sensor,
        residual_force), on the device"""
        return self._run(backend.h, *arrays)

    def assemble_host(self, *arrays):
        """assemble on the host (no GPU), bit-equal to the device"""
        return self._run(None, *arrays)


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


def boxqp(H, g, lower=None, upper=None, warm=None):
    """BoxQPSolve on the host (no GPU): minimise 0.5 x'Hx + g'x over lower <= x <= upper by projected Newton steps (csrc/riccati.h has the
    definition) from `warm` (zeros) clamped into the box -> dict(nfree (-1: H not positive definite on the free set), x [n], index [nfree]
    the free dimensions ascending, R [nfree, nfree] the lower Cholesky factor of H[index][:, index])."""
    H = np.ascontiguousarray(H, dtype=np.float64); n = H.shape[0]
    g = np.ascontiguousarray(g, dtype=np.float64).reshape(n)
    lo = None if lower is None else np.ascontiguousarray(lower, dtype=np.float64).reshape(n)
    hi = None if upper is None else np.ascontiguousarray(upper, dtype=np.float64).reshape(n)
    x = np.zeros(n) if warm is None else np.array(warm, dtype=np.float64).reshape(n)
    R = np.zeros(n * n); index = np.zeros(max(n, 1), np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(_dp)      # noqa: E731
    nf = _lib().mjpc_ilqg_boxqp(n, p(H), p(g), p(lo), p(hi), p(x), p(R), index.ctypes.data_as(_ip))
    k = max(nf, 0)
    return dict(nfree=int(nf), x=x, index=index[:k].copy(), R=R[:k * k].reshape(k, k).copy())


def ilqg_policy_action(model, times, states, actions, feedback_gain, time, state=None, representation=1, feedback_scaling=1.0):
    """iLQGPolicy::Action on the host (no GPU): the nominal action interpolated at `time` (0 zero-order, 1 linear, 2 cubic), plus
    feedback_scaling * K (state (-) nominal state) when a state is given, clamped to the ctrlrange.  times [H], states [H, nq+nv+na],
    actions [H, nu], feedback_gain [H, nu, 2nv+na]."""
    nq, nv, na, nu, njnt = (int(model[k]) for k in ("nq", "nv", "na", "nu", "njnt"))
    ints = [np.ascontiguousarray(np.asarray(model[k], dtype=np.int32).reshape(-1)) for k in ("jnt_type", "jnt_qposadr", "jnt_dofadr")]
    ints = [a if a.size else np.zeros(1, np.int32) for a in ints]
    rng = np.ascontiguousarray(np.asarray(model["actuator_ctrlrange"], dtype=np.float64).reshape(-1))
    t = np.ascontiguousarray(times, dtype=np.float64).reshape(-1); H = t.size
    xs = np.ascontiguousarray(states, dtype=np.float64).reshape(H, nq + nv + na); us = np.ascontiguousarray(actions, dtype=np.float64).reshape(H, nu)
    K = np.ascontiguousarray(feedback_gain, dtype=np.float64).reshape(H, nu * (2 * nv + na))
    st = None if state is None else np.ascontiguousarray(state, dtype=np.float64).reshape(nq + nv + na)
    out = np.zeros(nu)
    _lib().mjpc_ilqg_policy_action(nq, nv, na, nu, njnt, *[a.ctypes.data_as(_ip) for a in ints], _ptr(rng), int(representation), H, _ptr(t), _ptr(xs),
                                   _ptr(us), _ptr(K), float(feedback_scaling), None if st is None else _ptr(st), float(time), _ptr(out))
    cplanner._check()
    return out


class ILQGBackwardPass:
    """mjpc_hip::iLQGBackwardPass with its BoxQP: the backward pass of iLQG over given model and cost derivatives, on the host
    (riccati_host, riccati: no GPU) or on the device (compute, compute_fused), bit-equal to each other.  Arrays as
    HipBackend.ilqg_backward_pass; the results are dicts like its."""

    def __init__(self, nd, nu, T=2):
        self.nd, self.nu, self.T = int(nd), int(nu), int(T)
        self.lib = _lib()
        self.h = C.c_void_p(self.lib.mjpc_ilqg_bp_create(self.nd, self.nu, self.T))

    def close(self):
        if getattr(self, "h", None):
            self.lib.mjpc_ilqg_bp_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, T=None):
        self.lib.mjpc_ilqg_bp_reset(self.h, int(self.T if T is None else T))

    @property
    def regularization(self):
        """(regularization, regularization_rate, regularization_factor)"""
        o = np.zeros(3)
        self.lib.mjpc_ilqg_bp_regularization(self.h, None, _ptr(o))
        return tuple(float(v) for v in o)

    @regularization.setter
    def regularization(self, v):
        s = np.array(v, dtype=np.float64).reshape(3)
        self.lib.mjpc_ilqg_bp_regularization(self.h, _ptr(s), None)

    def scale_regularization(self, factor, reg_min=1.0e-6, reg_max=1.0e6):
        self.lib.mjpc_ilqg_bp_scale_regularization(self.h, float(factor), float(reg_min), float(reg_max))
        return self.regularization

    def update_regularization(self, z, s, reg_min=1.0e-6, reg_max=1.0e6):
        self.lib.mjpc_ilqg_bp_update_regularization(self.h, float(reg_min), float(reg_max), float(z), float(s))
        return self.regularization

    def _args(self, A, B, cx, cu, cxx, cxu, cuu, actions, action_limits, regularization_type, action_limits_on, max_regularization_iterations,
              min_regularization, max_regularization):
        cx = np.ascontiguousarray(cx, dtype=np.float64).reshape(-1, self.nd); T = cx.shape[0]
        nd, nu = self.nd, self.nu
        need = dict(A=(T - 1) * nd * nd, B=(T - 1) * nd * nu, cu=T * nu, cxx=T * nd * nd, cxu=T * nd * nu, cuu=T * nu * nu)
        arrs = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (A, B, cx, cu, cxx, cxu, cuu)]
        for a, name in zip(arrs, ("A", "B", "cx", "cu", "cxx", "cxu", "cuu")):
            if name in need and a.size < need[name]:
                raise ValueError(f"ILQGBackwardPass: {name} holds {a.size} numbers, {need[name]} are needed")
        if action_limits_on and (actions is None or action_limits is None):
            raise ValueError("ILQGBackwardPass: actions and action_limits are needed with action_limits = 1")
        act = None if actions is None else np.ascontiguousarray(actions, dtype=np.float64).reshape(-1)
        lim = None if action_limits is None else np.ascontiguousarray(action_limits, dtype=np.float64).reshape(-1)
        si = np.array([regularization_type, action_limits_on, max_regularization_iterations], np.int32)
        sd = np.array([min_regularization, max_regularization], np.float64)
        self.T = max(self.T, T)
        return T, arrs, act, lim, si, sd

    def _result(self, T, k, K, status):
        nd, nu = self.nd, self.nu
        o = dict(k=k, K=K, Vx=np.zeros((T, nd)), Vxx=np.zeros((T, nd, nd)), Qx=np.zeros((T - 1, nd)), Qu=np.zeros((T - 1, nu)), Qxx=np.zeros((T - 1, nd, nd)),
                 Qxu=np.zeros((T - 1, nd, nu)), Quu=np.zeros((T - 1, nu, nu)), dV=np.zeros(2))
        self.lib.mjpc_ilqg_bp_blocks(self.h, T, *[_ptr(o[n_]) for n_ in ("Vx", "Vxx", "Qx", "Qu", "Qxx", "Qxu", "Quu", "dV")])
        reg = self.regularization
        o["status"] = status; o["regularization"] = reg[0]; o["regularization_rate"] = reg[1]
        return o

    def _run(self, fn, head, A, B, cx, cu, cxx, cxu, cuu, actions, action_limits, regularization_type, action_limits_on, max_regularization_iterations,
             min_regularization, max_regularization, fill, with_status=True):
        T, arrs, act, lim, si, sd = self._args(A, B, cx, cu, cxx, cxu, cuu, actions, action_limits, regularization_type, action_limits_on,
                                               max_regularization_iterations, min_regularization, max_regularization)
        k = np.full((T, self.nu), float(fill)); K = np.full((T, self.nu, self.nd), float(fill)); st = np.zeros(3, np.int32)
        p = lambda a: None if a is None else _ptr(a)      # noqa: E731
        tail = [st.ctypes.data_as(_ip)] if with_status else []
        rc = fn(self.h, *head(T), *[_ptr(a) for a in arrs], p(act), p(lim), si.ctypes.data_as(_ip), _ptr(sd), _ptr(k), _ptr(K), *tail)
        cplanner._check()
        return T, k, K, st, rc

    def riccati_host(self, A, B, cx, cu, cxx, cxu, cuu, actions=None, action_limits=None, regularization_type=0, action_limits_on=1,
                     max_regularization_iterations=5, min_regularization=1.0e-6, max_regularization=1.0e6, fill=0.0):
        """the regularisation loop on the host (no GPU), from this object's regularization / rate / factor"""
        T, k, K, st, _ = self._run(self.lib.mjpc_ilqg_bp_riccati_host, lambda T: (T,), A, B, cx, cu, cxx, cxu, cuu, actions, action_limits, regularization_type,
                                   action_limits_on, max_regularization_iterations, min_regularization, max_regularization, fill)
        return self._result(T, k, K, st)

    def riccati(self, reg, A, B, cx, cu, cxx, cxu, cuu, actions=None, action_limits=None, regularization_type=0, action_limits_on=1,
                max_regularization_iterations=5, min_regularization=1.0e-6, max_regularization=1.0e6, fill=0.0):
        """iLQGBackwardPass::Riccati as the reference calls it: every sweep uses `reg`; status[0] is its return value (0 = complete, else
        the failing time index).  The box-QP's warm start is the object's (zero after reset())."""
        T, k, K, st, rc = self._run(self.lib.mjpc_ilqg_bp_riccati, lambda T: (T, float(reg)), A, B, cx, cu, cxx, cxu, cuu, actions, action_limits,
                                    regularization_type, action_limits_on, max_regularization_iterations, min_regularization, max_regularization, fill,
                                    with_status=False)
        o = self._result(T, k, K, st)
        o["status"] = int(rc)
        return o

    def compute(self, backend: HipBackend, A, B, cx, cu, cxx, cxu, cuu, actions=None, action_limits=None, regularization_type=0, action_limits_on=1,
                max_regularization_iterations=5, min_regularization=1.0e-6, max_regularization=1.0e6, fill=0.0):
        """the same on the device (mjpc_hip_ilqg_backward_pass)"""
        T, k, K, st, rc = self._run(self.lib.mjpc_ilqg_bp_compute, lambda T: (backend.h, T), A, B, cx, cu, cxx, cxu, cuu, actions, action_limits,
                                    regularization_type, action_limits_on, max_regularization_iterations, min_regularization, max_regularization, fill)
        if rc != 0:
            raise RuntimeError("ILQGBackwardPass.compute failed: " + self.lib.mjpc_hip_last_error().decode())
        return self._result(T, k, K, st)

    def compute_fused(self, backend: HipBackend, x, u, h, residual, mocap=None, userdata=None, tol=1e-6, mode=0, regularization_type=0,
                      action_limits_on=1, max_regularization_iterations=5, min_regularization=1.0e-6, max_regularization=1.0e6):
        """derivatives and backward pass in one device call (mjpc_hip_trajectory_ilqg); the object's dimensions must be the backend's model's"""
        ds, nd, nu, nr = backend._dims()
        if (nd, nu) != (self.nd, self.nu):
            raise ValueError("ILQGBackwardPass.compute_fused: the object's dimensions are not the model's")
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, ds); T = x.shape[0]
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(T, nu); h = np.ascontiguousarray(h, dtype=np.float64).reshape(T)
        r = np.ascontiguousarray(residual, dtype=np.float64).reshape(T, nr)
        mo, ud, pmo, pud = backend._shared(mocap, userdata)
        si = np.array([regularization_type, action_limits_on, max_regularization_iterations], np.int32)
        sd = np.array([min_regularization, max_regularization], np.float64)
        k = np.zeros((max(T, 1), nu)); K = np.zeros((max(T, 1), nu, nd)); st = np.zeros(3, np.int32); fail = np.zeros(max(T, 1), np.int32)
        rc = self.lib.mjpc_ilqg_bp_compute_fused(self.h, backend.h, T, _ptr(x), _ptr(u), _ptr(h), _ptr(r), pmo, pud, float(tol), int(mode), si.ctypes.data_as(_ip),
                                                 _ptr(sd), _ptr(k), _ptr(K), st.ctypes.data_as(_ip), fail.ctypes.data_as(_ip))
        cplanner._check()
        if rc != 0:
            raise RuntimeError("ILQGBackwardPass.compute_fused failed: " + self.lib.mjpc_hip_last_error().decode())
        self.T = max(self.T, T)
        o = self._result(T, k, K, st)
        o["failure"] = fail[:T]
        return o
