"""ctypes wrappers of the rollout engine's C ABI (include/mjpc_hip.h): `HipBackend` = one engine (mjpc_hip_plan and friends),
`HipMultiBackend` = one planner process with one engine per GPU (mjpc_hip_multi_*).

The rollouts of mjpc/planners/sampling/planner.cc:342-380 run on the GPU behind that ABI; the host logic of the reference's
SamplingPlanner lives in C++ (csrc/planner.cc, driven from Python through cplanner.py).  There is no CPU fallback: a missing
libmjpc_hip.so raises in capi.load_engine().  (The Python restatement of the host logic that the tests cross-check the C++ planner
against is test infrastructure: tests/host_mirror.py.)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

kZeroSpline, kLinearSpline, kCubicSpline = 0, 1, 2
kMaxTrajectoryHorizon = 512          # mjpc/trajectory.h:27
kMaxTrajectoryReference = 128        # mjpc/planners/planner.h:28 (lifted here)


class HipBackend:
    """Thin object wrapper over the C ABI (include/mjpc_hip.h)."""

    def __init__(self, model: dict, task: dict, max_samples=128, max_horizon=kMaxTrajectoryHorizon, device=0):
        self.lib = capi.load_engine()
        self.cm = capi.CModel(model, task)
        self.model = model; self.task = task
        self.h = self.lib.mjpc_hip_create(C.byref(self.cm.c_model), C.byref(self.cm.c_task), int(max_samples),
                                          int(max_horizon), int(device))
        if not self.h:
            raise RuntimeError("mjpc_hip_create failed: " + self.lib.mjpc_hip_last_error().decode())
        self.max_samples = max_samples

    def close(self):
        if getattr(self, "h", None):
            self.lib.mjpc_hip_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_task(self, task: dict):
        self.task = task
        t = self.cm.make_task(task)
        if self.lib.mjpc_hip_set_task(self.h, C.byref(t)) != 0:
            raise RuntimeError(self.lib.mjpc_hip_last_error().decode())

    def set_fetch_mode(self, summary_only: bool):
        """summary_only: plan() brings back returns / failure flags / local elite (index, return, knots) only; the winner's
        trajectory rows stay on the device until candidate() asks for them (shards of a multi-GPU plan)."""
        if self.lib.mjpc_hip_set_fetch_mode(self.h, 1 if summary_only else 0) != 0:
            raise RuntimeError(self.lib.mjpc_hip_last_error().decode())

    def _alloc_out(self, nl, H, P):
        m, t = self.model, self.task
        ds = m["nq"] + m["nv"] + m["na"]; nu = m["nu"]; nr = t["num_residual"]; ntr = 3 * t["num_trace"]
        o = dict(returns=np.zeros(nl), failure=np.zeros(nl, np.int32), states=np.zeros((H, ds)), actions=np.zeros((H, nu)),
                 times=np.zeros(H), residual=np.zeros((H, nr)), costs=np.zeros(H), trace=np.zeros((H, max(ntr, 1))),
                 winner_knots=np.zeros((P, nu)))
        c = capi.MjpcHipPlanOutput()
        for k in ["returns", "states", "actions", "times", "residual", "costs", "trace", "winner_knots"]:
            setattr(c, k, o[k].ctypes.data_as(capi.c_double_p))
        c.failure = o["failure"].ctypes.data_as(capi.c_int_p)
        return o, c, ntr

    def make_input(self, **kw):
        return capi.make_plan_input(self.cm, **kw)

    def plan(self, **kw):
        inp = self.make_input(**kw)
        return self.plan_input(inp)

    def plan_input(self, inp):
        o, c, ntr = self._alloc_out(inp.num_local, inp.horizon, inp.num_spline_points)
        rc = self.lib.mjpc_hip_plan(self.h, C.byref(inp), C.byref(c))
        if rc != 0:
            raise RuntimeError("mjpc_hip_plan failed: " + self.lib.mjpc_hip_last_error().decode())
        o["winner"] = c.winner; o["winner_return"] = c.winner_return
        o["noise_compute_time_us"] = c.noise_compute_time_us; o["rollouts_compute_time_us"] = c.rollouts_compute_time_us
        o["trace"] = o["trace"][:, :ntr]
        return o

    def plan_async(self, inp):
        if self.lib.mjpc_hip_plan_async(self.h, C.byref(inp)) != 0:
            raise RuntimeError("mjpc_hip_plan_async failed: " + self.lib.mjpc_hip_last_error().decode())

    def plan_fetch(self, inp):
        o, c, ntr = self._alloc_out(inp.num_local, inp.horizon, inp.num_spline_points)
        if self.lib.mjpc_hip_plan_fetch(self.h, C.byref(c)) != 0:
            raise RuntimeError("mjpc_hip_plan_fetch failed: " + self.lib.mjpc_hip_last_error().decode())
        o["winner"] = c.winner; o["winner_return"] = c.winner_return
        o["trace"] = o["trace"][:, :ntr]
        return o

    def plan_mixed(self, first_explicit, **kw):
        """Sample-Gradient batch (mjpc_hip_plan_mixed): candidates with global index < first_explicit are sampled with the
        required noise_std (the nominal_index one un-noised), the others use candidate_knots[i] verbatim; noisy rows leave
        their standard normals in the engine's noise history."""
        inp = self.make_input(**kw)
        o, c, ntr = self._alloc_out(inp.num_local, inp.horizon, inp.num_spline_points)
        if self.lib.mjpc_hip_plan_mixed(self.h, C.byref(inp), int(first_explicit), C.byref(c)) != 0:
            raise RuntimeError("mjpc_hip_plan_mixed failed: " + self.lib.mjpc_hip_last_error().decode())
        o["winner"] = c.winner; o["winner_return"] = c.winner_return
        o["noise_compute_time_us"] = c.noise_compute_time_us; o["rollouts_compute_time_us"] = c.rollouts_compute_time_us
        o["trace"] = o["trace"][:, :ntr]
        self._last_PN = inp.num_spline_points * self.model["nu"]
        return o

    def plan_feedback(self, state, time, horizon, times, states, actions, feedback_gain, action_step, feedback_scaling, action_improvement=None,
                      mode=capi.FEEDBACK_INDEXED, representation=1, use_feedback=True, mocap=None, userdata=None, candidate_offset=0):
        """Rollouts under a feedback policy (mjpc_hip_plan_feedback): candidate i applies
        clamp((actions[t] + action_step[i] * action_improvement[t]) + feedback_scaling[i] * (feedback_gain[t] * StateDiff(states[t], x_t)))
        with the tables indexed by the step (FEEDBACK_INDEXED) or interpolated at the step's time (FEEDBACK_TIME).  The winner's
        rows come back as after plan(); fetch_all(N, H, 0) gives every candidate's."""
        N = int(len(np.asarray(action_step).ravel()))
        inp = self.make_input(state=state, mocap=mocap, time=time, knot_times=np.zeros(1), knot_values=np.zeros(self.model["nu"]), interpolation=0,
                              num_trajectory=N, horizon=horizon, userdata=userdata, candidate_offset=candidate_offset,
                              num_local=N - int(candidate_offset))
        pol = capi.make_feedback_policy(times, states, actions, feedback_gain, action_step, feedback_scaling, action_improvement=action_improvement,
                                        mode=mode, representation=representation, use_feedback=use_feedback)
        o, c, ntr = self._alloc_out(max(N - int(candidate_offset), 1), horizon, 1)
        if self.lib.mjpc_hip_plan_feedback(self.h, C.byref(inp), C.byref(pol), C.byref(c)) != 0:
            raise RuntimeError("mjpc_hip_plan_feedback failed: " + self.lib.mjpc_hip_last_error().decode())
        o["winner"] = c.winner; o["winner_return"] = c.winner_return
        o["rollouts_compute_time_us"] = c.rollouts_compute_time_us
        o["resample_time_us"] = self.lib.mjpc_hip_feedback_resample_time_us(self.h)
        o["trace"] = o["trace"][:, :ntr]
        del o["winner_knots"]
        return o

    def sample_gradient(self, slot, scale):
        """gradient[k] = sum_i history[slot[i]][k] * scale[i] over the noise history, k < P * nu of the last plan
        (mjpc_hip_sample_gradient): products rounded, added in ascending i."""
        sl = np.ascontiguousarray(slot, dtype=np.int32); sc = np.ascontiguousarray(scale, dtype=np.float64)
        if sl.shape != sc.shape or sl.ndim != 1:
            raise ValueError("sample_gradient: slot and scale must be 1-d and of equal length")
        g = np.zeros(36 * self.model["nu"])
        if self.lib.mjpc_hip_sample_gradient(self.h, int(sl.size), sl.ctypes.data_as(capi.c_int_p), sc.ctypes.data_as(capi.c_double_p),
                                             g.ctypes.data_as(capi.c_double_p)) != 0:
            raise RuntimeError("mjpc_hip_sample_gradient failed: " + self.lib.mjpc_hip_last_error().decode())
        return g[:getattr(self, "_last_PN", g.size)]

    def noise_history_reset(self):
        if self.lib.mjpc_hip_noise_history_reset(self.h) != 0:
            raise RuntimeError(self.lib.mjpc_hip_last_error().decode())

    def _dims(self):
        m = self.model
        nq, nv, na, nu = m["nq"], m["nv"], m["na"], m["nu"]
        return nq + nv + na, 2 * nv + na, nu, self.task["num_residual"]

    def _shared(self, mocap, userdata):
        mo = np.ascontiguousarray(np.zeros(7 * self.model["nmocap"]) if mocap is None else mocap, dtype=np.float64).ravel()
        if mo.size != 7 * self.model["nmocap"]:
            raise ValueError("mocap must hold 7 numbers per mocap body")
        ud = None if userdata is None else np.ascontiguousarray(userdata, dtype=np.float64).ravel()
        dp = capi.c_double_p
        return mo, ud, (mo.ctypes.data_as(dp) if mo.size else None), (ud.ctypes.data_as(dp) if ud is not None and ud.size else None)

    def step_batch(self, states, ctrl, time, mocap=None, userdata=None):
        """One step from each of n different states (mjpc_hip_step_batch): states [n, nq+nv+na], ctrl [n, nu], time [n] ->
        dict(next_states [n, ds], residual [n, nr] evaluated inside the step, failure [n] MJPC_WARN_* bits).  Row i is bit for bit the
        first step of plan(N=1, H=2, P=1, candidate_knots=ctrl[i]) from states[i]."""
        ds, _, nu, nr = self._dims()
        x = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, ds); n = x.shape[0]
        u = np.ascontiguousarray(ctrl, dtype=np.float64).reshape(n, nu); t = np.ascontiguousarray(time, dtype=np.float64).reshape(n)
        mo, ud, pmo, pud = self._shared(mocap, userdata)
        o = dict(next_states=np.zeros((n, ds)), residual=np.zeros((n, nr)), failure=np.zeros(n, np.int32))
        dp = capi.c_double_p
        u_ = u if u.size else np.zeros(1); r_ = o["residual"] if nr else np.zeros(1)
        rc = self.lib.mjpc_hip_step_batch(self.h, n, x.ctypes.data_as(dp), u_.ctypes.data_as(dp), t.ctypes.data_as(dp), pmo, pud,
                                          o["next_states"].ctypes.data_as(dp), r_.ctypes.data_as(dp), o["failure"].ctypes.data_as(capi.c_int_p))
        if rc != 0:
            raise RuntimeError("mjpc_hip_step_batch failed: " + self.lib.mjpc_hip_last_error().decode())
        return o

    def transition_fd(self, x, u, time, mocap=None, userdata=None, eps=1e-6, centered=False, last_is_terminal=False, fill=0.0):
        """Finite-difference transition derivatives at T knots (mjpc_hip_transition_fd): dict(A [T, nd, nd], B [T, nd, nu], C [T, nr, nd],
        D [T, nr, nu], failure [T]), nd = 2 nv + na.  With last_is_terminal the last knot's A / B / D are not written: they keep `fill`."""
        ds, nd, nu, nr = self._dims()
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, ds); T = x.shape[0]
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(T, nu); t = np.ascontiguousarray(time, dtype=np.float64).reshape(T)
        mo, ud, pmo, pud = self._shared(mocap, userdata)
        o = dict(A=np.full((T, nd, nd), float(fill)), B=np.full((T, nd, nu), float(fill)), C=np.full((T, nr, nd), float(fill)),
                 D=np.full((T, nr, nu), float(fill)), failure=np.zeros(T, np.int32))
        dp = capi.c_double_p
        ptr = lambda a: (a if a.size else np.zeros(1)).ctypes.data_as(dp)      # noqa: E731
        rc = self.lib.mjpc_hip_transition_fd(self.h, T, x.ctypes.data_as(dp), ptr(u), t.ctypes.data_as(dp), pmo, pud, float(eps), int(bool(centered)),
                                             int(bool(last_is_terminal)), ptr(o["A"]), ptr(o["B"]), ptr(o["C"]), ptr(o["D"]),
                                             o["failure"].ctypes.data_as(capi.c_int_p))
        if rc != 0:
            raise RuntimeError("mjpc_hip_transition_fd failed: " + self.lib.mjpc_hip_last_error().decode())
        return o

    def inverse_batch(self, states, ctrl, qacc, time, mocap=None, userdata=None, discrete=False, fill=0.0):
        """One inverse-dynamics evaluation at each of n configurations (mjpc_hip_inverse_batch): states [n, nq+nv+na], ctrl [n, nu],
        qacc [n, nv], time [n] -> dict(qfrc_inverse [n, nv], qfrc_constraint [n, nv], residual [n, nr] with the late rows at the given
        acceleration, failure [n] MJPC_WARN_* bits).  discrete: qacc is a step's (v' - v) / timestep.  A refused call (discrete on a
        model with a dense implicit integrator) raises and writes nothing: the outputs would have kept `fill`."""
        ds, _, nu, nr = self._dims()
        nv = self.model["nv"]
        x = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, ds); n = x.shape[0]
        u = np.ascontiguousarray(ctrl, dtype=np.float64).reshape(n, nu); t = np.ascontiguousarray(time, dtype=np.float64).reshape(n)
        a = np.ascontiguousarray(qacc, dtype=np.float64).reshape(n, nv)
        mo, ud, pmo, pud = self._shared(mocap, userdata)
        o = dict(qfrc_inverse=np.full((n, nv), float(fill)), qfrc_constraint=np.full((n, nv), float(fill)), residual=np.full((n, nr), float(fill)),
                 failure=np.zeros(n, np.int32))
        dp = capi.c_double_p
        ptr = lambda v: (v if v.size else np.zeros(1)).ctypes.data_as(dp)      # noqa: E731
        rc = self.lib.mjpc_hip_inverse_batch(self.h, n, ptr(x), ptr(u), ptr(a), ptr(t), pmo, pud, int(bool(discrete)), ptr(o["qfrc_inverse"]),
                                             ptr(o["qfrc_constraint"]), ptr(o["residual"]), o["failure"].ctypes.data_as(capi.c_int_p))
        if rc != 0:
            raise RuntimeError("mjpc_hip_inverse_batch failed: " + self.lib.mjpc_hip_last_error().decode())
        return o

    def inverse_fd(self, x, u, qacc, time, mocap=None, userdata=None, discrete=False, eps=1e-6, centered=False, want=(1,) * 6, fill=0.0):
        """Finite-difference derivatives of the inverse dynamics at T configurations (mjpc_hip_inverse_fd): dict(DfDq, DfDv, DfDa
        [T, nv, nv], DsDq, DsDv, DsDa [T, nr, nv], failure [T]), entry [i][j] = d out_i / d in_j.  want: which of the six blocks are
        asked for, in that order (the others are not computed and come back as None)."""
        ds, _, nu, nr = self._dims()
        nv = self.model["nv"]
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, ds); T = x.shape[0]
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(T, nu); t = np.ascontiguousarray(time, dtype=np.float64).reshape(T)
        a = np.ascontiguousarray(qacc, dtype=np.float64).reshape(T, nv)
        mo, ud, pmo, pud = self._shared(mocap, userdata)
        names = ["DfDq", "DfDv", "DfDa", "DsDq", "DsDv", "DsDa"]
        o = {k: (np.full((T, nv if i < 3 else nr, nv), float(fill)) if want[i] else None) for i, k in enumerate(names)}
        o["failure"] = np.zeros(T, np.int32)
        dp = capi.c_double_p
        ptr = lambda v: None if v is None else (v if v.size else np.zeros(1)).ctypes.data_as(dp)      # noqa: E731
        rc = self.lib.mjpc_hip_inverse_fd(self.h, T, ptr(x), ptr(u), ptr(a), ptr(t), pmo, pud, int(bool(discrete)), float(eps), int(bool(centered)),
                                          *[ptr(o[k]) for k in names], o["failure"].ctypes.data_as(capi.c_int_p))
        if rc != 0:
            raise RuntimeError("mjpc_hip_inverse_fd failed: " + self.lib.mjpc_hip_last_error().decode())
        return o

    def unscented_moments(self, state, factor, sigma_step, weights, ctrl, time, noise_process, noise_sensor, sensor_first_row=0, num_sensor=None,
                          mocap=None, userdata=None, sigma_next=True):
        """The device half of an unscented filter update (mjpc_hip_unscented_moments): the 2nd+1 sigma points around `state` from the lower
        Cholesky factor [nd, nd], one step of each, and dict(state_mean [ds], sensor_mean [ns], cov_ss [nd, nd], cov_sy [nd, ns],
        cov_yy [ns, ns], sigma_next [2nd+1, ds] or None, failure: OR of the rows' MJPC_WARN_* bits).  weights = (mean0, cov0, sigma); the
        measurement is residual rows [sensor_first_row, sensor_first_row + num_sensor) (default: all rows from sensor_first_row)."""
        ds, nd, nu, nr = self._dims()
        ns = nr - int(sensor_first_row) if num_sensor is None else int(num_sensor)
        arr = lambda a, n: np.ascontiguousarray(a, dtype=np.float64).reshape(n)      # noqa: E731
        x = arr(state, ds); L = arr(factor, (nd, nd)); w = arr(weights, 3); u = arr(ctrl, nu) if nu else np.zeros(1)
        qp = arr(noise_process, nd); qs = arr(noise_sensor, max(ns, 0))
        mo, ud, pmo, pud = self._shared(mocap, userdata)
        m = max(ns, 0)
        o = dict(state_mean=np.zeros(ds), sensor_mean=np.zeros(m), cov_ss=np.zeros((nd, nd)), cov_sy=np.zeros((nd, m)), cov_yy=np.zeros((m, m)),
                 sigma_next=np.zeros((2 * nd + 1, ds)) if sigma_next else None)
        fail = np.zeros(1, np.int32)
        dp = capi.c_double_p
        ptr = lambda a: None if a is None else (a if a.size else np.zeros(1)).ctypes.data_as(dp)      # noqa: E731
        rc = self.lib.mjpc_hip_unscented_moments(self.h, ptr(x), ptr(L), float(sigma_step), ptr(w), ptr(u), float(time), pmo, pud, ptr(qp), ptr(qs),
                                                 int(sensor_first_row), ns, ptr(o["state_mean"]), ptr(o["sensor_mean"]), ptr(o["cov_ss"]),
                                                 ptr(o["cov_sy"]), ptr(o["cov_yy"]), ptr(o["sigma_next"]), fail.ctypes.data_as(capi.c_int_p))
        if rc != 0:
            raise RuntimeError("mjpc_hip_unscented_moments failed: " + self.lib.mjpc_hip_last_error().decode())
        o["failure"] = int(fail[0])
        return o

    def linearize_step(self, state, ctrl, time, mocap=None, userdata=None, eps=1e-6, centered=False):
        """One knot's step and its state derivatives (mjpc_hip_linearize_step): dict(next_state [ds], residual [nr], A [nd, nd], C [nr, nd],
        failure).  next_state / residual are step_batch's of the knot, A / C are transition_fd's at T = 1."""
        ds, nd, nu, nr = self._dims()
        x = np.ascontiguousarray(state, dtype=np.float64).reshape(ds)
        u = np.ascontiguousarray(ctrl, dtype=np.float64).reshape(nu) if nu else np.zeros(1)
        mo, ud, pmo, pud = self._shared(mocap, userdata)
        o = dict(next_state=np.zeros(ds), residual=np.zeros(nr), A=np.zeros((nd, nd)), C=np.zeros((nr, nd)))
        fail = np.zeros(1, np.int32)
        dp = capi.c_double_p
        ptr = lambda a: (a if a.size else np.zeros(1)).ctypes.data_as(dp)      # noqa: E731
        rc = self.lib.mjpc_hip_linearize_step(self.h, ptr(x), ptr(u), float(time), pmo, pud, float(eps), int(bool(centered)), ptr(o["next_state"]),
                                              ptr(o["residual"]), ptr(o["A"]), ptr(o["C"]), fail.ctypes.data_as(capi.c_int_p))
        if rc != 0:
            raise RuntimeError("mjpc_hip_linearize_step failed: " + self.lib.mjpc_hip_last_error().decode())
        o["failure"] = int(fail[0])
        return o

    def cost_derivatives(self, residual, C_, D, last_is_terminal=False, hessians=True, fill=0.0):
        """Cost derivatives of T knots from the residual [T, nr] and its Jacobian C [T, nr, nd], D [T, nr, nu] under the engine's current
        cost table and risk (mjpc_hip_cost_derivatives): dict(cr [T, nr], cx [T, nd], cu [T, nu], and with hessians cxx [T, nd, nd],
        cuu [T, nu, nu], cxu [T, nd, nu]).  With last_is_terminal the last knot's D is not read.  `fill`: what an entry the call does
        not write would keep."""
        _, nd, nu, nr = self._dims()
        r = np.ascontiguousarray(residual, dtype=np.float64).reshape(-1, nr) if nr else np.zeros((len(C_), 0)); T = r.shape[0]
        Cm = np.ascontiguousarray(C_, dtype=np.float64).reshape(T, nr, nd); Dm = np.ascontiguousarray(D, dtype=np.float64).reshape(T, nr, nu)
        o = dict(cr=np.full((T, nr), float(fill)), cx=np.full((T, nd), float(fill)), cu=np.full((T, nu), float(fill)))
        if hessians:
            o.update(cxx=np.full((T, nd, nd), float(fill)), cuu=np.full((T, nu, nu), float(fill)), cxu=np.full((T, nd, nu), float(fill)))
        dp = capi.c_double_p
        ptr = lambda a: (a if a.size else np.zeros(1)).ctypes.data_as(dp)      # noqa: E731
        outs = [ptr(o[k]) if k in o else None for k in ("cr", "cx", "cu", "cxx", "cuu", "cxu")]
        rc = self.lib.mjpc_hip_cost_derivatives(self.h, T, ptr(r), ptr(Cm), ptr(Dm), int(bool(last_is_terminal)), int(bool(hessians)), *outs)
        if rc != 0:
            raise RuntimeError("mjpc_hip_cost_derivatives failed: " + self.lib.mjpc_hip_last_error().decode())
        return o

    def trajectory_gradient(self, x, u, time, residual, mocap=None, userdata=None, eps=1e-6, centered=False):
        """One derivative iteration of the gradient planner on the device (mjpc_hip_trajectory_gradient): transition_fd with the last knot
        terminal, cost gradients, backward recursion -> dict(k [T, nu], Vx [T, nd], Qx [T-1, nd], Qu [T-1, nu], dV [2], failure [T])."""
        ds, nd, nu, nr = self._dims()
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, ds); T = x.shape[0]
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(T, nu); t = np.ascontiguousarray(time, dtype=np.float64).reshape(T)
        r = np.ascontiguousarray(residual, dtype=np.float64).reshape(T, nr)
        mo, ud, pmo, pud = self._shared(mocap, userdata)
        o = dict(k=np.zeros((T, nu)), Vx=np.zeros((T, nd)), Qx=np.zeros((max(T - 1, 0), nd)), Qu=np.zeros((max(T - 1, 0), nu)), dV=np.zeros(2),
                 failure=np.zeros(max(T, 1), np.int32))
        dp = capi.c_double_p
        ptr = lambda a: (a if a.size else np.zeros(1)).ctypes.data_as(dp)      # noqa: E731
        rc = self.lib.mjpc_hip_trajectory_gradient(self.h, T, x.ctypes.data_as(dp), ptr(u), t.ctypes.data_as(dp), ptr(r), pmo, pud, float(eps),
                                                   int(bool(centered)), ptr(o["k"]), ptr(o["Vx"]), ptr(o["Qx"]), ptr(o["Qu"]), ptr(o["dV"]),
                                                   o["failure"].ctypes.data_as(capi.c_int_p))
        if rc != 0:
            raise RuntimeError("mjpc_hip_trajectory_gradient failed: " + self.lib.mjpc_hip_last_error().decode())
        o["failure"] = o["failure"][:T]
        return o

    @staticmethod
    def _riccati_out(T, nd, nu):
        return dict(k=np.zeros((T, nu)), K=np.zeros((T, nu, nd)), Vx=np.zeros((T, nd)), Vxx=np.zeros((T, nd, nd)), Qx=np.zeros((T - 1, nd)),
                    Qu=np.zeros((T - 1, nu)), Qxx=np.zeros((T - 1, nd, nd)), Qxu=np.zeros((T - 1, nd, nu)), Quu=np.zeros((T - 1, nu, nu)), dV=np.zeros(2))

    def ilqg_backward_pass(self, A, B, cx, cu, cxx, cxu, cuu, actions=None, action_limits=None, regularization=1.0, regularization_rate=1.0,
                           settings=None, **kw):
        """The iLQG backward pass on the device (mjpc_hip_ilqg_backward_pass): Riccati recursion with the box-constrained control solve and the
        regularisation loop in one kernel.  cx [T, nd], cu [T, nu] give the dimensions (they need not be the engine's model's); A [T-1 or more,
        nd, nd], B [.., nd, nu], cxx [T, nd, nd], cxu [T, nd, nu], cuu [T, nu, nu], actions [T-1 or more, nu], action_limits [nu, 2].  settings: a
        capi.MjpcHipRiccatiSettings, or the keywords of capi.riccati_settings (regularization_type, action_limits_on, ...).  -> dict(k, K [T, nu, nd], Vx, Vxx, Qx, Qu, Qxx, Qxu, Quu, dV, status [3],
        regularization, regularization_rate)."""
        cx = np.ascontiguousarray(cx, dtype=np.float64); cu = np.ascontiguousarray(cu, dtype=np.float64)
        T, nd = cx.shape; nu = cu.shape[1]
        s = settings if settings is not None else capi.riccati_settings(**kw)
        flat = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(-1)      # noqa: E731
        ins = [flat(a) for a in (A, B, cx, cu, cxx, cxu, cuu, actions, action_limits)]
        need = [(T - 1) * nd * nd, (T - 1) * nd * nu, T * nd, (T - 1) * nu, T * nd * nd, (T - 1) * nd * nu, (T - 1) * nu * nu, (T - 1) * nu, 2 * nu]
        if T >= 2:
            for a, n_, name in zip(ins, need, ("A", "B", "cx", "cu", "cxx", "cxu", "cuu", "actions", "action_limits")):
                if a is not None and a.size < n_:
                    raise ValueError(f"ilqg_backward_pass: {name} holds {a.size} numbers, {n_} are read")
        o = self._riccati_out(max(T, 1), nd, nu)
        reg = np.array([regularization, regularization_rate], dtype=np.float64); st = np.zeros(3, np.int32)
        dp = capi.c_double_p
        ptr = lambda a: None if a is None else (a if a.size else np.zeros(1)).ctypes.data_as(dp)      # noqa: E731
        rc = self.lib.mjpc_hip_ilqg_backward_pass(self.h, T, nd, nu, *[ptr(a) for a in ins], C.byref(s), reg[0:].ctypes.data_as(dp), reg[1:].ctypes.data_as(dp),
                                                  *[ptr(o[k]) for k in ("k", "K", "Vx", "Vxx", "Qx", "Qu", "Qxx", "Qxu", "Quu", "dV")],
                                                  st.ctypes.data_as(capi.c_int_p))
        if rc != 0:
            raise RuntimeError("mjpc_hip_ilqg_backward_pass failed: " + self.lib.mjpc_hip_last_error().decode())
        o["status"] = st; o["regularization"] = float(reg[0]); o["regularization_rate"] = float(reg[1])
        return o

    def _window(self, q, act, ctrl, time, sensor_measurement, force_measurement, settings):
        nq, nv, na, nu = self.model["nq"], self.model["nv"], self.model["na"], self.model["nu"]
        f64 = lambda a, *sh: np.ascontiguousarray(np.zeros(sh) if a is None else a, dtype=np.float64).reshape(*sh)      # noqa: E731
        q = np.ascontiguousarray(q, dtype=np.float64); q = q.reshape((1,) + q.shape) if q.ndim == 2 else q
        W, T = q.shape[0], q.shape[1]
        tile = lambda a, n: np.ascontiguousarray(np.broadcast_to(np.zeros((1, T, n)) if a is None or n == 0 else f64(a, -1, T, n), (W, T, n)))      # noqa: E731
        return W, T, [q.reshape(W, T, nq), tile(act, na), tile(ctrl, nu), f64(time, T), f64(sensor_measurement, T, settings.num_sensor_rows),
                      f64(force_measurement, T, nv)]

    def direct_cost(self, settings, q, act, ctrl, time, sensor_measurement, force_measurement, mocap=None, userdata=None, discrete=True, fill=0.0):
        """The direct optimiser's cost of nwin candidate windows in one call (mjpc_hip_direct_cost): q [nwin, T, nq] (or [T, nq]); act, ctrl per
        window or shared (None: zeros); time [T], sensor_measurement [T, ns], force_measurement [T, nv] shared.  -> dict(cost [nwin, 3] = cost,
        cost_sensor, cost_force; velocity, acceleration, force_prediction [nwin, T, nv]; sensor_prediction [nwin, T, ns]; failure [nwin, T])."""
        W, T, ins = self._window(q, act, ctrl, time, sensor_measurement, force_measurement, settings)
        nv, ns = self.model["nv"], settings.num_sensor_rows
        mo, ud, pmo, pud = self._shared(mocap, userdata)
        o = dict(cost=np.full((W, 3), fill), velocity=np.full((W, T, nv), fill), acceleration=np.full((W, T, nv), fill),
                 sensor_prediction=np.full((W, T, ns), fill), force_prediction=np.full((W, T, nv), fill))
        fail = np.zeros((W, T), np.int32)
        ptr = lambda a: (a if a.size else np.zeros(1)).ctypes.data_as(capi.c_double_p)      # noqa: E731
        rc = self.lib.mjpc_hip_direct_cost(self.h, W, T, C.byref(settings), int(bool(discrete)), *[ptr(a) for a in ins], pmo, pud,
                                           *[ptr(a) for a in o.values()], fail.ctypes.data_as(capi.c_int_p))
        if rc != 0:
            raise RuntimeError("mjpc_hip_direct_cost failed: " + self.lib.mjpc_hip_last_error().decode())
        o["failure"] = fail
        return o

    def direct_cost_derivatives(self, settings, q, act, ctrl, time, sensor_measurement, force_measurement, mocap=None, userdata=None, discrete=True,
                                eps=1e-6, centered=False, fill=0.0):
        """Cost, gradient and band Hessian of one window with everything on the device (mjpc_hip_direct_cost_derivatives): q [T, nq], act, ctrl,
        time [T], measurements as direct_cost.  -> the dict of direct_assemble plus DfDq .. DsDa, dvdq0, dvdq1 [T, nv, nv], failure [T]."""
        W, T, ins = self._window(q, act, ctrl, time, sensor_measurement, force_measurement, settings)
        if W != 1:
            raise ValueError("direct_cost_derivatives: one window")
        nv, nr, ns = self.model["nv"], self.task["num_residual"], settings.num_sensor_rows
        mo, ud, pmo, pud = self._shared(mocap, userdata)
        o = dict(cost=np.full(3, fill), gradient=np.full(T * nv, fill), hessian_band=np.full((T * nv, 3 * nv), fill),
                 block_sensor=np.full((T, ns, 3 * nv), fill), block_force=np.full((T, nv, 3 * nv), fill), norm_gradient_sensor=np.full((T, ns), fill),
                 norm_gradient_force=np.full((T, nv), fill), residual_sensor=np.full((T, ns), fill), residual_force=np.full((T, nv), fill),
                 DfDq=np.full((T, nv, nv), fill), DfDv=np.full((T, nv, nv), fill), DfDa=np.full((T, nv, nv), fill), DsDq=np.full((T, nr, nv), fill),
                 DsDv=np.full((T, nr, nv), fill), DsDa=np.full((T, nr, nv), fill), dvdq0=np.full((T, nv, nv), fill), dvdq1=np.full((T, nv, nv), fill))
        fail = np.zeros(T, np.int32)
        ptr = lambda a: (a if a.size else np.zeros(1)).ctypes.data_as(capi.c_double_p)      # noqa: E731
        rc = self.lib.mjpc_hip_direct_cost_derivatives(self.h, T, C.byref(settings), float(eps), int(bool(centered)), int(bool(discrete)),
                                                       *[ptr(a) for a in ins], pmo, pud, *[ptr(a) for a in o.values()], fail.ctypes.data_as(capi.c_int_p))
        if rc != 0:
            raise RuntimeError("mjpc_hip_direct_cost_derivatives failed: " + self.lib.mjpc_hip_last_error().decode())
        o["failure"] = fail
        return o

    def direct_assemble(self, settings, residual_sensor, residual_force, DfDq, DfDv, DfDa, DsDq, DsDv, DsDa, dvdq0, dvdq1, fill=0.0):
        """The direct optimiser's window cost, gradient and band Hessian from given arrays (mjpc_hip_direct_assemble): the chain rule over the six
        inverse blocks DfD* [T, nv, nv], DsD* [T, nr, nv] and the velocity blocks dvdq0, dvdq1 [T, nv, nv], the norms of residual_sensor [T, ns] and
        residual_force [T, nv], and the sums, on the device.  settings: capi.direct_settings(...).  nv, nr and T are the arrays' (they need not be
        the engine's model's).  -> dict(cost [3] = cost, cost_sensor, cost_force; gradient [T nv]; hessian_band [T nv, 3 nv]; block_sensor
        [T, ns, 3 nv]; block_force [T, nv, 3 nv]; norm_gradient_sensor; norm_gradient_force; residual_sensor; residual_force)."""
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)      # noqa: E731
        DfDq = f64(DfDq); T, nv = DfDq.shape[0], DfDq.shape[-1]
        ns = settings.num_sensor_rows
        DsDq = f64(DsDq).reshape(T, -1, nv); nr = DsDq.shape[1]
        ins = [f64(residual_sensor).reshape(T, ns), f64(residual_force).reshape(T, nv), DfDq.reshape(T, nv, nv), f64(DfDv).reshape(T, nv, nv),
               f64(DfDa).reshape(T, nv, nv), DsDq, f64(DsDv).reshape(T, nr, nv), f64(DsDa).reshape(T, nr, nv), f64(dvdq0).reshape(T, nv, nv),
               f64(dvdq1).reshape(T, nv, nv)]
        o = dict(cost=np.full(3, fill), gradient=np.full(T * nv, fill), hessian_band=np.full((T * nv, 3 * nv), fill),
                 block_sensor=np.full((T, ns, 3 * nv), fill), block_force=np.full((T, nv, 3 * nv), fill), norm_gradient_sensor=np.full((T, ns), fill),
                 norm_gradient_force=np.full((T, nv), fill), residual_sensor=np.full((T, ns), fill), residual_force=np.full((T, nv), fill))
        dp = capi.c_double_p
        ptr = lambda a: (a if a.size else np.zeros(1)).ctypes.data_as(dp)      # noqa: E731
        rc = self.lib.mjpc_hip_direct_assemble(self.h, T, nv, nr, C.byref(settings), *[ptr(a) for a in ins], *[ptr(a) for a in o.values()])
        if rc != 0:
            raise RuntimeError("mjpc_hip_direct_assemble failed: " + self.lib.mjpc_hip_last_error().decode())
        return o

    def trajectory_ilqg(self, x, u, time, residual, mocap=None, userdata=None, eps=1e-6, centered=False, regularization=1.0, regularization_rate=1.0,
                        settings=None, **kw):
        """One derivative iteration of iLQG on the device (mjpc_hip_trajectory_ilqg): transition_fd with the last knot terminal, cost derivatives
        with Hessians, backward pass; one download.  The action limits are the model's ctrlrange (an unlimited actuator: -inf, +inf).
        -> the dict of ilqg_backward_pass plus failure [T]."""
        ds, nd, nu, nr = self._dims()
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, ds); T = x.shape[0]
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(T, nu); t = np.ascontiguousarray(time, dtype=np.float64).reshape(T)
        r = np.ascontiguousarray(residual, dtype=np.float64).reshape(T, nr)
        mo, ud, pmo, pud = self._shared(mocap, userdata)
        s = settings if settings is not None else capi.riccati_settings(**kw)
        o = self._riccati_out(max(T, 1), nd, nu)
        fail = np.zeros(max(T, 1), np.int32)
        reg = np.array([regularization, regularization_rate], dtype=np.float64); st = np.zeros(3, np.int32)
        dp = capi.c_double_p
        ptr = lambda a: (a if a.size else np.zeros(1)).ctypes.data_as(dp)      # noqa: E731
        rc = self.lib.mjpc_hip_trajectory_ilqg(self.h, T, x.ctypes.data_as(dp), ptr(u), t.ctypes.data_as(dp), ptr(r), pmo, pud, float(eps), int(bool(centered)),
                                               C.byref(s), reg[0:].ctypes.data_as(dp), reg[1:].ctypes.data_as(dp),
                                               *[ptr(o[k]) for k in ("k", "K", "Vx", "Vxx", "Qx", "Qu", "Qxx", "Qxu", "Quu", "dV")],
                                               st.ctypes.data_as(capi.c_int_p), fail.ctypes.data_as(capi.c_int_p))
        if rc != 0:
            raise RuntimeError("mjpc_hip_trajectory_ilqg failed: " + self.lib.mjpc_hip_last_error().decode())
        o["status"] = st; o["regularization"] = float(reg[0]); o["regularization_rate"] = float(reg[1]); o["failure"] = fail[:T]
        return o

    def candidate(self, local_index, H, P):
        o, c, ntr = self._alloc_out(1, H, P)
        if self.lib.mjpc_hip_get_candidate(self.h, int(local_index), C.byref(c)) != 0:
            raise RuntimeError(self.lib.mjpc_hip_last_error().decode())
        o["trace"] = o["trace"][:, :ntr]
        return o

    def fetch_all(self, nl, H, P):
        """Every local candidate's Trajectory arrays of the last plan (tests / GUI traces)."""
        m, t = self.model, self.task
        ds = m["nq"] + m["nv"] + m["na"]; nu = m["nu"]; nr = t["num_residual"]; ntr = 3 * t["num_trace"]
        o = dict(states=np.zeros((nl, H, ds)), actions=np.zeros((nl, H, nu)), times=np.zeros((nl, H)),
                 residual=np.zeros((nl, H, nr)), costs=np.zeros((nl, H)), trace=np.zeros((nl, H, max(ntr, 1))),
                 knots=np.zeros((nl, P, nu)), diag=np.zeros((nl, 4), np.int32))
        rc = self.lib.mjpc_hip_get_all_candidates(self.h, *[o[k].ctypes.data_as(capi.c_double_p) for k in
                                                         ["states", "actions", "times", "residual", "costs", "trace", "knots"]],
                                               o["diag"].ctypes.data_as(capi.c_int_p))
        if rc != 0:
            raise RuntimeError(self.lib.mjpc_hip_last_error().decode())
        o["trace"] = o["trace"][:, :, :ntr]
        return o

    def lds_bytes(self):
        return self.lib.mjpc_hip_lds_bytes(self.h)

    def spill_bytes(self):
        """Bytes of HBM slab per candidate of the spill flavour (state too large for LDS, rollout_spill.hip); 0 when it runs in LDS."""
        n = C.c_int(0)
        self.lib.mjpc_hip_debug_spill(self.h, C.byref(n))
        return n.value

    def dense_tier(self):
        """(LDS bytes of the two-candidates-per-CU tier or 0, whether the last plan ran on it)."""
        used = C.c_int(0)
        n = self.lib.mjpc_hip_dense_tier(self.h, C.byref(used))
        return n, bool(used.value)

    def dense_capacity(self):
        """(rows, contacts, hot tables in LDS) of the dense tier; (0, 0, False) without one.  Diagnostics."""
        a = C.c_int(0); b = C.c_int(0); h = C.c_int(0)
        self.lib.mjpc_hip_debug_dense_capacity(self.h, C.byref(a), C.byref(b), C.byref(h))
        return a.value, b.value, bool(h.value)

    def kernel_time(self):
        a = C.c_double(0); b = C.c_double(0)
        n = self.lib.mjpc_hip_kernel_time(self.h, C.byref(a), C.byref(b))
        return n, a.value, b.value


class HipMultiBackend:
    """One planner process, one rollout engine per GPU (mjpc_hip_multi_*, include/mjpc_hip.h): plan() block-partitions the
    global candidate batch over the engines, picks the elite across them and copies the winner's trajectory from its owner.
    devices: HIP ordinals, repeats allowed (several engines on one GPU: 1-GPU rehearsal)."""

    def __init__(self, model: dict, task: dict, devices, max_samples=128, max_horizon=kMaxTrajectoryHorizon):
        self.lib = capi.load_engine()
        self.cm = capi.CModel(model, task)
        self.model = model; self.task = task
        dv = (C.c_int * len(devices))(*[int(x) for x in devices])
        self.h = self.lib.mjpc_hip_multi_create(C.byref(self.cm.c_model), C.byref(self.cm.c_task), int(max_samples), int(max_horizon),
                                                len(devices), dv)
        if not self.h:
            raise RuntimeError("mjpc_hip_multi_create failed: " + self.lib.mjpc_hip_last_error().decode())
        self.h = C.c_void_p(self.h)

    def close(self):
        if getattr(self, "h", None):
            self.lib.mjpc_hip_multi_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    _alloc_out = HipBackend._alloc_out

    def plan(self, **kw):
        inp = capi.make_plan_input(self.cm, **kw)
        o, c, ntr = self._alloc_out(inp.num_trajectory, inp.horizon, inp.num_spline_points)
        if self.lib.mjpc_hip_multi_plan(self.h, C.byref(inp), C.byref(c)) != 0:
            raise RuntimeError("mjpc_hip_multi_plan failed: " + self.lib.mjpc_hip_last_error().decode())
        o["winner"] = c.winner; o["winner_return"] = c.winner_return
        o["noise_compute_time_us"] = c.noise_compute_time_us; o["rollouts_compute_time_us"] = c.rollouts_compute_time_us
        o["trace"] = o["trace"][:, :ntr]
        return o

    def candidate(self, index, H, P):
        o, c, ntr = self._alloc_out(1, H, P)
        if self.lib.mjpc_hip_multi_get_candidate(self.h, int(index), C.byref(c)) != 0:
            raise RuntimeError(self.lib.mjpc_hip_last_error().decode())
        o["trace"] = o["trace"][:, :ntr]
        return o

    def knots(self, N, P):
        k = np.zeros((N, P, self.model["nu"]))
        if self.lib.mjpc_hip_multi_get_knots(self.h, k.ctypes.data_as(capi.c_double_p)) != 0:
            raise RuntimeError(self.lib.mjpc_hip_last_error().decode())
        return k

    def traces(self, N, H):
        ntr = 3 * self.task["num_trace"]
        t = np.zeros((N, H, max(ntr, 1)))
        if self.lib.mjpc_hip_multi_get_traces(self.h, t.ctypes.data_as(capi.c_double_p)) != 0:
            raise RuntimeError(self.lib.mjpc_hip_last_error().decode())
        return t[:, :, :ntr] if ntr else t[:, :, :0]
