"""ctypes view of the C++ host planner (include/mjpc_hip_planner.h via include/mjpc_hip_planner_c.h).

The C++ classes `mjpc_hip::TimeSpline` / `mjpc_hip::SamplingPlanner` in libmjpc_hip.so are the product's host side
(the reference's planner is compiled C++: mjpc/planners/sampling/planner.cc); this module only lets Python drive
them.  There is no Python fall-back: a missing library raises in capi.load_engine().
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

c_double_p = C.POINTER(C.c_double)
c_int_p = C.POINTER(C.c_int)
_ERR_CB = C.CFUNCTYPE(None, C.c_char_p)

PLANNER_C_SYMBOLS = [
    "mjpc_planner_set_error_handler",
    "mjpc_spline_create", "mjpc_spline_destroy", "mjpc_spline_size", "mjpc_spline_add_node", "mjpc_spline_sample",
    "mjpc_spline_discard_before", "mjpc_spline_clear", "mjpc_spline_set_interpolation",
    "mjpc_planner_create", "mjpc_planner_create_sharded", "mjpc_planner_destroy", "mjpc_planner_reset", "mjpc_planner_set_state", "mjpc_planner_set_task",
    "mjpc_planner_optimize_policy", "mjpc_planner_nominal_trajectory", "mjpc_planner_action_from_policy",
    "mjpc_planner_optimize_policy_candidates", "mjpc_planner_candidate_score", "mjpc_planner_action_from_candidate_policy",
    "mjpc_planner_copy_candidate_to_policy", "mjpc_planner_winner", "mjpc_planner_improvement", "mjpc_planner_num_parameters",
    "mjpc_planner_set_seed", "mjpc_planner_set_num_trajectory", "mjpc_planner_set_noise", "mjpc_planner_returns",
    "mjpc_planner_policy", "mjpc_planner_best_trajectory", "mjpc_planner_timings",
    "mjpc_cem_create", "mjpc_cem_destroy", "mjpc_cem_reset", "mjpc_cem_set_state", "mjpc_cem_set_seed", "mjpc_cem_set_noise",
    "mjpc_cem_optimize_policy", "mjpc_cem_nominal_trajectory", "mjpc_cem_action_from_policy", "mjpc_cem_improvement",
    "mjpc_cem_returns", "mjpc_cem_variance", "mjpc_cem_policy", "mjpc_cem_best_trajectory",
    "mjpc_testspeed_run",
    "mjpc_robust_create", "mjpc_robust_destroy", "mjpc_robust_reset", "mjpc_robust_set_state", "mjpc_robust_set_seed",
    "mjpc_robust_optimize_policy", "mjpc_robust_action_from_policy", "mjpc_robust_last", "mjpc_robust_delegate",
]
# the flat C view of the SampleGradientPlanner (same header)
SAMPLE_GRADIENT_C_SYMBOLS = [
    "mjpc_sg_create", "mjpc_sg_destroy", "mjpc_sg_reset", "mjpc_sg_set_state", "mjpc_sg_set_task", "mjpc_sg_set_seed", "mjpc_sg_set_noise",
    "mjpc_sg_set_counts", "mjpc_sg_optimize_policy", "mjpc_sg_nominal_trajectory", "mjpc_sg_action_from_policy", "mjpc_sg_improvement",
    "mjpc_sg_winner", "mjpc_sg_winner_type", "mjpc_sg_num_gradient", "mjpc_sg_num_parameters", "mjpc_sg_returns", "mjpc_sg_trajectory_order",
    "mjpc_sg_gradient", "mjpc_sg_return_weight", "mjpc_sg_step_size", "mjpc_sg_policy", "mjpc_sg_candidate_policy", "mjpc_sg_best_trajectory",
    "mjpc_sg_timings", "mjpc_sg_return_weights", "mjpc_sg_log_scale",
]


class PlannerError(RuntimeError):
    """Raised where the reference would abort through mju_error (planner.cc:69-72, spline.cc:205-208)."""


_lib = None
_pending: list[str] = []


@_ERR_CB
def _on_error(msg):
    _pending.append(msg.decode() if msg else "unknown")


def _check():
    if _pending:
        msg = _pending[0]
        _pending.clear()
        raise PlannerError(msg)


def _dp(a):
    return None if a is None else a.ctypes.data_as(c_double_p)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = capi.load_engine()
    vp, d, i = C.c_void_p, C.c_double, C.c_int
    sig = {
        "mjpc_planner_set_error_handler": (None, [_ERR_CB]),
        "mjpc_spline_create": (vp, [i, i]), "mjpc_spline_destroy": (None, [vp]), "mjpc_spline_size": (i, [vp]),
        "mjpc_spline_add_node": (None, [vp, d, c_double_p]), "mjpc_spline_sample": (None, [vp, d, c_double_p]),
        "mjpc_spline_discard_before": (i, [vp, d]), "mjpc_spline_clear": (None, [vp]),
        "mjpc_spline_set_interpolation": (None, [vp, i]),
        "mjpc_planner_create": (vp, [C.POINTER(capi.MjpcHipModel), C.POINTER(capi.MjpcHipTask), c_double_p, i, i, i, i, i, i, i]),
        "mjpc_planner_create_sharded": (vp, [C.POINTER(capi.MjpcHipModel), C.POINTER(capi.MjpcHipTask), c_double_p, i, i, i, i, i, i, i, C.POINTER(C.c_int)]),
        "mjpc_planner_destroy": (None, [vp]), "mjpc_planner_reset": (None, [vp, i, c_double_p]),
        "mjpc_planner_set_state": (None, [vp, c_double_p, c_double_p, c_double_p, d]),
        "mjpc_planner_set_task": (None, [vp, C.POINTER(capi.MjpcHipTask)]),
        "mjpc_planner_optimize_policy": (None, [vp, i]), "mjpc_planner_nominal_trajectory": (None, [vp, i]),
        "mjpc_planner_action_from_policy": (None, [vp, c_double_p, d, i]),
        "mjpc_planner_optimize_policy_candidates": (i, [vp, i, i]), "mjpc_planner_candidate_score": (d, [vp, i]),
        "mjpc_planner_action_from_candidate_policy": (None, [vp, c_double_p, i, d]),
        "mjpc_planner_copy_candidate_to_policy": (None, [vp, i]), "mjpc_planner_winner": (i, [vp]),
        "mjpc_planner_improvement": (d, [vp]), "mjpc_planner_num_parameters": (i, [vp]),
        "mjpc_planner_set_seed": (None, [vp, C.c_ulonglong, C.c_ulonglong]), "mjpc_planner_set_num_trajectory": (None, [vp, i]),
        "mjpc_planner_set_noise": (None, [vp, c_double_p, c_int_p]), "mjpc_planner_returns": (None, [vp, c_double_p, i]),
        "mjpc_planner_policy": (i, [vp, i, c_double_p, c_double_p]),
        "mjpc_planner_best_trajectory": (i, [vp] + [c_double_p] * 7 + [c_int_p]),
        "mjpc_planner_timings": (None, [vp, c_double_p, c_double_p, c_double_p]),
        "mjpc_cem_create": (vp, [C.POINTER(capi.MjpcHipModel), C.POINTER(capi.MjpcHipTask), d, d, i, i, i, i, i, i, i]),
        "mjpc_cem_destroy": (None, [vp]), "mjpc_cem_reset": (None, [vp, i, c_double_p]),
        "mjpc_cem_set_state": (None, [vp, c_double_p, c_double_p, c_double_p, d]),
        "mjpc_cem_set_seed": (None, [vp, C.c_ulonglong, C.c_ulonglong]), "mjpc_cem_set_noise": (None, [vp, c_double_p]),
        "mjpc_cem_optimize_policy": (None, [vp, i]), "mjpc_cem_nominal_trajectory": (None, [vp, i]),
        "mjpc_cem_action_from_policy": (None, [vp, c_double_p, d, i]), "mjpc_cem_improvement": (d, [vp]),
        "mjpc_cem_returns": (None, [vp, c_double_p, i]), "mjpc_cem_variance": (None, [vp, c_double_p, i]),
        "mjpc_cem_policy": (i, [vp, c_double_p, c_double_p]),
        "mjpc_cem_best_trajectory": (i, [vp, c_double_p, c_double_p, c_double_p, c_double_p]),
        "mjpc_robust_create": (vp, [C.POINTER(capi.MjpcHipModel), C.POINTER(capi.MjpcHipTask), c_double_p, i, i, i, i, i, d, d, i, i, i]),
        "mjpc_robust_destroy": (None, [vp]), "mjpc_robust_reset": (None, [vp, i]),
        "mjpc_robust_set_state": (None, [vp, c_double_p, c_double_p, c_double_p, d]),
        "mjpc_robust_set_seed": (None, [vp, C.c_ulonglong, C.c_ulonglong, C.c_ulonglong]),
        "mjpc_robust_optimize_policy": (None, [vp, i]), "mjpc_robust_action_from_policy": (None, [vp, c_double_p, d]),
        "mjpc_robust_last": (None, [vp, c_int_p, c_double_p, c_double_p]), "mjpc_robust_delegate": (vp, [vp]),
        "mjpc_sg_create": (vp, [C.POINTER(capi.MjpcHipModel), C.POINTER(capi.MjpcHipTask), d, i, i, d, i, i, i, i, i]),
        "mjpc_sg_destroy": (None, [vp]), "mjpc_sg_reset": (None, [vp, i, c_double_p]),
        "mjpc_sg_set_state": (None, [vp, c_double_p, c_double_p, c_double_p, d]),
        "mjpc_sg_set_task": (None, [vp, C.POINTER(capi.MjpcHipTask)]),
        "mjpc_sg_set_seed": (None, [vp, C.c_ulonglong, C.c_ulonglong]), "mjpc_sg_set_noise": (None, [vp, c_double_p]),
        "mjpc_sg_set_counts": (None, [vp, i, i]),
        "mjpc_sg_optimize_policy": (None, [vp, i]), "mjpc_sg_nominal_trajectory": (None, [vp, i]),
        "mjpc_sg_action_from_policy": (None, [vp, c_double_p, d, i]), "mjpc_sg_improvement": (d, [vp]),
        "mjpc_sg_winner": (i, [vp]), "mjpc_sg_winner_type": (i, [vp]), "mjpc_sg_num_gradient": (i, [vp]), "mjpc_sg_num_parameters": (i, [vp]),
        "mjpc_sg_returns": (None, [vp, c_double_p, i]), "mjpc_sg_trajectory_order": (None, [vp, c_int_p, i]),
        "mjpc_sg_gradient": (None, [vp, c_double_p, i]), "mjpc_sg_return_weight": (i, [vp, c_double_p]), "mjpc_sg_step_size": (i, [vp, c_double_p]),
        "mjpc_sg_policy": (i, [vp, c_double_p, c_double_p]), "mjpc_sg_candidate_policy": (i, [vp, i, c_double_p, c_double_p]),
        "mjpc_sg_best_trajectory": (i, [vp, c_double_p, c_double_p, c_double_p, c_double_p]),
        "mjpc_sg_timings": (None, [vp, c_double_p, c_double_p, c_double_p, c_double_p]),
        "mjpc_sg_return_weights": (None, [c_int_p, i, c_double_p]), "mjpc_sg_log_scale": (None, [c_double_p, d, d, i]),
        "mjpc_gd_create": (vp, [C.POINTER(capi.MjpcHipModel), C.POINTER(capi.MjpcHipTask), i, i, i, i, i, d, d, i, i, i, i]),
        "mjpc_gd_destroy": (None, [vp]), "mjpc_gd_reset": (None, [vp, i, c_double_p]),
        "mjpc_gd_set_state": (None, [vp, c_double_p, c_double_p, c_double_p, d]),
        "mjpc_gd_set_task": (None, [vp, C.POINTER(capi.MjpcHipTask)]), "mjpc_gd_set_num_trajectory": (None, [vp, i]),
        "mjpc_gd_optimize_policy": (None, [vp, i]), "mjpc_gd_nominal_trajectory": (None, [vp, i]),
        "mjpc_gd_action_from_policy": (None, [vp, c_double_p, d, i]), "mjpc_gd_improvement": (d, [vp]),
        "mjpc_gd_policy": (i, [vp, c_double_p, c_double_p]), "mjpc_gd_set_policy": (None, [vp, c_double_p, c_double_p]),
        "mjpc_gd_best_trajectory": (i, [vp, c_double_p, c_double_p, c_double_p, c_double_p]),
        "mjpc_gd_values": (None, [vp, c_double_p]), "mjpc_gd_timings": (None, [vp, c_double_p]), "mjpc_gd_returns": (None, [vp, c_double_p, i]),
        "mjpc_gd_linesearch_steps": (i, [vp, c_double_p]), "mjpc_gd_parameter_update": (i, [vp, c_double_p]),
        "mjpc_ilqg_create": (vp, [C.POINTER(capi.MjpcHipModel), C.POINTER(capi.MjpcHipTask), i, i, i, i, c_double_p, i, i, i]),
        "mjpc_ilqg_destroy": (None, [vp]), "mjpc_ilqg_reset": (None, [vp, i, c_double_p]),
        "mjpc_ilqg_set_state": (None, [vp, c_double_p, c_double_p, c_double_p, d]),
        "mjpc_ilqg_set_task": (None, [vp, C.POINTER(capi.MjpcHipTask)]), "mjpc_ilqg_set_num_trajectory": (None, [vp, i]),
        "mjpc_ilqg_optimize_policy": (None, [vp, i]), "mjpc_ilqg_nominal_trajectory": (None, [vp, i]), "mjpc_ilqg_iteration": (None, [vp, i]),
        "mjpc_ilqg_action_from_policy": (None, [vp, c_double_p, c_double_p, d, i]), "mjpc_ilqg_improvement": (d, [vp]),
        "mjpc_ilqg_best_trajectory": (i, [vp, c_double_p, c_double_p, c_double_p, c_double_p]),
        "mjpc_ilqg_values": (None, [vp, c_double_p]), "mjpc_ilqg_timings": (None, [vp, c_double_p]), "mjpc_ilqg_returns": (None, [vp, c_double_p, i]),
        "mjpc_ilqg_linesearch_steps": (i, [vp, c_double_p]),
        "mjpc_ilqg_get_policy": (i, [vp, i, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
        "mjpc_ilqg_best_rollout": (i, [c_double_p, c_int_p, i]),
        "mjpc_ilqs_create": (vp, [C.POINTER(capi.MjpcHipModel), C.POINTER(capi.MjpcHipTask), c_double_p, i, i, i, i, i, i, i, i, c_double_p, i, i, i]),
        "mjpc_ilqs_set_noise_exploration": (None, [vp, d, d]),
        "mjpc_ilqs_destroy": (None, [vp]), "mjpc_ilqs_reset": (None, [vp, i, c_double_p]),
        "mjpc_ilqs_set_state": (None, [vp, c_double_p, c_double_p, c_double_p, d]),
        "mjpc_ilqs_set_task": (None, [vp, C.POINTER(capi.MjpcHipTask)]),
        "mjpc_ilqs_optimize_policy": (None, [vp, i]), "mjpc_ilqs_nominal_trajectory": (None, [vp, i]),
        "mjpc_ilqs_action_from_policy": (None, [vp, c_double_p, c_double_p, d, i]),
        "mjpc_ilqs_best_trajectory": (i, [vp, c_double_p, c_double_p, c_double_p, c_double_p]),
        "mjpc_ilqs_values": (None, [vp, c_int_p]), "mjpc_ilqs_timings": (None, [vp, c_double_p]),
        "mjpc_ilqs_sampling": (vp, [vp]), "mjpc_ilqs_ilqg": (vp, [vp]),
        "mjpc_ilqs_fitted_knots": (i, [vp, c_double_p, c_double_p]),
        "mjpc_ilqs_sampling_member": (i, [vp, i, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
        "mjpc_ilqs_action_source": (i, [i, i, i]),
        "mjpc_ilqs_spline_fit": (i, [i, i, c_double_p, i, c_double_p, i, c_double_p, c_double_p]),
        "mjpc_gd_spline_mapping": (None, [i, i, c_double_p, i, c_double_p, i, c_double_p]),
        "mjpc_gd_policy_action": (None, [i, i, c_double_p, c_double_p, c_double_p, i, d, c_double_p]),
        "mjpc_testspeed_run": (d, [C.POINTER(capi.MjpcHipModel), C.POINTER(capi.MjpcHipTask), vp, i, c_double_p, c_double_p, d, i, i, d, i,
                                   c_double_p, c_double_p, i, d, c_double_p]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res; f.argtypes = args
    L.mjpc_planner_set_error_handler(_on_error)
    _lib = L
    return L


class TimeSpline:
    """mjpc_hip::TimeSpline (C++) — same surface as mjpc::spline::TimeSpline (spline.h:41-276)."""

    def __init__(self, dim=0, interpolation=0):
        self._L = lib()
        self.dim_ = int(dim)
        self._h = C.c_void_p(self._L.mjpc_spline_create(self.dim_, int(interpolation)))

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.mjpc_spline_destroy(self._h); self._h = None

    def Size(self): return self._L.mjpc_spline_size(self._h)
    def Dim(self): return self.dim_
    def SetInterpolation(self, interpolation): self._L.mjpc_spline_set_interpolation(self._h, int(interpolation))
    def Clear(self): self._L.mjpc_spline_clear(self._h)

    def AddNode(self, time, values=None):
        v = None if values is None else np.ascontiguousarray(values, dtype=np.float64)
        self._L.mjpc_spline_add_node(self._h, float(time), _dp(v))
        _check()

    def DiscardBefore(self, time): return self._L.mjpc_spline_discard_before(self._h, float(time))

    def Sample(self, time):
        out = np.zeros(self.dim_)
        self._L.mjpc_spline_sample(self._h, float(time), _dp(out))
        _check()
        return out


class Trajectory:
    pass


class _Planner:
    """What the four ctypes views share: the handle and the calls that differ only in the C symbol prefix."""
    _prefix = ""

    def __init__(self):
        self._L = lib()
        self._h = None
        self._noise = None

    def _fn(self, name):
        return getattr(self._L, self._prefix + name)

    def Allocate(self):        # done inside the C create call (Initialize + Allocate)
        pass

    def close(self):
        if self._h:
            self._fn("destroy")(self._h); self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def Reset(self, horizon=0, initial_repeated_action=None):
        a = None if initial_repeated_action is None else np.ascontiguousarray(initial_repeated_action, dtype=np.float64)
        self._fn("reset")(self._h, int(horizon or 0), _dp(a)); _check()

    def SetState(self, state, mocap=None, userdata=None, time=0.0):
        s = np.ascontiguousarray(state, dtype=np.float64)
        m = None if mocap is None else np.ascontiguousarray(mocap, dtype=np.float64)
        u = None if userdata is None else np.ascontiguousarray(userdata, dtype=np.float64)
        self._fn("set_state")(self._h, _dp(s), _dp(m), _dp(u), float(time))

    def SetTask(self, task: dict):
        t = self.cm.make_task(task)
        self._fn("set_task")(self._h, C.byref(t)); _check()

    def set_seed(self, seed, plan_iter=0): self._fn("set_seed")(self._h, int(seed), int(plan_iter))
    def OptimizePolicy(self, horizon): self._fn("optimize_policy")(self._h, int(horizon)); _check()
    def NominalTrajectory(self, horizon): self._fn("nominal_trajectory")(self._h, int(horizon)); _check()

    def ActionFromPolicy(self, time, use_previous=False):
        a = np.zeros(self.nu)
        self._fn("action_from_policy")(self._h, _dp(a), float(time), int(bool(use_previous))); _check()
        return a

    @property
    def improvement(self): return self._fn("improvement")(self._h)

    def returns(self, n):
        out = np.zeros(int(n)); self._fn("returns")(self._h, _dp(out), int(n)); return out

    def _knots(self, name, *lead):
        """a `<prefix><name>(handle, *lead, times, values)` call that returns P: asked once for P, once for the arrays"""
        f = self._fn(name)
        P = f(self._h, *lead, None, None)
        t = np.zeros(max(P, 1)); v = np.zeros((max(P, 1), self.nu))
        f(self._h, *lead, _dp(t), _dp(v))
        return t[:P], v[:P]

    def policy_knots(self): return self._knots("policy")

    def BestTrajectory(self):
        Hm = self.max_horizon
        st = np.zeros((Hm, self.ns)); ac = np.zeros((Hm, self.nu)); co = np.zeros(Hm); tot = C.c_double()
        H = self._fn("best_trajectory")(self._h, _dp(st), _dp(ac), _dp(co), C.byref(tot))
        t = Trajectory()
        t.horizon = H; t.states = st.ravel()[:H * self.ns].reshape(H, self.ns); t.actions = ac.ravel()[:H * self.nu].reshape(H, self.nu)
        t.costs = co[:H]; t.total_return = tot.value
        return t


class SamplingPlanner(_Planner):
    """mjpc_hip::SamplingPlanner (C++) driven from Python; method names follow planners/sampling/planner.h:51-112."""
    _prefix = "mjpc_planner_"

    def Initialize(self, model: dict, task: dict, numerics: dict | None = None, max_samples=128, max_horizon=512, device=0, devices=None):
        """devices: list of HIP ordinals to shard every plan step's candidate batch over (one engine each); None = `device` only."""
        numerics = numerics or {}
        self.cm = capi.CModel(model, task)
        se = numerics.get("sampling_exploration", 0.1)
        se = list(se) if isinstance(se, (list, tuple)) else [se]
        self._expl = np.array([float(se[0]), float(se[1]) if len(se) > 1 else 0.0])
        self.nu = int(model["nu"]); self.ns = int(model["nq"] + model["nv"] + model["na"])
        self.nr = int(task["num_residual"]); self.ntrace = int(task["num_trace"])
        self.max_samples, self.max_horizon = int(max_samples), int(max_horizon)
        self.close()
        args = (C.byref(self.cm.c_model), C.byref(self.cm.c_task), _dp(self._expl),
                int(numerics.get("sampling_trajectories", 10)), int(numerics.get("sampling_representation", 2)),
                int(numerics.get("sampling_sliding_plan", 0)), int(numerics.get("sampling_spline_points", 512)),
                self.max_samples, self.max_horizon)
        if devices is None:
            h = self._L.mjpc_planner_create(*args, int(device))
        else:
            dv = (C.c_int * len(devices))(*[int(x) for x in devices])
            h = self._L.mjpc_planner_create_sharded(*args, len(devices), dv)
        self._h = C.c_void_p(h)
        _check()

    def set_num_trajectory(self, n): self._L.mjpc_planner_set_num_trajectory(self._h, int(n))

    def set_noise(self, eps, sel):
        if eps is None:
            self._noise = None
            self._L.mjpc_planner_set_noise(self._h, None, None)
            return
        e = np.ascontiguousarray(eps, dtype=np.float64); s = np.ascontiguousarray(sel, dtype=np.int32)
        self._noise = (e, s)
        self._L.mjpc_planner_set_noise(self._h, _dp(e), s.ctypes.data_as(c_int_p))

    def OptimizePolicyCandidates(self, ncandidates, horizon):
        n = self._L.mjpc_planner_optimize_policy_candidates(self._h, int(ncandidates), int(horizon)); _check()
        return n

    def CandidateScore(self, candidate): return self._L.mjpc_planner_candidate_score(self._h, int(candidate))
    def CopyCandidateToPolicy(self, candidate): self._L.mjpc_planner_copy_candidate_to_policy(self._h, int(candidate)); _check()

    def ActionFromCandidatePolicy(self, candidate, time):
        a = np.zeros(self.nu)
        self._L.mjpc_planner_action_from_candidate_policy(self._h, _dp(a), int(candidate), float(time)); _check()
        return a

    @property
    def winner(self): return self._L.mjpc_planner_winner(self._h)
    def NumParameters(self): return self._L.mjpc_planner_num_parameters(self._h)
    def policy_knots(self, previous=False): return self._knots("policy", int(previous))

    def timings(self):
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self._L.mjpc_planner_timings(self._h, C.byref(a), C.byref(b), C.byref(c))
        return dict(noise_us=a.value, rollouts_us=b.value, policy_update_us=c.value)

    def BestTrajectory(self):      # the long form: times, residual, trace and the failure flag as well; None before the first rollout
        Hm = self.max_horizon
        st = np.zeros((Hm, self.ns)); ac = np.zeros((Hm, self.nu)); ti = np.zeros(Hm); re = np.zeros((Hm, max(self.nr, 1)))
        co = np.zeros(Hm); tr = np.zeros((Hm, 3 * max(self.ntrace, 1))); tot = C.c_double(); fail = C.c_int()
        H = self._L.mjpc_planner_best_trajectory(self._h, _dp(st), _dp(ac), _dp(ti), _dp(re), _dp(co), _dp(tr), C.byref(tot), C.byref(fail))
        if H == 0:
            return None
        t = Trajectory()
        t.horizon = H; t.states = st.ravel()[:H * self.ns].reshape(H, self.ns); t.actions = ac.ravel()[:H * self.nu].reshape(H, self.nu)
        t.times = ti[:H]; t.residual = re.ravel()[:H * self.nr].reshape(H, self.nr); t.costs = co[:H]
        t.trace = tr.ravel()[:H * 3 * self.ntrace].reshape(H, 3 * self.ntrace)
        t.total_return = tot.value; t.failure = bool(fail.value)
        return t


class CrossEntropyPlanner(_Planner):
    """mjpc_hip::CrossEntropyPlanner (C++) driven from Python; names follow planners/cross_entropy/planner.h:32-147."""
    _prefix = "mjpc_cem_"

    def Initialize(self, model: dict, task: dict, numerics: dict | None = None, max_samples=128, max_horizon=512, device=0):
        numerics = numerics or {}
        self.cm = capi.CModel(model, task)
        self.nu = int(model["nu"]); self.ns = int(model["nq"] + model["nv"] + model["na"])
        self.max_samples, self.max_horizon = int(max_samples), int(max_horizon)
        self.P = int(numerics.get("sampling_spline_points", 512))
        self.close()
        h = self._L.mjpc_cem_create(C.byref(self.cm.c_model), C.byref(self.cm.c_task), float(numerics.get("sampling_exploration", 0.1)),
                                    float(numerics.get("std_min", 0.1)), int(numerics.get("sampling_trajectories", 10)),
                                    int(numerics.get("n_elite", -1)), int(numerics.get("sampling_representation", 0)), self.P,
                                    self.max_samples, self.max_horizon, int(device))
        self._h = C.c_void_p(h)
        _check()

    def set_noise(self, eps):
        self._noise = None if eps is None else np.ascontiguousarray(eps, dtype=np.float64)
        self._L.mjpc_cem_set_noise(self._h, _dp(self._noise))

    def variance(self):
        out = np.zeros(self.P * self.nu); self._L.mjpc_cem_variance(self._h, _dp(out), out.size); return out


class SampleGradientPlanner(_Planner):
    """mjpc_hip::SampleGradientPlanner (C++) driven from Python; names follow planners/sample_gradient/planner.h:35-175."""
    _prefix = "mjpc_sg_"
    kNominal, kPerturb, kGradient = 0, 1, 2

    def Initialize(self, model: dict, task: dict, numerics: dict | None = None, max_samples=128, max_horizon=512, device=0):
        numerics = numerics or {}
        self.cm = capi.CModel(model, task)
        self.nu = int(model["nu"]); self.ns = int(model["nq"] + model["nv"] + model["na"])
        self.max_samples, self.max_horizon = int(max_samples), int(max_horizon)
        self.P = int(numerics.get("sampling_spline_points", 512))
        self.close()
        h = self._L.mjpc_sg_create(C.byref(self.cm.c_model), C.byref(self.cm.c_task), float(numerics.get("sampling_exploration", 0.1)),
                                   int(numerics.get("sampling_trajectories", 10)), int(numerics.get("sample_gradient_trajectories", 0)),
                                   float(numerics.get("sample_gradient_filter", 1.0)), int(numerics.get("sampling_representation", 0)), self.P,
                                   self.max_samples, self.max_horizon, int(device))
        self._h = C.c_void_p(h)
        _check()

    def set_counts(self, trajectories, gradient_trajectories): self._L.mjpc_sg_set_counts(self._h, int(trajectories), int(gradient_trajectories))

    def set_noise(self, eps):
        self._noise = None if eps is None else np.ascontiguousarray(eps, dtype=np.float64)
        self._L.mjpc_sg_set_noise(self._h, _dp(self._noise))

    @property
    def winner(self): return self._L.mjpc_sg_winner(self._h)
    @property
    def winner_type_(self): return self._L.mjpc_sg_winner_type(self._h)
    @property
    def num_gradient_(self): return self._L.mjpc_sg_num_gradient(self._h)
    def NumParameters(self): return self._L.mjpc_sg_num_parameters(self._h)

    def trajectory_order(self, n):
        out = np.zeros(int(n), np.int32); self._L.mjpc_sg_trajectory_order(self._h, out.ctypes.data_as(c_int_p), int(n)); return out

    def gradient(self):
        out = np.zeros(self.NumParameters()); self._L.mjpc_sg_gradient(self._h, _dp(out), out.size); return out

    def return_weight(self):
        out = np.zeros(max(self._L.mjpc_sg_return_weight(self._h, None), 1)); n = self._L.mjpc_sg_return_weight(self._h, _dp(out)); return out[:n]

    def step_size(self):
        out = np.zeros(max(self._L.mjpc_sg_step_size(self._h, None), 1)); n = self._L.mjpc_sg_step_size(self._h, _dp(out)); return out[:n]

    def candidate_policy(self, index): return self._knots("candidate_policy", int(index))

    def timings(self):
        a, b, c, g = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        self._L.mjpc_sg_timings(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(g))
        return dict(noise_us=a.value, rollouts_us=b.value, policy_update_us=c.value, gradient_candidates_us=g.value)


class GradientPlanner(_Planner):
    """mjpc_hip::GradientPlanner (C++) driven from Python; names follow planners/gradient/planner.h."""
    _prefix = "mjpc_gd_"
    kMaxGradientSplinePoints = 25

    def Initialize(self, model: dict, task: dict, numerics: dict | None = None, settings: dict | None = None, max_samples=128, max_horizon=512, device=0):
        numerics = numerics or {}; settings = settings or {}
        self.cm = capi.CModel(model, task)
        self.nu = int(model["nu"]); self.ns = int(model["nq"] + model["nv"] + model["na"])
        self.max_samples, self.max_horizon = int(max_samples), int(max_horizon)
        self.P = int(numerics.get("gradient_spline_points", 10))
        self.close()
        h = self._L.mjpc_gd_create(C.byref(self.cm.c_model), C.byref(self.cm.c_task), int(numerics.get("gradient_num_trajectory", 32)), self.P,
                                   int(numerics.get("gradient_representation", 1)), int(numerics.get("derivative_skip", 0)),
                                   int(settings.get("max_rollout", 1)), float(settings.get("min_linesearch_step", 1.0e-8)),
                                   float(settings.get("fd_tolerance", 1.0e-5)), int(settings.get("fd_mode", 0)), self.max_samples, self.max_horizon, int(device))
        self._h = C.c_void_p(h)
        _check()

    def set_num_trajectory(self, n): self._L.mjpc_gd_set_num_trajectory(self._h, int(n))

    def set_policy(self, times, values):
        t = np.ascontiguousarray(times, dtype=np.float64); v = np.ascontiguousarray(values, dtype=np.float64)
        assert t.size == self.P and v.size == self.P * self.nu
        self._L.mjpc_gd_set_policy(self._h, _dp(t), _dp(v))

    def values(self):
        o = np.zeros(6); self._L.mjpc_gd_values(self._h, _dp(o))
        return dict(action_step=o[0], expected=o[1], improvement=o[2], surprise=o[3], winner=int(o[4]), failed=bool(o[5]))

    def timings(self):
        o = np.zeros(5); self._L.mjpc_gd_timings(self._h, _dp(o))
        return dict(nominal_us=o[0], derivative_us=o[1], gradient_us=o[2], rollouts_us=o[3], policy_update_us=o[4])

    def linesearch_steps(self):
        out = np.zeros(max(self._L.mjpc_gd_linesearch_steps(self._h, None), 1)); n = self._L.mjpc_gd_linesearch_steps(self._h, _dp(out)); return out[:n]

    def parameter_update(self):
        out = np.zeros(max(self._L.mjpc_gd_parameter_update(self._h, None), 1)); n = self._L.mjpc_gd_parameter_update(self._h, _dp(out))
        return out[:n].reshape(-1, self.nu)


class iLQGPlanner(_Planner):
    """mjpc_hip::iLQGPlanner (C++) driven from Python; names follow planners/ilqg/planner.h."""
    _prefix = "mjpc_ilqg_"
    SETTINGS = ("min_linesearch_step", "fd_tolerance", "fd_mode", "min_regularization", "max_regularization", "regularization_type",
                "max_regularization_iterations", "action_limits", "nominal_feedback_scaling")
    DEFAULTS = (1.0e-3, 1.0e-6, 0, 1.0e-6, 1.0e6, 0, 5, 1, 1)

    def Initialize(self, model: dict, task: dict, numerics: dict | None = None, settings: dict | None = None, max_samples=128, max_horizon=512, device=0):
        numerics = numerics or {}; settings = settings or {}
        self.cm = capi.CModel(model, task)
        self.nu = int(model["nu"]); self.ns = int(model["nq"] + model["nv"] + model["na"]); self.nd = int(2 * model["nv"] + model["na"])
        self.max_samples, self.max_horizon = int(max_samples), int(max_horizon)
        s = np.array([float(settings.get(k, v)) for k, v in zip(self.SETTINGS, self.DEFAULTS)])
        self.close()
        h = self._L.mjpc_ilqg_create(C.byref(self.cm.c_model), C.byref(self.cm.c_task), int(numerics.get("ilqg_num_rollouts", 10)),
                                     int(numerics.get("ilqg_representation", 1)), int(numerics.get("derivative_skip", 0)),
                                     int(bool(settings.get("fused", True))), _dp(s), self.max_samples, self.max_horizon, int(device))
        self._h = C.c_void_p(h)
        _check()

    def set_num_trajectory(self, n): self._L.mjpc_ilqg_set_num_trajectory(self._h, int(n))

    def Iteration(self, horizon): self._L.mjpc_ilqg_iteration(self._h, int(horizon)); _check()

    def ActionFromPolicy(self, time, use_previous=False, state=None):
        a = np.zeros(self.nu)
        st = None if state is None else np.ascontiguousarray(state, dtype=np.float64)
        self._L.mjpc_ilqg_action_from_policy(self._h, _dp(a), _dp(st), float(time), int(bool(use_previous))); _check()
        return a

    def values(self):
        o = np.zeros(12); self._L.mjpc_ilqg_values(self._h, _dp(o))
        return dict(action_step=o[0], expected=o[1], improvement=o[2], surprise=o[3], winner=int(o[4]), backward_pass_failed=bool(o[5]),
                    feedback_scaling=o[6], regularization=o[7], regularization_rate=o[8], all_failed=bool(o[9]), dV=o[10:12].copy())

    def timings(self):
        o = np.zeros(6); self._L.mjpc_ilqg_timings(self._h, _dp(o))
        return dict(nominal_us=o[0], derivative_us=o[1], rollouts_us=o[2], policy_update_us=o[3], resample_kernel_us=o[4], rollout_kernel_us=o[5])

    def linesearch_steps(self):
        out = np.zeros(max(self._L.mjpc_ilqg_linesearch_steps(self._h, None), 1)); n = self._L.mjpc_ilqg_linesearch_steps(self._h, _dp(out)); return out[:n]

    def get_policy(self, which=0):
        """which: 0 policy, 1 previous_policy, 2 the nominal candidate -> dict of its first `horizon` knots"""
        H = self._L.mjpc_ilqg_get_policy(self._h, int(which), None, None, None, None, None, None)
        Hn = max(H, 1)
        o = dict(times=np.zeros(Hn), states=np.zeros((Hn, self.ns)), actions=np.zeros((Hn, self.nu)), feedback_gain=np.zeros((Hn, self.nu, self.nd)),
                 action_improvement=np.zeros((Hn, self.nu)))
        fs = C.c_double()
        self._L.mjpc_ilqg_get_policy(self._h, int(which), _dp(o["times"]), _dp(o["states"]), _dp(o["actions"]), _dp(o["feedback_gain"]),
                                     _dp(o["action_improvement"]), C.cast(C.byref(fs), c_double_p))
        o = {k: v[:H] for k, v in o.items()}
        o["feedback_scaling"] = fs.value; o["horizon"] = H
        return o


class iLQSPlanner(_Planner):
    """mjpc_hip::iLQSPlanner (C++) driven from Python; names follow planners/ilqs/planner.h.  `.sampling` and `.ilqg` are ordinary
    SamplingPlanner / iLQGPlanner views of its two members over borrowed handles: they never destroy them."""
    _prefix = "mjpc_ilqs_"
    kSampling, kiLQG = 0, 1
    kMaxSplinePoints = 25

    def Initialize(self, model: dict, task: dict, numerics: dict | None = None, settings: dict | None = None, max_samples=128, max_horizon=512, device=0):
        numerics = numerics or {}; settings = settings or {}
        self.cm = capi.CModel(model, task)
        se = numerics.get("sampling_exploration", 0.1)
        se = list(se) if isinstance(se, (list, tuple)) else [se]
        self._expl = np.array([float(se[0]), float(se[1]) if len(se) > 1 else 0.0])
        self.nu = int(model["nu"]); self.ns = int(model["nq"] + model["nv"] + model["na"]); self.nd = int(2 * model["nv"] + model["na"])
        self.nr = int(task["num_residual"])
        self.max_samples, self.max_horizon = int(max_samples), int(max_horizon)
        s = np.array([float(settings.get(k, v)) for k, v in zip(iLQGPlanner.SETTINGS, iLQGPlanner.DEFAULTS)])
        self.close()
        h = self._L.mjpc_ilqs_create(C.byref(self.cm.c_model), C.byref(self.cm.c_task), _dp(self._expl), int(numerics.get("sampling_trajectories", 10)),
                                     int(numerics.get("sampling_representation", 2)), int(numerics.get("sampling_sliding_plan", 0)),
                                     int(numerics.get("sampling_spline_points", 10)), int(numerics.get("ilqg_num_rollouts", 10)),
                                     int(numerics.get("ilqg_representation", 1)), int(numerics.get("derivative_skip", 0)),
                                     int(bool(settings.get("fused", True))), _dp(s), self.max_samples, self.max_horizon, int(device))
        self._h = C.c_void_p(h)
        self.sampling = self._view(SamplingPlanner, self._L.mjpc_ilqs_sampling(self._h), task)
        self.ilqg = self._view(iLQGPlanner, self._L.mjpc_ilqs_ilqg(self._h), task)
        _check()

    def _view(self, cls, handle, task):
        v = cls.__new__(cls)
        v._L = self._L; v._h = C.c_void_p(handle); v._noise = None
        v.cm = self.cm; v.nu = self.nu; v.ns = self.ns; v.nd = self.nd; v.nr = self.nr; v.ntrace = int(task["num_trace"])
        v.max_samples = self.max_samples; v.max_horizon = self.max_horizon
        v.close = lambda: None
        return v

    def ActionFromPolicy(self, time, use_previous=False, state=None):
        a = np.zeros(self.nu)
        st = None if state is None else np.ascontiguousarray(state, dtype=np.float64)
        self._L.mjpc_ilqs_action_from_policy(self._h, _dp(a), _dp(st), float(time), int(bool(use_previous))); _check()
        return a

    def set_noise_exploration(self, first, second=0.0):
        """sampling's noise_exploration sliders"""
        self._L.mjpc_ilqs_set_noise_exploration(self._h, float(first), float(second))

    def values(self):
        o = np.zeros(6, np.int32); self._L.mjpc_ilqs_values(self._h, o.ctypes.data_as(c_int_p))
        return dict(active_policy=int(o[0]), previous_active_policy=int(o[1]), converted=bool(o[2]), returned_early=bool(o[3]), iterated=bool(o[4]),
                    adopted=bool(o[5]))

    def timings(self):
        o = np.zeros(2); self._L.mjpc_ilqs_timings(self._h, _dp(o))
        return dict(fit_us=o[0], fit_cache_miss=bool(o[1]), sampling=self.sampling.timings(), ilqg=self.ilqg.timings())

    def fitted_knots(self):
        """the knots of the last conversion of iLQG's nominal to sampling's spline, clamped: times [P], values [P, nu]"""
        return self._knots("fitted_knots")

    def sampling_member(self, index, horizon):
        """sampling.trajectory[index] of the last plan step (batch index, not rank)"""
        H = int(horizon)
        o = dict(states=np.zeros((H, self.ns)), actions=np.zeros((H, self.nu)), times=np.zeros(H), residual=np.zeros((H, max(self.nr, 1))))
        tot = C.c_double()
        n = self._L.mjpc_ilqs_sampling_member(self._h, int(index), _dp(o["states"]), _dp(o["actions"]), _dp(o["times"]), _dp(o["residual"]),
                                              C.cast(C.byref(tot), c_double_p)); _check()
        assert n == H, (n, H)
        o["residual"] = o["residual"].ravel()[:H * self.nr].reshape(H, self.nr); o["total_return"] = tot.value
        return o


def ilqs_action_source(previous_active_policy, active_policy, use_previous):
    """iLQSPlanner::ActionSource (host closed form, no GPU needed): 0 sampling's current policy, 1 sampling's previous, 2 iLQG's current, 3 iLQG's previous"""
    return lib().mjpc_ilqs_action_source(int(previous_active_policy), int(active_policy), int(bool(use_previous)))


def ilqs_spline_fit(representation, knot_times, action_times, actions):
    """SplineFit (host closed form, no GPU needed): the least-squares knots [P, nu] of a spline over knot_times through actions [H1, nu] at
    action_times, or None when the normal matrix is singular"""
    kt = np.ascontiguousarray(knot_times, dtype=np.float64); at = np.ascontiguousarray(action_times, dtype=np.float64)
    u = np.ascontiguousarray(actions, dtype=np.float64).reshape(at.size, -1)
    out = np.zeros((kt.size, u.shape[1]))
    rc = lib().mjpc_ilqs_spline_fit(int(representation), int(kt.size), _dp(kt), int(at.size), _dp(at), int(u.shape[1]), _dp(u), _dp(out))
    return out if rc == 0 else None


def ilqg_best_rollout(returns, failures):
    """iLQGPlanner::BestRollout (host closed form, no GPU needed): from the last index down, strict <; -1 when every candidate failed"""
    r = np.ascontiguousarray(returns, dtype=np.float64); f = np.ascontiguousarray(failures, dtype=np.int32)
    return lib().mjpc_ilqg_best_rollout(_dp(r), f.ctypes.data_as(c_int_p), int(r.size))


def gradient_spline_mapping(representation, dim, input_times, output_times):
    """Zero / Linear / CubicSplineMapping::Compute (host closed form, no GPU needed): [(dim * num_output), (dim * num_input)]"""
    ti = np.ascontiguousarray(input_times, dtype=np.float64); to = np.ascontiguousarray(output_times, dtype=np.float64)
    out = np.zeros((int(dim) * to.size, int(dim) * ti.size))
    lib().mjpc_gd_spline_mapping(int(representation), int(dim), _dp(ti), int(ti.size), _dp(to), int(to.size), _dp(out))
    _check()
    return out


def gradient_policy_action(representation, ctrlrange, times, parameters, time):
    """GradientPolicy::Action (host closed form, no GPU needed)"""
    cr = np.ascontiguousarray(ctrlrange, dtype=np.float64).ravel(); nu = cr.size // 2
    t = np.ascontiguousarray(times, dtype=np.float64); p = np.ascontiguousarray(parameters, dtype=np.float64)
    a = np.zeros(nu)
    lib().mjpc_gd_policy_action(int(representation), nu, _dp(cr), _dp(t), _dp(p), int(t.size), float(time), _dp(a))
    return a


def sample_gradient_return_weights(order):
    """the planner's fitness-shaping weights over an order of candidate indices (host closed form, no GPU needed)"""
    o = np.ascontiguousarray(order, dtype=np.int32); w = np.zeros(o.size)
    lib().mjpc_sg_return_weights(o.ctypes.data_as(c_int_p), int(o.size), _dp(w))
    return w


def sample_gradient_step_sizes(steps, max_value=2.0, min_value=1.0e-3):
    """LogScale(max, min, steps) as the planner spaces its gradient candidates (host closed form, no GPU needed)"""
    v = np.zeros(max(int(steps), 1))
    lib().mjpc_sg_log_scale(_dp(v), float(max_value), float(min_value), int(steps))
    return v[:int(steps)]


def testspeed(planner, state, mocap=None, time0=0.0, horizon=None, steps_per_planning_iteration=1, total_time=1.0, device=0, mode=0, mode_time=0.0):
    """mjpc/testspeed.cc:44-129 (`SynchronousPlanningCost`) through the C++ harness: `planner` is a cplanner.SamplingPlanner or
    cplanner.CrossEntropyPlanner / cplanner.SampleGradientPlanner / cplanner.GradientPlanner / cplanner.iLQGPlanner / cplanner.iLQSPlanner that has been Initialize()d / Reset(); the world is stepped on the HIP engine as well."""
    L = lib()
    cm = planner.cm
    m = cm.model
    nsteps = int(np.ceil(total_time / m["timestep"]))
    st = np.ascontiguousarray(state, dtype=np.float64).copy()
    mc = None if (mocap is None or m["nmocap"] == 0) else np.ascontiguousarray(mocap, dtype=np.float64).copy()
    costs = np.zeros(nsteps); out = np.zeros(6); params = np.zeros(max(int(cm.task["num_parameter"]), 1))
    kind = (1 if isinstance(planner, CrossEntropyPlanner) else 2 if isinstance(planner, SampleGradientPlanner) else 3 if isinstance(planner, GradientPlanner)
            else 4 if isinstance(planner, iLQGPlanner) else 5 if isinstance(planner, iLQSPlanner) else 0)
    total = L.mjpc_testspeed_run(C.byref(cm.c_model), C.byref(cm.c_task), planner._h, kind, _dp(st), _dp(mc), float(time0), int(horizon),
                                 int(steps_per_planning_iteration), float(total_time), int(device), _dp(costs), _dp(out), int(mode), float(mode_time), _dp(params))
    _check()
    return dict(total_cost=total, average_cost=out[0], wall_seconds=out[1], realtime_factor=out[2], plan_seconds=out[3],
                plan_steps=int(out[4]), failure=bool(out[5]), cost_per_step=costs, state=st, mocap=mc, parameters=params)


class RobustPlanner(_Planner):
    """mjpc_hip::RobustPlanner (C++) driven from Python; mirrors planners/robust/robust_planner.h:31-80 over a SamplingPlanner."""
    _prefix = "mjpc_robust_"

    def Initialize(self, model: dict, task: dict, numerics: dict | None = None, max_samples=128, max_horizon=512, device=0):
        numerics = numerics or {}
        self.cm = capi.CModel(model, task)
        se = numerics.get("sampling_exploration", 0.1)
        se = list(se) if isinstance(se, (list, tuple)) else [se]
        self._expl = np.array([float(se[0]), float(se[1]) if len(se) > 1 else 0.0])
        self.nu = int(model["nu"]); self.ns = int(model["nq"] + model["nv"] + model["na"])
        self.close()
        h = self._L.mjpc_robust_create(C.byref(self.cm.c_model), C.byref(self.cm.c_task), _dp(self._expl),
                                       int(numerics.get("sampling_trajectories", 10)), int(numerics.get("sampling_representation", 2)),
                                       int(numerics.get("sampling_spline_points", 512)), int(numerics.get("robust_repetitions", 5)),
                                       int(numerics.get("robust_candidates", -1)), float(numerics.get("robust_xfrc", 0.1)),
                                       float(numerics.get("robust_xfrc_rate", 0.1)), int(max_samples), int(max_horizon), int(device))
        self._h = C.c_void_p(h)
        _check()
        # a non-owning view of the delegate for the mjpc_planner_* accessors
        self.delegate = SamplingPlanner.__new__(SamplingPlanner)
        self.delegate._L = self._L; self.delegate._h = C.c_void_p(self._L.mjpc_robust_delegate(self._h)); self.delegate._noise = None
        self.delegate.cm = self.cm; self.delegate.nu = self.nu; self.delegate.ns = self.ns
        self.delegate.nr = int(task["num_residual"]); self.delegate.ntrace = int(task["num_trace"])
        self.delegate.max_samples = int(max_samples); self.delegate.max_horizon = int(max_horizon)
        self.delegate.close = lambda: None

    def Reset(self, horizon=0): self._L.mjpc_robust_reset(self._h, int(horizon or 0))

    def set_seed(self, delegate_seed, robust_seed, plan_iter=0):
        self._L.mjpc_robust_set_seed(self._h, int(delegate_seed), int(robust_seed), int(plan_iter))

    def ActionFromPolicy(self, time):
        a = np.zeros(self.nu)
        self._L.mjpc_robust_action_from_policy(self._h, _dp(a), float(time)); _check()
        return a

    def last(self):
        o = np.zeros(3, np.int32)
        self._L.mjpc_robust_last(self._h, o.ctypes.data_as(c_int_p), None, None)
        nc, rep = int(o[1]), int(o[2])
        scores = np.zeros(max(nc, 1)); noisy = np.zeros(max(nc * rep, 1))
        self._L.mjpc_robust_last(self._h, o.ctypes.data_as(c_int_p), _dp(scores), _dp(noisy))
        return dict(best_candidate=int(o[0]), scores=scores[:nc], noisy_returns=noisy[:nc * rep].reshape(nc, rep) if nc else noisy[:0])
