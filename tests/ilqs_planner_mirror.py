"""numpy mirror of the iLQS planner (mjpc/planners/ilqs/planner.cc:33-263; TEST INFRASTRUCTURE ONLY): host_mirror.SamplingPlanner and
ilqg_planner_mirror.ILQGPlannerMirror taking turns over a backend, and the spline fit of the conversion as a sequential computation by the
summation rule (every sum starts at 0.0 and takes its index ascending, one rounded product and one rounded add per term).  Written from the
reference and include/mjpc_hip_planner.h, not from planner.cc of this project."""
import math

import numpy as np

import gradient_planner_mirror as gm
from host_mirror import TimeSpline

kSampling, kiLQG = 0, 1
kMaxSplinePoints = 25
# ActionFromPolicy's source (ilqs/planner.cc:228-253)
SAMPLING_CURRENT, SAMPLING_PREVIOUS, ILQG_CURRENT, ILQG_PREVIOUS = 0, 1, 2, 3


class SingularFit(Exception):
    pass


def action_source(previous_active, active, use_previous):
    if use_previous:
        if previous_active == kSampling:
            return SAMPLING_PREVIOUS
        return ILQG_CURRENT if active == kSampling else ILQG_PREVIOUS
    return SAMPLING_CURRENT if active == kSampling else ILQG_CURRENT


def fit_operator(representation, knot_times, action_times):
    """W = (M'M)^-1 M' [P, H1] of the scalar mapping M [H1, P]: the normal matrix, its lower Cholesky factor row by row, then forward and
    back substitution per column.  Python floats: every operation is one IEEE double operation."""
    M = gm.spline_mapping(representation, 1, knot_times, action_times).tolist()
    H1, P = len(M), len(knot_times)
    L = [[0.0] * P for _ in range(P)]
    for i in range(P):
        for j in range(i + 1):
            acc = 0.0
            for t in range(H1):
                acc += M[t][i] * M[t][j]
            L[i][j] = acc
    for i in range(P):
        for j in range(i):
            acc = 0.0
            for k in range(j):
                acc += L[i][k] * L[j][k]
            L[i][j] = (L[i][j] - acc) / L[j][j]
        acc = 0.0
        for k in range(i):
            acc += L[i][k] * L[i][k]
        pivot = L[i][i] - acc
        if not (pivot > 0.0) or not math.isfinite(pivot):
            raise SingularFit(f"pivot {i}: {pivot}")
        L[i][i] = math.sqrt(pivot)
    W = np.zeros((P, H1))
    for t in range(H1):
        y = [0.0] * P; x = [0.0] * P
        for i in range(P):
            acc = 0.0
            for k in range(i):
                acc += L[i][k] * y[k]
            y[i] = (M[t][i] - acc) / L[i][i]
        for i in range(P - 1, -1, -1):
            acc = 0.0
            for k in range(i + 1, P):
                acc += L[k][i] * x[k]
            x[i] = (y[i] - acc) / L[i][i]
        for i in range(P):
            W[i, t] = x[i]
    return W


def fit_apply(W, actions):
    W = np.asarray(W, float).tolist(); u = np.asarray(actions, float).reshape(len(W[0]), -1).tolist()
    P, H1, nu = len(W), len(W[0]), len(u[0])
    out = np.zeros((P, nu))
    for p in range(P):
        for j in range(nu):
            acc = 0.0
            for t in range(H1):
                acc += W[p][t] * u[t][j]
            out[p, j] = acc
    return out


def spline_fit(representation, knot_times, action_times, actions):
    """knots [P, nu], or None when singular"""
    try:
        return fit_apply(fit_operator(representation, knot_times, action_times), actions)
    except SingularFit:
        return None


class SplineConversion:
    """the conversion of ilqs/planner.cc:96-161 with its cache: W is recomputed only when (H - 1, P, representation) changed since the
    last conversion, and belongs to the times of the conversion that filled it"""

    def __init__(self, ctrlrange, timestep):
        self.cr = np.asarray(ctrlrange, float).reshape(-1, 2); self.timestep = float(timestep)
        self.key = None; self.W = None; self.cache_miss = False

    def reset(self):
        self.key = None

    def knot_times(self, time, horizon, P):
        shift = max((horizon - 1) * self.timestep / (P - 1), 1.0e-5)
        out = []; t = float(time)
        for _ in range(P):
            out.append(t); t += shift                      # repeated addition, like the reference
        return out

    def convert(self, representation, time, horizon, P, action_times, actions):
        """-> (knot times [P], clamped knots [P, nu]); SingularFit when the factorisation fails (nothing cached then)"""
        H1 = horizon - 1
        kt = self.knot_times(time, horizon, P)
        key = (H1, P, representation)
        self.cache_miss = key != self.key
        if self.cache_miss:
            self.key = None
            self.W = fit_operator(representation, kt, [float(v) for v in action_times[:H1]])
            self.key = key
        theta = fit_apply(self.W, np.asarray(actions, float)[:H1])
        return kt, np.minimum(np.maximum(theta, self.cr[:, 0]), self.cr[:, 1])


class ILQSPlannerMirror:
    """sampling: a host_mirror.SamplingPlanner (Initialize / Allocate / Reset done, on its own backend); ilqg: an ILQGPlannerMirror; P: the
    sampling spline's knots.  Refusals of Initialize (header): P < 2, P > 25, zero-order representation."""

    def __init__(self, model, sampling, ilqg, P):
        if P < 2 or P > kMaxSplinePoints or sampling.interpolation_ == 0:
            raise ValueError("iLQS: refused")
        self.m = model; self.sampling = sampling; self.ilqg = ilqg; self.P = P
        self.conversion = SplineConversion(model["actuator_ctrlrange"], model["timestep"])
        self.active = self.previous_active = kSampling
        self.converted = self.returned_early = self.iterated = self.adopted = False
        self.fitted = None

    def set_state(self, state, mocap, time):
        self.sampling.SetState(state, mocap, None, time)
        self.ilqg.set_state(state, time)

    def _member0(self, H):
        s = self.sampling
        r = s.backend.candidate(0, H, len(s._last_kt))
        return dict(states=r["states"].copy(), actions=r["actions"].copy(), times=r["times"].copy(), residual=r["residual"].copy(), ret=float(s.returns[0]))

    def optimize(self, H):
        s, q = self.sampling, self.ilqg
        self.converted = self.returned_early = self.iterated = self.adopted = False
        self.previous_active = self.active
        if self.previous_active == kiLQG:
            q.nominal(H)
            kt, knots = self.conversion.convert(s.policy.plan.Interpolation(), s.time, H, self.P, q.cand["times"], q.cand["actions"])
            self.fitted = (np.array(kt), knots)
            plan = TimeSpline(self.m["nu"], s.policy.plan.Interpolation())
            for t, v in zip(kt, knots):
                plan.AddNode(t, v)
            s.policy.plan = plan
            self.converted = True
        s.OptimizePolicy(H)
        reference = s.returns[0] if self.previous_active == kSampling else q.cand["ret"]
        if s.winner > 0 and s.returns[s.winner] < reference:
            self.active = kSampling
            self.returned_early = True
            return
        if self.previous_active == kSampling:
            c = self._member0(H)
            c["actions"][H - 1] = c["actions"][H - 2]
            c["K"] = np.zeros((H,) + q.policy["K"].shape[1:]); c["k"] = np.zeros((H,) + q.policy["k"].shape[1:])
            q.cand = c
        before = q.previous
        q.iteration(H)
        self.iterated = True
        self.adopted = q.previous is not before          # iteration() replaces `previous` exactly when it adopts a policy
        if not self.adopted:
            return
        reference = s.returns[s.winner] if self.previous_active == kSampling else q.returns[0]
        if q.best["ret"] < reference:
            self.active = kiLQG

    def action(self, time, state=None, use_previous=False, H=None):
        src = action_source(self.previous_active, self.active, use_previous)
        if src == SAMPLING_CURRENT:
            return self.sampling.ActionFromPolicy(time, False)
        if src == SAMPLING_PREVIOUS:
            return self.sampling.ActionFromPolicy(time, True)
        return self.ilqg.action(time, state, previous=src == ILQG_PREVIOUS, H=H)

    def best(self):
        """(states, total_return) of the active member's best trajectory"""
        if self.active == kSampling:
            b = self.sampling.BestTrajectory()
            return b.states, b.total_return
        return self.ilqg.best["states"], self.ilqg.best["ret"]
