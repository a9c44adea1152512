"""numpy mirror of the iLQG planner loop (mjpc/planners/ilqg/planner.cc:156-223, 377-615; TEST INFRASTRUCTURE ONLY) over callables for the
rollouts and the derivative pass, written from the reference and include/mjpc_hip_planner.h, not from planner.cc of this project."""
import math

import numpy as np

import riccati_mirror as rm


def log_scale(max_value, min_value, steps):
    step = (math.log(max_value) - math.log(min_value)) / max(steps - 1, 1)
    return [math.exp(math.log(min_value) + i * step) for i in range(steps)]


def best_rollout(returns, failures):
    best, value = -1, 0.0
    for j in range(len(returns) - 1, -1, -1):
        if failures[j]:
            continue
        if best == -1 or returns[j] < value:
            value, best = returns[j], j
    return best


def update_regularization(reg, rate, factor, reg_min, reg_max, z, s):
    bad = lambda v: math.isnan(v) or v > 1e10 or v < -1e10          # noqa: E731
    if bad(z) or bad(s):
        return rm.scale_regularization(reg, rate, factor * factor, reg_min, reg_max)
    if z > 0.5 or s > 0.3:
        return rm.scale_regularization(reg, rate, 1.0 / factor, reg_min, reg_max)
    if z < 0.1 or s < 0.06:
        return rm.scale_regularization(reg, rate, factor, reg_min, reg_max)
    return reg, rate


class ILQGPlannerMirror:
    """rollouts(state, time, H, policy dict, mode, representation, action_step, feedback_scaling, improvement) -> dict(returns, failure, rows(i));
    backward(x, u, times, residual, regularization, rate) -> dict(k, K, dV, status, regularization, regularization_rate, failure)"""

    def __init__(self, model, rollouts, backward, H_max, num_trajectory=10, representation=1, min_linesearch_step=1e-3, min_regularization=1e-6,
                 max_regularization=1e6):
        self.m = model; self.rollouts = rollouts; self.backward = backward
        nq, nv, na, nu = (int(model[k]) for k in ("nq", "nv", "na", "nu"))
        self.N = num_trajectory; self.rep = representation; self.min_step = min_linesearch_step
        self.reg_min, self.reg_max = min_regularization, max_regularization
        z = lambda *s: np.zeros(s)          # noqa: E731
        self.policy = dict(times=z(H_max), states=z(H_max, nq + nv + na), actions=z(H_max, nu), K=z(H_max, nu, 2 * nv + na), k=z(H_max, nu), feedback_scaling=1.0)
        self.previous = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in self.policy.items()}
        self.reg, self.rate, self.factor = 1.0, 1.0, 2.0
        self.feedback_scaling = 1.0; self.winner = -1; self.backward_failed = False
        self.action_step = self.expected = self.improvement = self.surprise = 0.0

    def set_state(self, state, time):
        self.state = np.asarray(state, float).copy(); self.time = float(time)

    def _steps(self):
        return np.array(log_scale(1.0, self.min_step, self.N - 1) + [0.0])

    def _cut(self, H):
        return {k: (v[:H] if hasattr(v, "shape") else v) for k, v in self.policy.items()}

    def nominal(self, H):
        self.steps = self._steps()
        pol = self._cut(H)
        o = self.rollouts(self.state, self.time, H, pol, 1, self.rep, np.zeros(self.N), self.steps, False)
        self.returns = o["returns"].copy()
        best = best_rollout(o["returns"], o["failure"])
        if best == -1:
            self.cand = dict(states=pol["states"].copy(), actions=pol["actions"].copy(), times=pol["times"].copy(), residual=None, ret=None)
            self.feedback_scaling = 0.0
        else:
            r = o["rows"](best)
            a = r["actions"].copy(); a[H - 1] = a[H - 2]
            self.cand = dict(states=r["states"], actions=a, times=r["times"], residual=r["residual"], ret=float(o["returns"][best]))
            self.feedback_scaling = float(self.steps[best])
        self.cand["K"] = pol["K"].copy(); self.cand["k"] = pol["k"].copy()

    def iteration(self, H):
        c = self.cand
        previous_return = c["ret"]
        self.steps = self._steps()
        b = self.backward(c["states"], c["actions"], c["times"], c["residual"], self.reg, self.rate)
        self.reg, self.rate = b["regularization"], b["regularization_rate"]
        self.backward_failed = bool(b["status"][0] == 0 or np.any(b["failure"]))
        if self.backward_failed:
            return
        c["K"], c["k"] = b["K"][:H].copy(), b["k"][:H].copy()
        self.dV = b["dV"].copy()
        pol = dict(times=c["times"], states=c["states"], actions=c["actions"], K=c["K"], k=c["k"])
        o = self.rollouts(self.state, self.time, H, pol, 0, self.rep, self.steps, np.ones(self.N), True)
        self.returns = o["returns"].copy()
        best = best_rollout(o["returns"], o["failure"])
        if best == -1:
            return
        self.winner = best
        r = o["rows"](best)
        a = r["actions"].copy(); a[H - 1] = a[H - 2]
        self.best = dict(states=r["states"], actions=a, times=r["times"], ret=float(o["returns"][best]))
        self.action_step = float(self.steps[best])
        if best == 0:        # the reference has overwritten slot 0 with the winning rollout by the time it copies the policy
            new = dict(times=r["times"].copy(), states=r["states"].copy(), actions=a.copy())
        else:
            new = dict(times=c["times"].copy(), states=c["states"].copy(), actions=c["actions"] + c["k"] * self.action_step)
        self.expected = -1.0 * self.action_step * (self.dV[0] + self.action_step * self.dV[1]) + 1.0e-16
        self.improvement = previous_return - self.best["ret"]
        self.surprise = min(max(0.0, self.improvement / self.expected), 2.0)
        self.reg, self.rate = update_regularization(self.reg, self.rate, self.factor, self.reg_min, self.reg_max, self.surprise, self.action_step)
        self.previous = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in self.policy.items()}
        for k in ("times", "states", "actions"):
            self.policy[k][:H] = new[k]
        self.policy["K"][:H] = c["K"]; self.policy["k"][:H] = c["k"]
        self.policy["feedback_scaling"] = 1.0

    def optimize(self, H):
        self.nominal(H)
        self.iteration(H)

    def action(self, time, state=None, previous=False, H=None):
        p = self.previous if previous else self.policy
        H = H or len(p["times"])
        return rm.policy_action(self.m, p["times"][:H], p["states"][:H], p["actions"][:H], p["K"][:H], time, state, self.rep,
                                feedback_scaling=p["feedback_scaling"])
