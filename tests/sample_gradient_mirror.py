"""TEST INFRASTRUCTURE: a Python restatement of mjpc::SampleGradientPlanner (planners/sample_gradient/planner.cc:169-493) over a
plan backend (the CPU oracle in the tests).  The product's planner is the C++ class in csrc/planner.cc, whose batch and gradient sum
run on the HIP engine; this mirror only exists so that the tests can hold it against an independent implementation.

One plan step = two backend calls: rows [0, n_noisy) with noise_std (absolute noise, row 0 un-noised), rows [n_noisy, N) with
candidate_knots.  The standard normals come from oracle_noise (the device's Philox stream, test_device_philox_matches_oracle_noise),
the noise history is a numpy array, the gradient a plain sequential loop."""
import math

import numpy as np

import oracle_lib as ol
from host_mirror import SamplingPolicy, TimeSpline

P_MAX = 36          # the engine's spline capacity: a history slot holds P_MAX * nu normals
kNominal, kPerturb, kGradient = 0, 1, 2


def return_weights(order, n_noisy):
    """planner.cc:437-449: fitness shaping over the candidate INDICES in order[:n_noisy] (not their ranks)"""
    f0 = math.log(0.5 * n_noisy + 1.0)
    den = 0.0
    for i in range(n_noisy):
        den += max(0.0, f0 - math.log(int(order[i]) + 1))
    return np.array([max(0.0, f0 - math.log(int(order[i]) + 1)) / den - 1.0 / n_noisy for i in range(n_noisy)])


def log_scale(max_value, min_value, steps):
    """utilities.cc:802-808"""
    step = (math.log(max_value) - math.log(min_value)) / max(steps - 1, 1)
    v = np.array([math.exp(math.log(min_value) + i * step) for i in range(steps)])
    v[:1] = min_value            # the scale starts at min_value itself (exp(log(1e-3)) is one ulp above 1e-3)
    return v


def sequential_gradient(hist, slot, scale, PN):
    """planner.cc:452-459: gradient = 0; gradient += noise[slot[i]] * scale[i] in ascending i, every product and sum rounded"""
    g = np.zeros(PN)
    for i in range(len(slot)):
        g = g + hist[slot[i], :PN] * scale[i]
    return g


def order_by_return(returns):
    """(return, index), lowest index first; non-finite returns last"""
    r = np.where(np.isfinite(returns), returns, np.inf)
    return np.argsort(r, kind="stable")


class SampleGradientMirror:
    def __init__(self, backend, model, task, numerics, max_samples=None):
        self.backend = backend; self.model = model; self.task = task
        self.noise_exploration = float(numerics.get("sampling_exploration", 0.1))
        self.N = int(numerics.get("sampling_trajectories", 10))
        self.num_gradient = int(numerics.get("sample_gradient_trajectories", 0))
        self.gradient_filter = float(numerics.get("sample_gradient_filter", 1.0))
        self.interp = int(numerics.get("sampling_representation", 0))
        self.P = int(numerics.get("sampling_spline_points", 512))
        self.nu = model["nu"]
        self.max_samples = int(max_samples or self.N)
        self.seed = 0x5EED; self.plan_iter = 0; self.injected_noise = None
        self.policy = SamplingPolicy(model, self.P); self.resampled = SamplingPolicy(model, self.P)

    def Reset(self, horizon, initial_repeated_action=None):
        self.policy.Reset(horizon, initial_repeated_action); self.resampled.Reset(horizon, initial_repeated_action)
        self.candidate = [SamplingPolicy(self.model, self.P) for _ in range(self.max_samples)]      # Reset(horizon): empty plans
        self.hist = np.zeros((self.max_samples, P_MAX * self.nu))
        self.gradient = np.zeros(P_MAX * self.nu); self.gradient_previous = np.zeros(P_MAX * self.nu)
        self.return_weight = np.zeros(0); self.step_size = np.zeros(0)
        self.order = np.arange(self.max_samples)
        self.time = 0.0; self.improvement = 0.0; self.winner = 0; self.winner_type = kNominal

    def SetState(self, state, mocap, userdata, time):
        self.state = np.array(state, float); self.mocap = mocap; self.time = float(time)

    def _resample(self, pol, H, P):
        """ResamplePolicy, planner.cc:302-326"""
        t = self.time; shift = max((H - 1) * self.model["timestep"] / (P - 1), 1.0e-5)
        scratch = TimeSpline(self.nu, pol.plan.Interpolation())
        for _ in range(P):
            scratch.AddNode(t, pol.Action(t)); t += shift
        pol.plan = scratch; pol.num_spline_points = P

    def OptimizePolicy(self, H):
        nu, P, N = self.nu, self.P, self.N
        self.num_gradient = min(self.num_gradient, N - 1)
        ng = self.num_gradient; nn = N - ng
        self.policy.plan.SetInterpolation(self.interp)
        self.resampled.CopyFrom(self.policy)
        self._resample(self.resampled, H, P)
        for i in range(ng):
            self._resample(self.candidate[nn + i], H, P)
        times, nominal = self.resampled.plan.arrays()
        interp = self.resampled.plan.Interpolation()
        # ----- rollouts: noisy rows, then explicit rows
        if self.injected_noise is not None:
            eps = np.asarray(self.injected_noise, float).reshape(N, P, nu)
        else:
            eps, _ = ol.noise(self.seed, self.plan_iter, 0, N, P, nu)
        std = np.full(P * nu, self.noise_exploration)
        common = dict(state=self.state, mocap=self.mocap, time=self.time, knot_times=times, knot_values=nominal, interpolation=interp,
                      num_trajectory=N, horizon=H, sigma=(0.0, 0.0), seed=self.seed, stream=self.plan_iter)
        a = self.backend.plan(noise_eps=eps, noise_std=std, nominal_index=0, candidate_offset=0, num_local=nn, **common)
        alla = self.backend._all
        returns = np.array(a["returns"]); failure = np.array(a["failure"]); knots = alla["knots"].reshape(nn, P, nu); states = alla["states"]
        if ng:
            table = np.zeros((N, P, nu))
            for i in range(nn, N):
                table[i] = self.candidate[i].plan.arrays()[1]
            b = self.backend.plan(candidate_knots=table, candidate_offset=nn, num_local=ng, **common)
            allb = self.backend._all
            returns = np.concatenate([returns, b["returns"]]); failure = np.concatenate([failure, b["failure"]])
            knots = np.concatenate([knots, allb["knots"].reshape(ng, P, nu)]); states = np.concatenate([states, allb["states"]])
        self.plan_iter += 1
        self.returns = returns; self.failure = failure; self.knots = knots; self.states = states
        self.hist[1:nn, :P * nu] = eps[1:nn].reshape(nn - 1, P * nu)         # AddNoiseToPolicy: rows 0 < i < n_noisy, first P * nu only
        # ----- update policy
        self.order[:N] = order_by_return(returns)
        self.full_order = self.order[:N].copy()
        self.winner = int(self.order[0]) if returns[self.order[0]] < returns[0] else 0
        self.winner_type = (kPerturb if self.winner < nn else kGradient) if self.winner > 0 else kNominal
        for i in range(nn):                                                   # candidate_policy[i] as rolled out
            c = self.candidate[i]
            c.plan = TimeSpline(nu, interp); c.num_spline_points = P
            for t in range(P):
                c.plan.AddNode(times[t], knots[i, t])
        self.policy.plan = self.candidate[self.winner].plan.copy()
        self.improvement = max(returns[0] - returns[self.winner], 0.0)
        self.winner_states = states[self.winner]
        self._gradient_candidates(N, ng, P)

    def _gradient_candidates(self, N, ng, P):
        """GradientCandidates, planner.cc:401-493"""
        if ng < 1:
            return
        nu = self.nu; PN = P * nu; nn = N - ng
        self.gradient_previous[:PN] = self.gradient[:PN]
        if len(self.return_weight) != nn:
            self.order[:nn] = order_by_return(self.returns[:nn])
            self.return_weight = return_weights(self.order, nn)
        self.slots = self.order[:nn].copy()
        self.scale = np.array([self.return_weight[i] / nn for i in range(nn)])
        self.gradient[:] = 0.0
        self.gradient[:PN] = sequential_gradient(self.hist, self.slots, self.scale, PN)
        if len(self.step_size) != ng:
            self.step_size = log_scale(2.0, 1.0e-3, ng)
        gf = self.gradient_filter
        r = self.model["actuator_ctrlrange"].reshape(-1, 2)
        for i in range(nn, N):
            c = self.candidate[i]
            c.CopyFrom(self.resampled)
            scaling = self.step_size[i - nn] / self.noise_exploration
            for t in range(c.plan.Size()):
                n = c.plan.values_[t]
                n = n + self.gradient[t * nu:(t + 1) * nu] * (-scaling * gf)
                n = n + self.gradient_previous[t * nu:(t + 1) * nu] * (-scaling * (1.0 - gf))
                c.plan.values_[t] = np.minimum(np.maximum(n, r[:, 0]), r[:, 1])

    def min_rank_gap(self):
        """smallest relative gap between adjacent sorted returns of the last plan's non-failed candidates, candidates whose knots are
        bit-identical (one policy, one return) counted once; inf with fewer than two distinct policies"""
        N = len(self.returns)
        ok = [i for i in self.full_order if self.failure[i] == 0]
        gap = np.inf
        for a, b in zip(ok[:-1], ok[1:]):
            if np.array_equal(self.knots[a], self.knots[b]):
                assert self.returns[a] == self.returns[b]
                continue
            gap = min(gap, abs(self.returns[b] - self.returns[a]) / max(abs(self.returns[a]), abs(self.returns[b]), 1e-300))
        return gap


class ResidualRefBackend:
    """OracleBackend for the registry tasks whose residuals the oracle does not write (Allegro, OP3): the oracle rolls the dynamics
    out, tests/task_ref.py turns its states and actions into residual rows and costs, a candidate's return is its mean cost - the
    engine's definition (test_gpu_registry_allegro_op3.py)."""

    def __init__(self, model, task, nthreads=8):
        from oracle_backend import OracleBackend
        from task_ref import TaskRef
        self.inner = OracleBackend(model, task, nthreads=nthreads)
        self.ref = TaskRef(model, task)
        self.nq, self.nv = model["nq"], model["nv"]
        self._all = None

    def plan(self, **kw):
        out = self.inner.plan(**kw)
        r = self.inner._all
        assert not r["failure"].any()
        S = r["states"]
        n, H = S.shape[:2]
        S2 = S.reshape(n * H, -1)
        res = np.asarray(self.ref.residual(S2[:, :self.nq], S2[:, self.nq:self.nq + self.nv], r["actions"].reshape(n * H, -1)))
        r["residual"] = res.reshape(n, H, -1)
        r["costs"] = np.asarray(self.ref.cost(r["residual"]))
        r["returns"] = r["costs"].mean(1)
        self._all = r
        out["returns"] = r["returns"]
        return out
