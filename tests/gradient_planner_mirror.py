"""numpy restatement of the gradient planner (TEST INFRASTRUCTURE ONLY), written from the reference text (policy, spline mappings and
the planner loop over a backend are at the end of the file):
    norm_derivatives     Norm(g, H, x, params, n, type), mjpc/norm.cc:50-210
    cost_derivatives     CostDerivatives::DerivativeStep / Compute, mjpc/planners/cost_derivatives.cc:77-224
    gradient_backward    Gradient::GradientStep / Compute, mjpc/planners/gradient/gradient.cc:43-108
Scalars are Python floats (IEEE doubles, every operation rounded on its own, libm for pow / exp / cosh / sinh); the matrix products
follow the summation rule of include/mjpc_hip.h (mjpc_hip_cost_derivatives): a contraction starts at 0.0 and adds one rounded product
per ascending contraction index.  numpy's elementwise `acc = acc + a * b` is exactly that for every output entry at once (a multiply
ufunc, then an add ufunc: no fused multiply-add)."""
import math

import numpy as np

MINVAL = 1e-15
RISK_NEUTRAL = 1e-6        # kRiskNeutralTolerance


def _sign(x):
    return 1.0 if x > 0 else (-1.0 if x < 0 else 0.0)


def norm_derivatives(x, params, typ):
    """(y, g [n], H [n, n]) of one term"""
    x = [float(v) for v in x]; n = len(x)
    prm = [float(v) for v in params] + [0.0, 0.0]
    p, q = prm[0], prm[1]
    g = [0.0] * n
    H = np.zeros((n, n))
    y = 0.0
    if typ == -1:                      # kNull
        y = x[0]; g[0] = 1.0
    elif typ == 0:                     # kQuadratic
        for i in range(n):
            y += x[i] * x[i]
        y *= 0.5
        for i in range(n):
            g[i] = x[i]; H[i, i] = 1.0
    elif typ == 1:                     # kL22
        c = 0.0
        for i in range(n):
            c += x[i] * x[i]
        a = math.pow(c, q / 2) + math.pow(p, q)
        s = math.pow(a, 1 / q)
        y = s - p
        d = math.pow(c, q / 2 - 1)
        b = s / a * d
        for i in range(n):
            g[i] = b * x[i]
        c = (1 - q) * d / a + (q - 2) / max(c, MINVAL)
        for i in range(n):
            for j in range(n):
                H[j, i] = b * ((1.0 if i == j else 0.0) + x[i] * x[j] * c)
    elif typ == 2:                     # kL2
        dot = 0.0
        for i in range(n):
            dot += x[i] * x[i]
        s = math.sqrt(dot + p * p)
        y = s - p
        if s:
            inv = 1 / s
            for i in range(n):
                g[i] = x[i] * inv
            for i in range(n):
                for j in range(n):
                    H[j, i] = ((1.0 if i == j else 0.0) - g[i] * g[j]) / s
    elif typ == 3:                     # kCosh
        for i in range(n):
            y += p * p * (math.cosh(x[i] / p) - 1.0)
            g[i] = p * math.sinh(x[i] / p)
            H[i, i] = math.cosh(x[i] / p)
    elif typ == 5:                     # kPowerLoss
        for i in range(n):
            s = abs(x[i])
            y += math.pow(s, p)
            g[i] = _sign(x[i]) * p * math.pow(s, p - 1)
            H[i, i] = (p - 1) * p * math.pow(s, p - 2)
    elif typ == 6:                     # kSmoothAbsLoss
        for i in range(n):
            s = math.sqrt(x[i] * x[i] + p * p)
            y += s - p
            g[i] = x[i] / s if s else 0.0
            H[i, i] = (1 - g[i] * g[i]) / s if s else 0.0
    elif typ == 7:                     # kSmoothAbs2Loss
        for i in range(n):
            a = abs(x[i])
            d = math.pow(a, q)
            e = d + math.pow(p, q)
            s = math.pow(e, 1 / q)
            y += s - p
            c = s * math.pow(a, q - 2) / e
            g[i] = c * x[i]
            H[i, i] = c * (q - 1) * (1 - d / e)
    elif typ == 8:                     # kRectifyLoss
        for i in range(n):
            if p > 0:
                s = math.exp(x[i] / p)
                y += p * math.log(1 + s)
                g[i] = s / (1 + s)
                H[i, i] = s / (p * (1 + s) * (1 + s))
            else:
                y += x[i] if x[i] > 0 else 0.0
                g[i] = 1.0 if x[i] > 0 else 0.0
    else:
        raise ValueError("unknown norm type %d" % typ)
    return y, np.array(g), H


def _matTvec(M, v):
    """M' v: ascending row of M"""
    acc = np.zeros(M.shape[1])
    for r in range(M.shape[0]):
        acc = acc + M[r] * v[r]
    return acc


def _matmat(Hm, J):
    """Hm J, ascending contraction index"""
    S = np.zeros((Hm.shape[0], J.shape[1]))
    for q in range(Hm.shape[1]):
        S = S + Hm[:, q:q + 1] * J[q:q + 1, :]
    return S


def _matTmat(J, S):
    """J' S, ascending row"""
    G = np.zeros((J.shape[1], S.shape[1]))
    for r in range(J.shape[0]):
        G = G + J[r][:, None] * S[r][None, :]
    return G


def cost_derivatives(task, residual, Cm, Dm, last_is_terminal=False, hessians=True):
    """dict(cr, cx, cu[, cxx, cuu, cxu]) over the T knots of residual [T, nr], Cm [T, nr, nd], Dm [T, nr, nu]"""
    nr = int(task["num_residual"])
    r = np.asarray(residual, float).reshape(-1, nr); T = r.shape[0]
    Cm = np.asarray(Cm, float).reshape(T, nr, -1); nd = Cm.shape[2]
    Dm = np.asarray(Dm, float).reshape(T, nr, -1); nu = Dm.shape[2]
    n = nd + nu
    dims = [int(v) for v in task["dim_norm_residual"]]; norms = [int(v) for v in task["norm"]]
    npar = [int(v) for v in task["num_norm_parameter"]]; prm = [float(v) for v in np.asarray(task["norm_parameter"]).ravel()]
    weights = [float(v) for v in task["weight"]]; risk = float(task["risk"])
    o = dict(cr=np.zeros((T, nr)), cx=np.zeros((T, nd)), cu=np.zeros((T, nu)))
    if hessians:
        o.update(cxx=np.zeros((T, nd, nd)), cuu=np.zeros((T, nu, nu)), cxu=np.zeros((T, nd, nu)))
    for t in range(T):
        term = bool(last_is_terminal) and t == T - 1
        J = np.concatenate([Cm[t], np.zeros((nr, nu)) if term else Dm[t]], axis=1)
        live = nd if term else n                  # a terminal knot has no D: everything about u stays zero
        g_acc = np.zeros(n); G_acc = np.zeros((n, n))
        c = 0.0
        fs = ps = 0
        for i in range(len(dims)):
            ni = dims[i]; w = weights[i] / T
            y, g, Hm = norm_derivatives(r[t, fs:fs + ni], prm[ps:ps + npar[i]], norms[i])
            o["cr"][t, fs:fs + ni] = g
            Ji = J[fs:fs + ni, :live]
            g_acc[:live] = g_acc[:live] + w * _matTvec(Ji, g)
            if hessians:
                S = _matmat(Hm, Ji) if norms[i] in (1, 2) else np.diag(Hm)[:, None] * Ji
                G_acc[:live, :live] = G_acc[:live, :live] + w * _matTmat(Ji, S)
            c += w * y
            fs += ni; ps += npar[i]
        if abs(risk) >= RISK_NEUTRAL:
            s = math.exp(risk * c)
            g_acc = g_acc * s                      # cx, cu first ...
            if hessians:                           # ... and the outer products from the scaled vectors (the reference's order)
                G_acc = G_acc * s + (g_acc[:, None] * g_acc[None, :]) * (risk * s)
        o["cx"][t] = g_acc[:nd]; o["cu"][t] = g_acc[nd:]
        if hessians:
            o["cxx"][t] = G_acc[:nd, :nd]; o["cxu"][t] = G_acc[:nd, nd:]; o["cuu"][t] = G_acc[nd:, nd:]
    return o


def gradient_backward(A, B, cx, cu):
    """dict(k [T, nu], Vx [T, nd], Qx [T-1, nd], Qu [T-1, nu], dV [2]); A [>= T-1, nd, nd], B [>= T-1, nd, nu]"""
    cx = np.asarray(cx, float); cu = np.asarray(cu, float)
    T, nd = cx.shape; nu = cu.shape[1]
    A = np.asarray(A, float).reshape(-1, nd, nd); B = np.asarray(B, float).reshape(-1, nd, nu)
    k = np.zeros((T, nu)); Vx = np.zeros((T, nd)); Qx = np.zeros((T - 1, nd)); Qu = np.zeros((T - 1, nu)); dV = np.zeros(2)
    Vx[T - 1] = cx[T - 1]
    for t in range(T - 1, 0, -1):
        Qx[t - 1] = _matTvec(A[t - 1], Vx[t]) + cx[t - 1]
        Qu[t - 1] = _matTvec(B[t - 1], Vx[t]) + cu[t - 1]
        k[t - 1] = Qu[t - 1] * -1.0
        Vx[t - 1] = Qx[t - 1]
        d = 0.0
        for i in range(nu):
            d += float(k[t - 1, i]) * float(Qu[t - 1, i])
        dV[0] += d
    k[T - 1] = k[T - 2]
    return dict(k=k, Vx=Vx, Qx=Qx, Qu=Qu, dV=dV)


# ----------------------------------------------------------------------------- policy, spline mappings, planner loop
# utilities.h:122-141, utilities.cc:286-404; gradient/policy.cc; gradient/spline_mapping.cc; gradient/planner.cc:40-415
def find_interval(xs, x):
    import bisect
    n = len(xs)
    ub = bisect.bisect_right(list(xs), x); lb = ub - 1
    if lb < 0:
        return 0, 0
    if lb > n - 1:
        return n - 1, n - 1
    return max(lb, 0), min(ub, n - 1)


def cubic_coefficients(x, xs):
    b0, b1 = find_interval(xs, x)
    if b0 == b1:
        return [1.0, 0.0, 0.0, 0.0]
    dx = xs[b1] - xs[b0]; t = (x - xs[b0]) / dx
    return [2.0 * t * t * t - 3.0 * t * t + 1.0, (t * t * t - 2.0 * t * t + t) * dx, -2.0 * t * t * t + 3 * t * t, (t * t * t - t * t) * dx]


def _slope(x, xs, ys, i):
    n = len(xs); b0, b1 = find_interval(xs, x)
    if b0 == 0 and b1 == 0:
        return (ys[b1 + 1][i] - ys[b1][i]) / (xs[b1 + 1] - xs[b1]) if n > 2 else 0.0
    if b0 == n - 1 and b1 == n - 1:
        return (ys[b0][i] - ys[b0 - 1][i]) / (xs[b0] - xs[b0 - 1]) if n > 2 else 0.0
    if b0 == 0:
        return (ys[b1][i] - ys[b0][i]) / (xs[b1] - xs[b0])
    return 0.5 * (ys[b1][i] - ys[b0][i]) / (xs[b1] - xs[b0]) + 0.5 * (ys[b0][i] - ys[b0 - 1][i]) / (xs[b0] - xs[b0 - 1])


def interpolate(representation, x, xs, ys):
    """Zero / Linear / CubicInterpolation of ys [P, dim] over xs at x, as GradientPolicy::Action picks them (no clamp)"""
    xs = [float(v) for v in xs]; ys = [[float(v) for v in row] for row in np.asarray(ys, float).reshape(len(xs), -1)]
    dim = len(ys[0]); b0, b1 = find_interval(xs, x)
    if b0 == b1 or representation == 0:
        return np.array(ys[b0])
    if representation == 1:
        t = (x - xs[b0]) / (xs[b1] - xs[b0])
        return np.array([ys[b0][i] * (1.0 - t) + ys[b1][i] * t for i in range(dim)])
    c = cubic_coefficients(x, xs)
    return np.array([c[0] * ys[b0][i] + c[1] * _slope(xs[b0], xs, ys, i) + c[2] * ys[b1][i] + c[3] * _slope(xs[b1], xs, ys, i) for i in range(dim)])


def policy_action(representation, ctrlrange, times, parameters, time):
    cr = np.asarray(ctrlrange, float).reshape(-1, 2)
    return np.clip(interpolate(representation, float(time), times, parameters), cr[:, 0], cr[:, 1])


def spline_mapping(representation, dim, input_times, output_times):
    """[(dim T), (dim S)]: knot values -> actions at output_times"""
    xs = [float(v) for v in input_times]; S = len(xs); T = len(output_times)
    M = np.zeros((dim * T, dim * S))
    if representation in (0, 1):
        for i, t in enumerate(output_times):
            b0, b1 = find_interval(xs, float(t))
            for j in range(dim):
                if representation == 0 or b0 == b1:
                    M[dim * i + j, dim * b0 + j] = 1.0
                else:
                    a = (float(t) - xs[b0]) / (xs[b1] - xs[b0])
                    M[dim * i + j, dim * b0 + j] = 1.0 - a; M[dim * i + j, dim * b1 + j] = a
        return M
    SM = np.zeros((2 * dim * S, dim * S))
    for r in range(dim * S):
        SM[r, r] = 1.0
    for i in range(S):
        dt1 = 1.0 / (xs[i] - xs[i - 1]) if i > 0 else 0.0
        dt2 = 1.0 / (xs[i + 1] - xs[i]) if i < S - 1 else 0.0
        if 0 < i < S - 1:
            dt1 *= 0.5; dt2 *= 0.5
        for j in range(dim):
            row = dim * S + dim * i + j
            if i - 1 >= 0:
                SM[row, dim * (i - 1) + j] = -dt1
            SM[row, dim * i + j] = dt1 - dt2
            if i + 1 <= S - 1:
                SM[row, dim * (i + 1) + j] = dt2
    CM = np.zeros((dim * T, 2 * dim * S))
    for i, t in enumerate(output_times):
        b0, b1 = find_interval(xs, float(t)); c = cubic_coefficients(float(t), xs)
        for j in range(dim):
            CM[dim * i + j, dim * b0 + j] = c[0]; CM[dim * i + j, dim * S + dim * b0 + j] = c[1]
            if b0 != b1:
                CM[dim * i + j, dim * b1 + j] = c[2]; CM[dim * i + j, dim * S + dim * b1 + j] = c[3]
    return _matmat(CM, SM)


def log_scale(max_value, min_value, steps):
    step = (math.log(max_value) - math.log(min_value)) / max(steps - 1, 1)
    return [math.exp(math.log(min_value) + i * step) for i in range(steps)]


class GradientPlannerMirror:
    """gradient/planner.cc over a backend.  plan_all(state, time, knot_times, candidates [N, P, nu], representation, H) ->
    dict(returns [N], states / actions / times / residual [N, H, .]); derivatives(x, u, t, residual) -> dict(k [H, nu], dV [2], failure [H])."""

    def __init__(self, model, plan_all, derivatives, spline_points, representation=1, num_trajectory=32, max_rollout=1, min_linesearch_step=1e-8):
        self.nu = int(model["nu"]); self.h = float(model["timestep"]); self.ctrlrange = np.asarray(model["actuator_ctrlrange"], float).reshape(-1, 2)
        self.plan_all, self.derivatives = plan_all, derivatives
        self.P, self.rep, self.N, self.max_rollout, self.min_step = int(spline_points), int(representation), int(num_trajectory), int(max_rollout), min_linesearch_step
        self.times = np.zeros(self.P); self.parameters = np.zeros((self.P, self.nu))
        self.state = None; self.time = 0.0
        self.winner = -1; self.failed = False

    def set_state(self, state, time):
        self.state = np.asarray(state, float).copy(); self.time = float(time)

    def action(self, time):
        return policy_action(self.rep, self.ctrlrange, self.times, self.parameters, time)

    def optimize(self, H):
        N, P = self.N, self.P
        # ResamplePolicy
        shift = max((H - 1) * self.h / (P - 1), 1.0e-5)
        t = self.time; ts = []; ps = []
        for _ in range(P):
            ts.append(t); ps.append(self.action(t)); t += shift
        times = np.array([ts[0] + i * shift for i in range(P)]); params = np.array(ps)
        o = self.plan_all(self.state, self.time, times, params[None], self.rep, H)
        c_prev = c_best = float(o["returns"][0])
        traj = {k: o[k][0] for k in ("states", "actions", "times", "residual")}
        self.failed = False
        for _ in range(self.max_rollout):
            g = self.derivatives(traj["states"], traj["actions"], traj["times"], traj["residual"])
            if np.any(g["failure"]):
                self.failed = True
                return
            M = spline_mapping(self.rep, self.nu, times, traj["times"][:H - 1])
            self.update = _matTvec(M, np.asarray(g["k"], float)[:H - 1].ravel()).reshape(P, self.nu)
            self.steps = log_scale(1.0, self.min_step, N - 1) + [0.0]
            cand = np.array([params + self.update * s for s in self.steps])
            o = self.plan_all(self.state, self.time, times, cand, self.rep, H)
            self.returns = o["returns"].copy()
            self.winner = N - 1
            for j in range(N - 1, -1, -1):
                if o["returns"][j] < c_best:
                    c_best = float(o["returns"][j]); self.winner = j
            params = cand[self.winner]
            traj = {k: o[k][self.winner] for k in ("states", "actions", "times", "residual")}
            self.action_step = self.steps[self.winner]
            self.expected = -self.action_step * float(g["dV"][0]) - 1.0e-16
            self.improvement = c_prev - c_best
            self.surprise = min(max(0.0, self.improvement / self.expected), 2.0)
        if c_best >= c_prev:
            self.winner = N - 1
        self.times, self.parameters = times, params
        self.best = traj
