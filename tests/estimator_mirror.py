"""numpy restatement of the estimators around ANY batched step function (TEST INFRASTRUCTURE ONLY), written from the reference's
mjpc/estimators/kalman.cc and unscented.cc: the sigma-point table, the weighted moments (mujoco_mpc_amd/csrc/estimator.h), the filter
algebra (the Estimators section of csrc/planner.cc) and the two filters.

Where bits are compared, sums run as explicit sequential loops over the contraction index (vectorised over the OUTPUT entries only:
numpy's elementwise products and sums are rounded separately), in the order of the code under test; `@` is not used there.  The
quaternion mean is numpy.linalg.eigh's principal eigenvector with the sign rule of estimator.h (dot product with the nominal row's
next quaternion >= 0); it is independent of the kernel's QUEST iteration.  The quaternion integration exists twice: in the kernel's own
bit-exact spelling (the table every comparison behind the step needs) and in MuJoCo's with numpy's functions (what that spelling is
checked against)."""
import math

import numpy as np

import transition_mirror as tm

MINVAL = 1e-15
OK, COVARIANCE_RANK, SENSOR_RANK, STEP_FLAGGED = 0, 1, 2, 3


def weights(nd, alpha=1.0, beta=2.0):
    """unscented.cc:134-143"""
    lam = nd * (alpha * alpha - 1.0)
    mean0 = lam / (nd + lam)
    return dict(sigma_step=math.sqrt(nd + lam), mean0=mean0, cov0=mean0 + 1.0 - alpha * alpha + beta, sigma=1.0 / (2.0 * (nd + lam)))


# ---------------------------------------------------------------------------- quaternions
# ukf_sincos / ukf_quatintegrate of csrc/estimator.h with Python floats, operation for operation (every product and sum rounded on its own,
# IEEE sqrt and divide): bit for bit the kernel's sigma points, so that the step function sees the same inputs
_S = [-2.50507602534068634195e-08, 2.75573137070700676789e-06, -1.98412698298579493134e-04, 8.33333333332248946124e-03, -1.66666666666666324348e-01]
_C = [2.08757232129817482790e-09, -2.75573143513906633035e-07, 2.48015872894767294178e-05, -1.38888888888741095749e-03, 4.16666666666666019037e-02]


def sincos_rn(x):
    if not abs(x) < 64.0:
        return math.sin(x), math.cos(x)
    k = float(np.rint(x * 0.63661977236758134308))
    r = (x + -(k * 1.57079632673412561417e+00)) + -(k * 6.07710050650619224932e-11)
    z = r * r
    ps, pc = 1.58969099521155010221e-10, -1.13596475577881948265e-11
    for i in range(5):
        ps = _S[i] + z * ps; pc = _C[i] + z * pc
    s = r + (r * z) * ps
    c = (1.0 + -(0.5 * z)) + (z * z) * pc
    q = int(k) & 3
    s1, c1 = (c, s) if q & 1 else (s, c)
    return (-s1 if q & 2 else s1), (-c1 if (q + 1) & 2 else c1)


def _normalize4(q):
    n2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]
    n = math.sqrt(n2)
    if n < MINVAL:
        return [1.0, 0.0, 0.0, 0.0]
    if abs(n - 1) > MINVAL:
        return [q[0] / n, q[1] / n, q[2] / n, q[3] / n]
    return list(q)


def quat_integrate(q, vel, scale):
    """ukf_quatintegrate: normalise(normalise(q) * exp(scale * vel))"""
    ax = [float(v) for v in vel]
    n = math.sqrt((ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2])
    ax = [1.0, 0.0, 0.0] if n < MINVAL else [ax[0] / n, ax[1] / n, ax[2] / n]
    angle = scale * n
    b = [1.0, 0.0, 0.0, 0.0]
    if angle != 0:
        sn, cs = sincos_rn(angle * 0.5)
        b = [cs, ax[0] * sn, ax[1] * sn, ax[2] * sn]
    a = _normalize4([float(v) for v in q])
    return _normalize4([((a[0] * b[0] + -(a[1] * b[1])) + -(a[2] * b[2])) + -(a[3] * b[3]),
                        ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) + -(a[3] * b[2]),
                        ((a[0] * b[2] + -(a[1] * b[3])) + a[2] * b[0]) + a[3] * b[1],
                        ((a[0] * b[3] + a[1] * b[2]) + -(a[2] * b[1])) + a[3] * b[0]])


def quat_integrate_mujoco(q, vel, scale):
    """mju_quatIntegrate in MuJoCo's spelling and numpy's functions: the independent statement the kernel's spelling is checked against"""
    v = np.array(vel, float)
    n = np.sqrt(np.sum(v * v))
    axis = np.array([1.0, 0.0, 0.0]) if n < MINVAL else v / n
    angle = scale * n
    r = np.concatenate([[np.cos(0.5 * angle)], axis * np.sin(0.5 * angle)])
    a = np.array(q, float)
    a = a / np.sqrt(np.sum(a * a))
    return np.array([a[0] * r[0] - a[1] * r[1] - a[2] * r[2] - a[3] * r[3], a[0] * r[1] + a[1] * r[0] + a[2] * r[3] - a[3] * r[2],
                     a[0] * r[2] - a[1] * r[3] + a[2] * r[0] + a[3] * r[1], a[0] * r[3] + a[1] * r[2] - a[2] * r[1] + a[3] * r[0]])


def quat_mean_eigh(Q, w, nominal):
    """principal eigenvector of sum_j 4 w_j q_j q_j' - (sum w) I, signed towards `nominal`"""
    Q = np.asarray(Q, float); w = np.asarray(w, float)
    K = 4.0 * np.einsum("j,ja,jb->ab", w, Q, Q) - w.sum() * np.eye(4)
    val, vec = np.linalg.eigh(K)
    v = vec[:, -1]
    return -v if float(v @ np.asarray(nominal, float)) < 0 else v


# ---------------------------------------------------------------------------- the algebra, sequential over the contraction index
def mm(A, B):
    A = np.asarray(A, float); B = np.asarray(B, float)
    s = np.zeros((A.shape[0], B.shape[1]))
    for k in range(A.shape[1]):
        s = s + A[:, k:k + 1] * B[k:k + 1, :]
    return s


def chol(H):
    """CholFactorSub with the identity index: lower factor, or None when a pivot is not > 0"""
    H = np.asarray(H, float); n = H.shape[0]
    R = np.zeros((n, n))
    for j in range(n):
        s = 0.0
        for k in range(j):
            s = s + R[j, k] * R[j, k]
        d = H[j, j] + -s
        if not d > 0:
            return None
        l = math.sqrt(d)
        R[j, j] = l
        if j + 1 < n:
            q = np.zeros(n - j - 1)
            for k in range(j):
                q = q + R[j + 1:, k] * R[j, k]
            R[j + 1:, j] = (H[j + 1:, j] + -q) / l
    return R


def chol_solve(R, B):
    """CholSolveSub for every ROW of B (vectorised over the rows)"""
    B = np.atleast_2d(np.asarray(B, float)); n = R.shape[0]
    X = np.zeros_like(B)
    for i in range(n):
        s = np.zeros(B.shape[0])
        for k in range(i):
            s = s + R[i, k] * X[:, k]
        X[:, i] = (B[:, i] + -s) / R[i, i]
    for i in range(n - 1, -1, -1):
        s = np.zeros(B.shape[0])
        for k in range(i + 1, n):
            s = s + R[k, i] * X[:, k]
        X[:, i] = (X[:, i] + -s) / R[i, i]
    return X


def symmetrize(P):
    return 0.5 * (P + P.T)


def kalman_gain(P, C, R):
    """(status, PCt, factor, gain)"""
    PCt = mm(P, np.asarray(C, float).T)
    S = mm(C, PCt)
    S[np.diag_indices_from(S)] += np.asarray(R, float)
    F = chol(S)
    if F is None:
        return SENSOR_RANK, None, None, None
    return OK, PCt, F, chol_solve(F, PCt)


def kalman_correct(PCt, F, gain, err, P):
    y = chol_solve(F, err)[0]
    return mm(PCt, y[:, None])[:, 0], symmetrize(P - mm(PCt, gain.T))


def covariance_predict(A, Q, P):
    N = mm(A, mm(P, np.asarray(A, float).T))
    N[np.diag_indices_from(N)] += np.asarray(Q, float)
    return symmetrize(N)


def unscented_correct(css, csy, cyy, err):
    """(status, correction, P)"""
    F = chol(cyy)
    if F is None:
        return SENSOR_RANK, None, None
    y = chol_solve(F, err)[0]
    G = chol_solve(F, csy)
    return OK, mm(csy, y[:, None])[:, 0], symmetrize(css - mm(csy, G.T))


def textbook_kalman(A, B, Cm, Q, R, x, P, u, y):
    """one measurement update then one prediction of the linear Kalman filter, in plain numpy"""
    S = Cm @ P @ Cm.T + R
    K = P @ Cm.T @ np.linalg.inv(S)
    x = x + K @ (y - Cm @ x)
    P = P - K @ S @ K.T
    P = 0.5 * (P + P.T)
    x = A @ x + B @ u
    P = A @ P @ A.T + Q
    return x, 0.5 * (P + P.T)


# ---------------------------------------------------------------------------- the model-dependent part
class Mirror:
    def __init__(self, model, task, first=0, ns=None):
        self.m = model
        self.d = tm.dims(model, task)
        self.map = tm.dofmap(model)
        self.first = int(first); self.ns = self.d["nr"] - self.first if ns is None else int(ns)
        self.fd = tm.Mirror(model, task)
        self.quats = sorted({qa for qa, ax in self.map if ax >= 0})
        self.quat_cols = np.array([ax >= 0 for _, ax in self.map] + [False] * (self.d["nd"] - self.d["nv"]))       # tangent coordinates of quaternions
        qm = np.zeros(self.d["ds"], bool)
        for qa in self.quats:
            qm[qa:qa + 4] = True
        self.quat_state = qm                                                                                          # state coordinates of quaternions

    def integrate(self, x, c, scale=1.0, quat=None):
        """x (+) scale c: mj_integratePos of c[0:nv] over `scale`, a plain add on qvel and act"""
        quat = quat or quat_integrate
        d = self.d; nq, nv = d["nq"], d["nv"]
        x = np.array(x, float); c = np.asarray(c, float)
        done = set()
        for dof, (qa, ax) in enumerate(self.map):
            if ax < 0:
                x[qa] = x[qa] + scale * c[dof]
            elif qa not in done:
                done.add(qa)
                x[qa:qa + 4] = quat(x[qa:qa + 4], c[dof:dof + 3], scale)
        x[nq:] = x[nq:] + scale * c[nv:]
        return x

    def sigma_table(self, x, L, sigma_step, u, time, quat=None):
        d = self.d; nd = d["nd"]; R = 2 * nd + 1
        L = np.tril(np.asarray(L, float).reshape(nd, nd))
        S = np.tile(np.asarray(x, float), (R, 1))
        for i in range(nd):
            c = sigma_step * L[:, i]
            S[i] = self.integrate(x, c, 1.0, quat); S[nd + i] = self.integrate(x, c, -1.0, quat)
        return S, np.tile(np.asarray(u, float).reshape(1, -1), (R, 1)), np.full(R, float(time))

    def moments_of(self, nxt, res, fail, w, noise_process, noise_sensor):
        """the weighted moments of stepped rows (ukf_mean_kernel, ukf_cov_kernel)"""
        d = self.d; nq, nv, nd, ds = d["nq"], d["nv"], d["nd"], d["ds"]; R = 2 * nd + 1
        Y = np.asarray(res, float)[:, self.first:self.first + self.ns]
        wm = np.full(R, w["sigma"]); wm[-1] = w["mean0"]
        wc = np.full(R, w["sigma"]); wc[-1] = w["cov0"]
        sm = np.zeros(ds); ym = np.zeros(self.ns)
        for j in range(R):
            sm = sm + nxt[j] * wm[j]; ym = ym + Y[j] * wm[j]
        for qa in self.quats:
            sm[qa:qa + 4] = quat_mean_eigh(nxt[:, qa:qa + 4], wc, nxt[-1, qa:qa + 4])
        D = np.zeros((R, nd + self.ns))
        for j in range(R):
            for dof, (qa, ax) in enumerate(self.map):
                D[j, dof] = (nxt[j, qa] - sm[qa]) if ax < 0 else tm.subquat(nxt[j, qa:qa + 4], sm[qa:qa + 4])[ax]
            D[j, nv:nd] = nxt[j, nq:] - sm[nq:]
            D[j, nd:] = Y[j] - ym
        cov = np.diag(np.concatenate([np.asarray(noise_process, float), np.asarray(noise_sensor, float)]))
        for j in range(R):
            cov = cov + (D[j][:, None] * D[j][None, :]) * wc[j]
        return dict(state_mean=sm, sensor_mean=ym, cov_ss=cov[:nd, :nd].copy(), cov_sy=cov[:nd, nd:].copy(), cov_yy=cov[nd:, nd:].copy(),
                    sigma_next=np.array(nxt), diff=D, failure=int(np.bitwise_or.reduce(np.asarray(fail, np.int32))))

    def moments(self, step, x, L, w, u, time, noise_process, noise_sensor):
        S, U, T = self.sigma_table(x, L, w["sigma_step"], u, time)
        nxt, res, fail = step(S, U, T)
        o = self.moments_of(nxt, res, fail, w, noise_process, noise_sensor)
        o["sigma"] = S
        return o


class _Filter:
    def __init__(self, model, task, step, first=0, ns=None, scale=1e-4, eps=1e-6, centered=False, alpha=1.0, beta=2.0):
        self.mir = Mirror(model, task, first, ns)
        self.step = step
        self.scale, self.eps, self.centered = scale, eps, centered
        self.w = weights(self.mir.d["nd"], alpha, beta)
        self.h = float(model["timestep"])

    def Reset(self, state, time=0.0):
        nd = self.mir.d["nd"]
        self.state = np.array(state, float); self.time = float(time)
        self.covariance = self.scale * np.eye(nd)
        self.noise_process = np.full(nd, self.scale); self.noise_sensor = np.full(self.mir.ns, self.scale)


class Kalman(_Filter):
    linearize = None        # (x, u, time, eps, centered) -> (A, C, next, residual, failure): to put another implementation of the device half in

    def _lin(self):
        if self.linearize is not None:
            return self.linearize(self.state, self.u, self.time, self.eps, self.centered)
        A, B, C, D, fail, _ = self.mir.fd.fd(self.step, self.state[None], self.u[None], np.array([self.time]), self.eps, self.centered)
        nxt, res, fl = self.step(self.state[None], self.u[None], np.array([self.time]))
        return A[0], C[0], nxt[0], res[0], int(fail[0])

    def UpdateMeasurement(self, ctrl, sensor):
        mir = self.mir
        self.u = np.array(ctrl, float).reshape(-1)
        A, C, nxt, res, fail = self._lin()
        if fail:
            return STEP_FLAGGED
        Cs = C[mir.first:mir.first + mir.ns]
        rc, PCt, F, G = kalman_gain(self.covariance, Cs, self.noise_sensor)
        if rc:
            return rc
        err = np.asarray(sensor, float) - res[mir.first:mir.first + mir.ns]
        corr, self.covariance = kalman_correct(PCt, F, G, err, self.covariance)
        self.state = mir.integrate(self.state, corr)
        return OK

    def UpdatePrediction(self):
        A, C, nxt, res, fail = self._lin()
        if fail:
            return STEP_FLAGGED
        self.state = nxt.copy()
        self.covariance = covariance_predict(A, self.noise_process, self.covariance)
        self.time += self.h
        return OK

    def Update(self, ctrl, sensor):
        keep = (self.state.copy(), self.covariance.copy())
        rc = self.UpdateMeasurement(ctrl, sensor)
        if rc:
            return rc
        rc = self.UpdatePrediction()
        if rc:
            self.state, self.covariance = keep
        return rc


class Unscented(_Filter):
    def Update(self, ctrl, sensor, moments=None):
        """moments: (mirror, x, L, w, u, time, noise_process, noise_sensor) -> dict, to put another implementation of the device half in"""
        mir = self.mir
        L = chol(self.covariance)
        if L is None:
            return COVARIANCE_RANK
        u = np.array(ctrl, float).reshape(-1)
        if moments is None:
            o = mir.moments(self.step, self.state, L, self.w, u, self.time, self.noise_process, self.noise_sensor)
        else:
            o = moments(mir, self.state, L, self.w, u, self.time, self.noise_process, self.noise_sensor)
        self.last = o
        if o["failure"]:
            return STEP_FLAGGED
        rc, corr, P = unscented_correct(o["cov_ss"], o["cov_sy"], o["cov_yy"], np.asarray(sensor, float) - o["sensor_mean"])
        if rc:
            return rc
        self.state = mir.integrate(o["state_mean"], corr)
        self.covariance = P
        self.time += self.h
        return OK
