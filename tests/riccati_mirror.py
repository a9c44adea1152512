"""numpy / plain-Python mirror of the iLQG backward pass (mujoco_mpc_amd/csrc/riccati.h; TEST INFRASTRUCTURE ONLY), by the summation rule of
gradient_planner_mirror.py: every contraction starts at 0.0 and runs over the ascending contraction index, a rounded product and a rounded add
per step (numpy does not fuse), `/` and sqrt correctly rounded.  Written from the formulas of include/mjpc_hip.h, not from the C++."""
import math

import numpy as np

import gradient_planner_mirror as gm


def _matTmat(A, B):          # A' B
    S = np.zeros((A.shape[1], B.shape[1]))
    for k in range(A.shape[0]):
        S = S + A[k][:, None] * B[k][None, :]
    return S


def _matmat(A, B):           # A B
    S = np.zeros((A.shape[0], B.shape[1]))
    for k in range(A.shape[1]):
        S = S + A[:, k:k + 1] * B[k:k + 1, :]
    return S


def _matvec(A, v):
    s = np.zeros(A.shape[0])
    for k in range(A.shape[1]):
        s = s + A[:, k] * v[k]
    return s


def _dot(a, b):
    s = 0.0
    for x, y in zip(a, b):
        s = s + float(x) * float(y)
    return s


def chol(H, index):
    """lower factor of H[index][:, index] as a list of rows, or None when a pivot is not > 0"""
    nf = len(index)
    R = [[0.0] * nf for _ in range(nf)]
    for j in range(nf):
        s = 0.0
        for k in range(j):
            s = s + R[j][k] * R[j][k]
        d = float(H[index[j], index[j]]) + -s
        if not d > 0:
            return None
        l = math.sqrt(d)
        R[j][j] = l
        for i in range(j + 1, nf):
            q = 0.0
            for k in range(j):
                q = q + R[i][k] * R[j][k]
            R[i][j] = (float(H[index[i], index[j]]) + -q) / l
    return R


def cholsolve(R, b):
    nf = len(R)
    x = [0.0] * nf
    for i in range(nf):
        s = 0.0
        for k in range(i):
            s = s + R[i][k] * x[k]
        x[i] = (float(b[i]) + -s) / R[i][i]
    for i in range(nf - 1, -1, -1):
        s = 0.0
        for k in range(i + 1, nf):
            s = s + R[k][i] * x[k]
        x[i] = (x[i] + -s) / R[i][i]
    return x


def _clamp(v, lo, hi):
    v = v if v < hi else hi
    return v if v > lo else lo


def _value(H, g, x):
    n = len(x)
    q = 0.0; l = 0.0
    for i in range(n):
        s = 0.0
        for j in range(n):
            s = s + float(H[i, j]) * x[j]
        q = q + x[i] * s
        l = l + x[i] * float(g[i])
    return 0.5 * q + l


def boxqp(H, g, lower, upper, warm=None):
    """-> (nfree or -1, x, index, R)"""
    n = len(g)
    lo = [float(v) for v in lower]; hi = [float(v) for v in upper]
    x = [_clamp(float(v), lo[i], hi[i]) for i, v in enumerate(np.zeros(n) if warm is None else warm)]
    value = _value(H, g, x)
    mask = [-1] * n
    index, R = [], None
    for _ in range(100):
        grad = [0.0] * n
        changed = False
        index = []
        for i in range(n):
            s = 0.0
            for j in range(n):
                s = s + float(H[i, j]) * x[j]
            grad[i] = float(g[i]) + s
            c = int((x[i] == lo[i] and grad[i] > 0) or (x[i] == hi[i] and grad[i] < 0))
            if mask[i] != c:
                changed = True
            mask[i] = c
            if not c:
                index.append(i)
        nf = len(index)
        if nf == 0:
            break
        if changed:
            R = chol(H, index)
            if R is None:
                return -1, x, index, None
        gn = 0.0
        for i in index:
            gn = gn + grad[i] * grad[i]
        if gn < 1.0e-16:
            break
        y = cholsolve(R, [grad[i] for i in index])
        search = [0.0] * n
        sdotg = 0.0
        for a, i in enumerate(index):
            search[i] = -y[a]
            sdotg = sdotg + -y[a] * grad[i]
        if not sdotg < 0:
            break
        step = 1.0
        accepted = False
        while step >= 1.0e-22:
            cand = [_clamp(x[i] + step * search[i], lo[i], hi[i]) for i in range(n)]
            nv = _value(H, g, cand)
            if nv + -value <= 0.1 * (step * sdotg):
                accepted = True
                break
            step = step * 0.5
        if not accepted:
            break
        x = cand; value = nv
    return len(index), x, index, R


def scale_regularization(reg, rate, factor, reg_min, reg_max):
    s = rate * factor
    rate = (s if s > factor else factor) if factor > 1 else (s if s < factor else factor)
    v = reg * rate
    v = v if v > reg_min else reg_min
    return (v if v < reg_max else reg_max), rate


class _State:
    pass


def _step(c, o, t, mu, reg_type, limits_on, st):
    A, B = c["A"][t], c["B"][t]
    n, m = B.shape
    W, wx = o["Vxx"][t + 1], o["Vx"][t + 1]
    tmp = _matTmat(A, W); tmp2 = _matTmat(B, W)
    Qx = _matvec(A.T, wx) + c["cx"][t]; Qu = _matvec(B.T, wx) + c["cu"][t]
    Qxx = _matmat(tmp, A) + c["cxx"][t]; Qxu = _matmat(tmp, B) + c["cxu"][t]; Quu = _matmat(tmp2, B) + c["cuu"][t]
    o["Qx"][t], o["Qu"][t], o["Qxx"][t], o["Qxu"][t], o["Quu"][t] = Qx, Qu, Qxx, Qxu, Quu
    if reg_type == 2:
        Wr = W.copy()
        for i in range(n):
            Wr[i, i] = Wr[i, i] + mu
        Hq = _matmat(_matTmat(B, Wr), B) + c["cuu"][t]
    else:
        Hq = Quu.copy()
        if mu:
            if reg_type == 0:
                for i in range(m):
                    Hq[i, i] = Hq[i, i] + mu
            elif reg_type == 1:
                Hq = Hq + _matTmat(B, B) * mu
    o["K"][t] = 0.0
    if limits_on == 1:
        lo = c["action_limits"][:, 0] - c["actions"][t]; hi = c["action_limits"][:, 1] - c["actions"][t]
        nf, x, index, R = boxqp(Hq, Qu, lo, hi, st.res)
        if nf < 0:
            return False
        st.res = list(x)
        k = np.array(x)
    else:
        index = list(range(m))
        R = chol(Hq, index)
        if R is None:
            return False
        k = -np.array(cholsolve(R, Qu))
    K = np.zeros((m, n))
    if index:
        for j in range(n):
            y = cholsolve(R, [Qxu[j, i] for i in index])
            for a, i in enumerate(index):
                K[i, j] = -y[a]
    o["k"][t] = k; o["K"][t] = K
    o["dV"][0] = o["dV"][0] + _dot(k, Qu)
    t1 = _matvec(Quu, k)
    o["dV"][1] = o["dV"][1] + 0.5 * _dot(k, t1)
    t2 = t1 + Qu
    o["Vx"][t] = (Qx + _matvec(K.T, t2)) + _matvec(Qxu, k)
    T3 = _matTmat(K, _matmat(Quu, K)); T2 = _matmat(Qxu, K)
    P = (Qxx + T3) + (T2 + T2.T)
    o["Vxx"][t] = 0.5 * (P + P.T)
    return True


def backward_pass(c, regularization=1.0, regularization_rate=1.0, regularization_type=0, action_limits_on=1, max_regularization_iterations=5,
                  min_regularization=1.0e-6, max_regularization=1.0e6, regularization_factor=2.0):
    """c: the dict of riccati_cases.trajectory -> the dict of HipBackend.ilqg_backward_pass (outputs start as zeros)"""
    T, n = c["cx"].shape; m = c["cu"].shape[1]
    o = dict(k=np.zeros((T, m)), K=np.zeros((T, m, n)), Vx=np.zeros((T, n)), Vxx=np.zeros((T, n, n)), Qx=np.zeros((T - 1, n)), Qu=np.zeros((T - 1, m)),
             Qxx=np.zeros((T - 1, n, n)), Qxu=np.zeros((T - 1, n, m)), Quu=np.zeros((T - 1, m, m)), dV=np.zeros(2))
    st = _State(); st.res = [0.0] * m
    reg, rate = float(regularization), float(regularization_rate)
    it, done, failed = 0, 0, -1
    o["Vx"][T - 1] = c["cx"][T - 1]; o["Vxx"][T - 1] = c["cxx"][T - 1]
    while it < max_regularization_iterations and not done:
        o["dV"][:] = 0.0
        failed = -1
        for t in range(T - 2, -1, -1):
            if not _step(c, o, t, reg, regularization_type, action_limits_on, st):
                failed = t
                break
        if failed < 0:
            done = 1
            o["k"][T - 1] = o["k"][T - 2]; o["K"][T - 1] = o["K"][T - 2]
        elif reg <= max_regularization:
            reg, rate = scale_regularization(reg, rate, regularization_factor, min_regularization, max_regularization)
            it += 1
        else:
            break
    o["status"] = np.array([done, -1 if done else failed, it], np.int32); o["regularization"] = reg; o["regularization_rate"] = rate
    return o


# ----------------------------------------------------------------------------- iLQGPolicy::Action
def _quat_diff(qa, qb):
    d = [qa[0] * qb[0] + qa[1] * qb[1] + qa[2] * qb[2] + qa[3] * qb[3],
         qa[0] * qb[1] - qa[1] * qb[0] - qa[2] * qb[3] + qa[3] * qb[2],
         qa[0] * qb[2] + qa[1] * qb[3] - qa[2] * qb[0] - qa[3] * qb[1],
         qa[0] * qb[3] - qa[1] * qb[2] + qa[2] * qb[1] - qa[3] * qb[0]]
    sn = math.sqrt(d[1] * d[1] + d[2] * d[2] + d[3] * d[3])
    axis = [1.0, 0.0, 0.0] if sn < 1e-15 else [d[1] / sn, d[2] / sn, d[3] / sn]
    speed = 2 * math.atan2(sn, d[0])
    if speed > math.pi:
        speed -= 2 * math.pi
    return [a * speed for a in axis]


def state_diff(model, s1, s2):
    nq, nv, na = int(model["nq"]), int(model["nv"]), int(model["na"])
    ds = np.zeros(2 * nv + na)
    for ty, qa, da in zip(np.ravel(model["jnt_type"]), np.ravel(model["jnt_qposadr"]), np.ravel(model["jnt_dofadr"])):
        if ty == 0:
            ds[da:da + 3] = s2[qa:qa + 3] - s1[qa:qa + 3]
            ds[da + 3:da + 6] = _quat_diff(s1[qa + 3:qa + 7], s2[qa + 3:qa + 7])
        elif ty == 1:
            ds[da:da + 3] = _quat_diff(s1[qa:qa + 4], s2[qa:qa + 4])
        else:
            ds[da] = s2[qa] - s1[qa]
    ds[nv:] = s2[nq:] - s1[nq:]
    return ds


def policy_action(model, times, states, actions, feedback_gain, time, state=None, representation=1, feedback_scaling=1.0):
    H = len(times)
    nq, nv, na, nu = (int(model[k]) for k in ("nq", "nv", "na", "nu"))
    times = [float(v) for v in times]
    b0, b1 = gm.find_interval(times, time)
    rep = 0 if b0 == b1 else representation
    a = gm.interpolate(rep, float(time), times[:H - 1], np.asarray(actions, float)[:H - 1])
    if state is not None:
        x = gm.interpolate(rep, float(time), times, np.asarray(states, float))
        if rep != 0:
            for ty, qa in zip(np.ravel(model["jnt_type"]), np.ravel(model["jnt_qposadr"])):
                if ty <= 1:
                    q = x[qa + (3 if ty == 0 else 0):][:4]
                    q /= math.sqrt(float(q @ q))
        K = gm.interpolate(rep, float(time), times[:H - 1], np.asarray(feedback_gain, float).reshape(H, -1)[:H - 1]).reshape(nu, 2 * nv + na)
        a = a + (K @ state_diff(model, x, np.asarray(state, float))) * feedback_scaling
    cr = np.asarray(model["actuator_ctrlrange"], float).reshape(-1, 2)
    return np.clip(a, cr[:, 0], cr[:, 1])
