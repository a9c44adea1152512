"""numpy restatement of mjpc_hip_transition_fd around ANY batched step function (TEST INFRASTRUCTURE ONLY): the perturbed table
(fd_assemble), the control-nudge rule (fd_nudge) and the differences (fd_entry) of mujoco_mpc_amd/csrc/transition_fd.h, plus the
reference's ModelDerivatives index set and interpolation weights (mjpc/planners/model_derivatives.cc:56-72, 108-161).

The table is built with Python floats in the kernel's operation order (every product and sum rounded on its own, IEEE sqrt and
divide, cos / sin of eps / 2 from libm), so that it is bit for bit the kernel's table and the step function sees the same inputs;
the differences on plain coordinates are then bit-equal too, those on quaternion coordinates go through atan2."""
import math

import numpy as np

MINVAL = 1e-15


def dims(model, task):
    nq, nv, na, nu = model["nq"], model["nv"], model["na"], model["nu"]
    return dict(nq=nq, nv=nv, na=na, nu=nu, ds=nq + nv + na, nd=2 * nv + na, nr=task["num_residual"])


def dofmap(model):
    """per dof: (qpos address of its coordinate - of w for a quaternion -, quaternion axis 0..2 or -1)"""
    out = [None] * model["nv"]
    for j in range(model["njnt"]):
        ty, qa, da = int(model["jnt_type"][j]), int(model["jnt_qposadr"][j]), int(model["jnt_dofadr"][j])
        if ty == 0:
            for k in range(3):
                out[da + k] = (qa + k, -1); out[da + 3 + k] = (qa + 3, k)
        elif ty == 1:
            for k in range(3):
                out[da + k] = (qa, k)
        else:
            out[da] = (qa, -1)
    return out


def nudge(limited, u, eps, lo, hi, centered):
    """(forward, backward) of one control"""
    fwd = (not limited) or (u + eps <= hi)
    bwd = (centered or not fwd) and ((not limited) or (u - eps >= lo))
    return bool(fwd), bool(bwd)


def _normalize4(q):
    n2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]
    n = math.sqrt(n2)
    if n < MINVAL:
        return [1.0, 0.0, 0.0, 0.0]
    if abs(n - 1) > MINVAL:
        return [q[0] / n, q[1] / n, q[2] / n, q[3] / n]
    return list(q)


def quat_nudge(q, ax, cs, sn):
    """normalise(normalise(q) * [cs, sn e_ax])"""
    w, x, y, z = _normalize4([float(v) for v in q])
    if ax == 0:
        r = [w * cs - x * sn, w * sn + x * cs, y * cs + z * sn, z * cs - y * sn]
    elif ax == 1:
        r = [w * cs - y * sn, x * cs - z * sn, w * sn + y * cs, z * cs + x * sn]
    else:
        r = [w * cs - z * sn, x * cs + y * sn, y * cs - x * sn, w * sn + z * cs]
    return _normalize4(r)


def subquat(qb, qa):
    """body-frame rotation vector of qa^-1 * qb (mju_subQuat(res, qb, qa))"""
    aw, ax, ay, az = qa[0], -qa[1], -qa[2], -qa[3]
    bw, bx, by, bz = qb
    d = np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                  aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])
    s = math.sqrt(d[1] * d[1] + d[2] * d[2] + d[3] * d[3])
    axis = np.array([1.0, 0.0, 0.0]) if s < MINVAL else d[1:] * (1.0 / s)
    speed = 2 * math.atan2(s, d[0])
    if speed > math.pi:
        speed -= 2 * math.pi
    return axis * speed


class Mirror:
    def __init__(self, model, task):
        self.m = model
        self.d = dims(model, task)
        self.map = dofmap(model)
        self.limited = np.asarray(model["actuator_ctrllimited"]).ravel().astype(bool)
        self.range = np.asarray(model["actuator_ctrlrange"], float).reshape(-1, 2)

    def slots(self, centered):
        nc = self.d["nd"] + self.d["nu"]
        return 1 + 2 * nc if centered else 1 + nc

    def flags(self, u, eps, centered, terminal=False):
        if terminal:
            return [(False, False)] * self.d["nu"]
        return [nudge(self.limited[k], float(u[k]), eps, self.range[k, 0], self.range[k, 1], centered) for k in range(self.d["nu"])]

    def assemble(self, x, u, time, eps, centered, last_is_terminal=False):
        d = self.d; nq, nv, nd, nu, ds = d["nq"], d["nv"], d["nd"], d["nu"], d["ds"]
        x = np.asarray(x, float).reshape(-1, ds); T = x.shape[0]
        u = np.asarray(u, float).reshape(T, nu); time = np.asarray(time, float).reshape(T)
        E = self.slots(centered)
        cs, sn = math.cos(0.5 * eps), math.sin(0.5 * eps)
        S = np.repeat(x, E, axis=0); U = np.repeat(u, E, axis=0); Tm = np.repeat(time, E)
        for t in range(T):
            fl = self.flags(u[t], eps, centered, last_is_terminal and t == T - 1)
            for s in range(1, E):
                g = t * E + s
                if centered:
                    c, sgn = (s - 1) >> 1, (-1.0 if (s - 1) & 1 else 1.0)
                else:
                    c, sgn = s - 1, 1.0
                if c >= nd:
                    k = c - nd; fwd, bwd = fl[k]
                    if centered:
                        if not (fwd if sgn > 0 else bwd):
                            continue
                    else:
                        if fwd:
                            sgn = 1.0
                        elif bwd:
                            sgn = -1.0
                        else:
                            continue
                    U[g, k] = float(u[t, k]) + sgn * eps
                elif c < nv:
                    qa, ax = self.map[c]
                    if ax < 0:
                        S[g, qa] = float(x[t, qa]) + sgn * eps
                    else:
                        S[g, qa:qa + 4] = quat_nudge(x[t, qa:qa + 4], ax, cs, sgn * sn)
                else:
                    S[g, nq + (c - nv)] = float(x[t, nq + (c - nv)]) + sgn * eps
        return S, U, Tm

    def difference(self, u, nxt, res, eps, centered, last_is_terminal=False, fill=np.nan):
        d = self.d; nq, nv, nd, nu, ds, nr = d["nq"], d["nv"], d["nd"], d["nu"], d["ds"], d["nr"]
        E = self.slots(centered)
        nxt = np.asarray(nxt, float).reshape(-1, E, ds); T = nxt.shape[0]
        res = np.asarray(res, float).reshape(T, E, nr); u = np.asarray(u, float).reshape(T, nu)
        M = np.full((T, nd + nr, nd + nu), fill)
        quat_rows = np.array([ax >= 0 for _, ax in self.map] + [False] * (nd - nv + nr))
        for t in range(T):
            term = last_is_terminal and t == T - 1
            fl = self.flags(u[t], eps, centered)
            for c in range(nd + nu):
                den = eps
                if c < nd:
                    if centered:
                        sb, sa, den = 1 + 2 * c, 2 + 2 * c, 2 * eps
                    else:
                        sb, sa = 1 + c, 0
                else:
                    fwd, bwd = fl[c - nd]
                    if not (fwd or bwd):
                        M[t, :, c] = 0.0
                        continue
                    if centered:
                        sb, sa = (1 + 2 * c if fwd else 0), (2 + 2 * c if bwd else 0)
                        if fwd and bwd:
                            den = 2 * eps
                    else:
                        sb, sa = (1 + c, 0) if fwd else (0, 1 + c)
                ya, yb = nxt[t, sa], nxt[t, sb]
                col = np.empty(nd + nr)
                for o in range(nv):
                    qa, ax = self.map[o]
                    col[o] = (yb[qa] - ya[qa]) if ax < 0 else subquat(yb[qa:qa + 4], ya[qa:qa + 4])[ax]
                col[nv:nd] = yb[nq:] - ya[nq:]
                col[nd:] = res[t, sb] - res[t, sa]
                M[t, :, c] = col / den
            if term:
                M[t, :nd, :] = fill; M[t, nd:, nd:] = fill
        return M[:, :nd, :nd].copy(), M[:, :nd, nd:].copy(), M[:, nd:, :nd].copy(), M[:, nd:, nd:].copy(), quat_rows[:nd]

    def fd(self, step, x, u, time, eps, centered, last_is_terminal=False, fill=np.nan):
        """step(states, ctrl, time) -> (next_states, residual, failure); returns A, B, C, D, failure[T], quaternion-row mask [nd]"""
        S, U, Tm = self.assemble(x, u, time, eps, centered, last_is_terminal)
        nxt, res, fail = step(S, U, Tm)
        A, B, C, D, qrows = self.difference(u, nxt, res, eps, centered, last_is_terminal, fill)
        E = self.slots(centered)
        return A, B, C, D, np.bitwise_or.reduce(np.asarray(fail).reshape(-1, E), axis=1), qrows


# ---------------------------------------------------------------------------- ModelDerivatives::Compute's index set and weights
def evaluate_indices(T, skip):
    """model_derivatives.cc:56-72: 0, then s, 2s, ... below T - s (s = skip + 1), then T - 2 and T - 1; an index listed twice is kept once"""
    s = skip + 1
    return sorted(set([0] + list(range(s, T - s, s)) + [T - 2, T - 1]))


def interpolate_plan(T, skip):
    """model_derivatives.cc:108-161: [(t, lower, upper, tt)] for every index that is not evaluated; tt = (t - lower) / (upper - lower)"""
    ev = evaluate_indices(T, skip)
    out = []
    for t in range(T):
        if t in ev:
            continue
        lo = max(e for e in ev if e < t); up = min(e for e in ev if e > t)
        out.append((t, lo, up, float(t - lo) / float(up - lo)))
    return ev, out


def interpolate(L, U, tt):
    """the reference's two steps: mju_scl(out, L, 1 - tt); mju_addToScl(out, U, tt)"""
    out = np.asarray(L, float) * (1.0 - tt)
    return out + np.asarray(U, float) * tt
