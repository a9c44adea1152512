"""Independent numpy reference for the direct optimiser's window cost (TEST INFRASTRUCTURE ONLY).  Nothing here comes from the kernel, its
emulation or the host mirror.

Two references:

  Window     a synthetic smooth window model on hinge dofs: sensors s(q, v, a) and an inverse-dynamics force f(q, v, a) in closed form, with
             v_t = (q_t - q_{t-1}) / h, a_t = (v_{t+1} - v_t) / h and the window's ends as the reference optimiser evaluates them (t = 0 at
             zero velocity and acceleration, t = T - 1 at zero acceleration).  residuals(Q) is the whole window's residual vector, cost(Q)
             the weighted sum of its norms, and jacobian(Q) the dense Jacobian of the residuals by centred differences over every
             coordinate of every configuration: it differentiates the whole window and has no chain rule in it.  g = J' W n', H = J' W n'' J
             are dense [ntotal][ntotal].  What the code under test gets are the model's closed-form blocks per configuration.
  assemble   the algebra on arbitrary blocks (dense velocity blocks, as quaternion dofs give them) with numpy's matrix products: dense J
             from the chain rule, dense g and H, the band cut out of H.

Norm types as in the cost table: 0 quadratic, 2 L2 (dense Hessian), 6 smooth abs (diagonal, not quadratic)."""
import numpy as np

POS, VEL, ACC = 0, 1, 2


# ------------------------------------------------------------------------------------------------------------------------ norms
def norm(x, typ, p):
    """value, gradient [n], Hessian [n, n]"""
    x = np.asarray(x, float); n = x.size
    if typ == 0:
        return 0.5 * x @ x, x.copy(), np.eye(n)
    if typ == 2:
        s = np.sqrt(x @ x + p * p)
        g = x / s
        return s - p, g, (np.eye(n) - np.outer(g, g)) / s
    if typ == 6:
        s = np.sqrt(x * x + p * p)
        return (s - p).sum(), x / s, np.diag(p * p / s ** 3)
    raise ValueError(typ)


class Spec:
    """the sensors (runs of rows of an nr-row residual starting at first_row), noises and settings, in plain Python"""

    def __init__(self, nv, nr, h, dim, stage, norm_type, prm, noise_sensor, noise_process, first_row=0, mask=None, sensor_flag=True, force_flag=True,
                 time_scaling_sensor=True, time_scaling_force=True, first_step_position_sensors=True, last_step_position_sensors=False,
                 last_step_velocity_sensors=False):
        self.nv, self.nr, self.h = nv, nr, float(h)
        self.dim, self.stage, self.norm_type = list(dim), list(stage), list(norm_type)
        self.prm = np.asarray(prm, float).reshape(len(self.dim), 2)
        self.noise_sensor, self.noise_process = np.asarray(noise_sensor, float), np.asarray(noise_process, float)
        self.first_row, self.mask = first_row, None if mask is None else np.asarray(mask, int)
        self.ns = int(sum(self.dim))
        self.first = np.concatenate([[0], np.cumsum(self.dim)[:-1]]).astype(int) if self.dim else np.zeros(0, int)
        self.flags = dict(sensor_flag=sensor_flag, force_flag=force_flag, time_scaling_sensor=time_scaling_sensor, time_scaling_force=time_scaling_force,
                          first_step_position_sensors=first_step_position_sensors, last_step_position_sensors=last_step_position_sensors,
                          last_step_velocity_sensors=last_step_velocity_sensors)

    def row_stage(self):
        return np.repeat(self.stage, self.dim).astype(int)

    def on(self, t, i):
        return self.mask is None or bool(self.mask[t, i])

    def weight(self, T, t, i):
        f, h = self.flags, self.h
        tw = {POS: 1.0, VEL: h ** 2, ACC: h ** 4}[self.stage[i]] if f["time_scaling_sensor"] else 1.0
        w = tw / self.noise_sensor[i] / self.dim[i] / T
        if t == 0:
            w *= float(f["first_step_position_sensors"])
        if t == T - 1:
            w *= float(f["last_step_position_sensors"] or f["last_step_velocity_sensors"])
        return w

    def force_weight(self, T):
        return (self.h ** 4 if self.flags["time_scaling_force"] else 1.0) / self.noise_process / self.nv / (T - 2)

    def residual_kept(self, T, t, i):
        st, f = self.stage[i], self.flags
        if t == 0:
            return st == POS
        if t == T - 1:
            return (st == POS and f["last_step_position_sensors"]) or (st == VEL and f["last_step_velocity_sensors"])
        return True

    def jacobian_kept(self, T, t):
        """[ns] which sensor rows keep their Jacobian at configuration t (at the last one a position or velocity row keeps it even where its
        residual is zeroed: the reference optimiser's rule)"""
        st = self.row_stage()
        return st == POS if t == 0 else (st < ACC if t == T - 1 else np.ones(self.ns, bool))


def totals(spec, T, rs, rf, J_s, J_f):
    """cost [3], dense gradient [ntotal], dense Hessian [ntotal, ntotal] from the residuals behind the zeroing rules rs [T, ns], rf [T, nv] (ends
    zero) and the dense Jacobians J_s [T, ns, ntotal], J_f [T, nv, ntotal]"""
    nt = J_f.shape[-1]
    cs = cf = 0.0
    g = np.zeros(nt); H = np.zeros((nt, nt))
    f = spec.flags
    if f["sensor_flag"]:
        for t in range(T):
            for i in range(len(spec.dim)):
                if not spec.on(t, i):
                    continue
                sl = slice(spec.first[i], spec.first[i] + spec.dim[i])
                y, ng, nh = norm(rs[t, sl], spec.norm_type[i], spec.prm[i, 0])
                w = spec.weight(T, t, i); Ji = J_s[t, sl]
                cs += w * y; g += w * Ji.T @ ng; H += w * Ji.T @ nh @ Ji
    if f["force_flag"]:
        wf = spec.force_weight(T)
        for t in range(1, T - 1):
            cf += 0.5 * rf[t] @ (wf * rf[t]); g += J_f[t].T @ (wf * rf[t]); H += J_f[t].T @ (wf[:, None] * J_f[t])
    return np.array([cs + cf, cs, cf]), g, H


def band_of(H, nband):
    """MuJoCo's lower band of a dense symmetric matrix: row R holds columns R - nband + 1 .. R, the diagonal last; leading zeros"""
    n = H.shape[0]
    B = np.zeros((n, nband))
    for R in range(n):
        for C in range(nband):
            G = R - (nband - 1 - C)
            if G >= 0:
                B[R, C] = H[R, G]
    return B


def outside_band(H, nband):
    n = H.shape[0]
    i, j = np.indices((n, n))
    return np.abs(H[np.abs(i - j) >= nband]).max(initial=0.0)


def zeroed_residuals(spec, T, rs_raw, rf_raw):
    rs = np.array(rs_raw, float); rf = np.array(rf_raw, float)
    for t in range(T):
        for i in range(len(spec.dim)):
            if not spec.residual_kept(T, t, i):
                rs[t, spec.first[i]:spec.first[i] + spec.dim[i]] = 0.0
    rf[0] = 0.0; rf[T - 1] = 0.0
    return rs, rf


# ------------------------------------------------------------------------------------------------------------------------ the algebra
def assemble(spec, rs_raw, rf_raw, Df, Ds, V0, V1):
    """Df [3][T, nv, nv], Ds [3][T, nr, nv] by (q, v, a), as a finite-difference call returns them (nothing zeroed); V0, V1 [T, nv, nv] (index 0
    unused).  -> dict(cost, gradient, H dense, hessian_band, J_s, J_f dense, residual_sensor, residual_force)"""
    T, nv = Df[0].shape[0], spec.nv
    nt, h = nv * T, spec.h
    rows = slice(spec.first_row, spec.first_row + spec.ns)
    J_s = np.zeros((T, spec.ns, nt)); J_f = np.zeros((T, nv, nt))
    col = lambda t: slice(nv * t, nv * (t + 1))      # noqa: E731
    for t in range(T):
        keep = spec.jacobian_kept(T, t)[:, None]
        Sq, Sv, Sa = (Ds[k][t, rows] * keep for k in range(3))
        if t == 0:
            J_s[t][:, col(0)] = Sq
            continue
        J_s[t][:, col(t - 1)] = Sv @ V0[t]; J_s[t][:, col(t)] = Sq + Sv @ V1[t]
        if t == T - 1:
            continue
        A0, A1, A2 = -V0[t] / h, (V0[t + 1] - V1[t]) / h, V1[t + 1] / h
        J_s[t][:, col(t - 1)] += Sa @ A0; J_s[t][:, col(t)] += Sa @ A1; J_s[t][:, col(t + 1)] = Sa @ A2
        Fq, Fv, Fa = (Df[k][t] for k in range(3))
        J_f[t][:, col(t - 1)] = Fv @ V0[t] + Fa @ A0; J_f[t][:, col(t)] = Fq + Fv @ V1[t] + Fa @ A1; J_f[t][:, col(t + 1)] = Fa @ A2
    rs, rf = zeroed_residuals(spec, T, rs_raw, rf_raw)
    cost, g, H = totals(spec, T, rs, rf, J_s, J_f)
    return dict(cost=cost, gradient=g, H=H, hessian_band=band_of(H, 3 * nv), J_s=J_s, J_f=J_f, residual_sensor=rs, residual_force=rf)


def blocks_of(J, T, nv):
    """the per-configuration blocks [T, rows, 3 nv] of a dense Jacobian [T, rows, ntotal]: column c of block t = global column nv (t - 1) + c"""
    B = np.zeros((T, J.shape[1], 3 * nv))
    for t in range(T):
        for c in range(3 * nv):
            G = nv * (t - 1) + c
            if 0 <= G < nv * T:
                B[t, :, c] = J[t, :, G]
    return B


# ------------------------------------------------------------------------------------------------------------------------ the window model
class Window:
    """s(q, v, a) = Ws tanh(Bq q + Bv v + Ba a + b) (a position-stage row has no v and a columns, a velocity-stage row no a columns; rows outside
    the sensors are filled too) and f(q, v, a) = M a + Wf tanh(Cq q + Cv v + c): smooth, with closed-form Jacobians."""

    def __init__(self, spec, T, seed):
        rng = np.random.default_rng(seed)
        self.spec, self.T = spec, T
        nv, nr = spec.nv, spec.nr
        st = np.full(nr, ACC); st[spec.first_row:spec.first_row + spec.ns] = spec.row_stage()
        self.Bq = rng.normal(0, 0.7, (nr, nv)); self.Bv = rng.normal(0, 0.3, (nr, nv)) * (st >= VEL)[:, None]
        self.Ba = rng.normal(0, 0.1, (nr, nv)) * (st >= ACC)[:, None]; self.b = rng.normal(0, 0.5, nr)
        self.Ws = rng.normal(0, 1.0, (nr, nr))
        L = rng.normal(0, 0.4, (nv, nv)); self.M = L @ L.T + np.eye(nv)
        self.Cq = rng.normal(0, 0.7, (nv, nv)); self.Cv = rng.normal(0, 0.3, (nv, nv)); self.c = rng.normal(0, 0.5, nv); self.Wf = rng.normal(0, 1.0, (nv, nv))
        # a smooth window, measurements off the predictions so that no residual is zero
        tt = np.arange(T)[:, None] * spec.h
        self.Q = rng.normal(0, 0.5, (1, nv)) + rng.normal(0, 1.0, (1, nv)) * tt + rng.normal(0, 2.0, (1, nv)) * tt ** 2 + rng.normal(0, 1e-3, (T, nv))
        self.y_sensor = rng.normal(0, 0.3, (T, spec.ns)); self.y_force = rng.normal(0, 0.3, (T, nv))

    def sensors(self, q, v, a):
        return self.Ws @ np.tanh(self.Bq @ q + self.Bv @ v + self.Ba @ a + self.b)

    def force(self, q, v, a):
        return self.M @ a + self.Wf @ np.tanh(self.Cq @ q + self.Cv @ v + self.c)

    def velacc(self, Q):
        T, h = self.T, self.spec.h
        V = np.zeros_like(Q); A = np.zeros_like(Q)
        V[1:] = (Q[1:] - Q[:-1]) / h
        A[1:T - 1] = (V[2:] - V[1:T - 1]) / h
        return V, A

    def predictions(self, Q):
        """raw sensor rows [T, ns] and forces [T, nv] of the window, ends evaluated as the optimiser evaluates them"""
        V, A = self.velacc(Q)
        sp = self.spec
        S = np.stack([self.sensors(Q[t], V[t], A[t])[sp.first_row:sp.first_row + sp.ns] for t in range(self.T)])
        F = np.stack([self.force(Q[t], V[t], A[t]) for t in range(self.T)])
        return S, F

    def raw_residuals(self, Q):
        S, F = self.predictions(Q)
        return S - self.y_sensor, F - self.y_force

    def cost(self, Q):
        rs, rf = zeroed_residuals(self.spec, self.T, *self.raw_residuals(Q))
        nt = Q.size
        return totals(self.spec, self.T, rs, rf, np.zeros((self.T, self.spec.ns, nt)), np.zeros((self.T, self.spec.nv, nt)))[0]

    def plus(self, Q, D):
        """Q (+) D for tangent increments D [T, nv]: plain addition on hinge dofs"""
        return Q + np.asarray(D).reshape(Q.shape)

    def jacobian(self, Q, eps):
        """dense J_s [T, ns, ntotal], J_f [T, nv, ntotal] by centred differences of the whole window's predictions, then the rows and blocks the
        optimiser drops at the two ends"""
        T, nv, sp = self.T, self.spec.nv, self.spec
        J_s = np.zeros((T, sp.ns, T * nv)); J_f = np.zeros((T, nv, T * nv))
        for G in range(T * nv):
            d = np.zeros(T * nv); d[G] = eps
            Sp, Fp = self.predictions(self.plus(Q, d.reshape(T, nv))); Sm, Fm = self.predictions(self.plus(Q, -d.reshape(T, nv)))
            J_s[:, :, G] = (Sp - Sm) / (2 * eps); J_f[:, :, G] = (Fp - Fm) / (2 * eps)
        for t in range(T):
            J_s[t] *= sp.jacobian_kept(T, t)[:, None]
        J_f[0] = 0.0; J_f[T - 1] = 0.0
        return J_s, J_f

    def reference(self, eps):
        J_s, J_f = self.jacobian(self.Q, eps)
        rs, rf = zeroed_residuals(self.spec, self.T, *self.raw_residuals(self.Q))
        cost, g, H = totals(self.spec, self.T, rs, rf, J_s, J_f)
        return dict(cost=cost, gradient=g, H=H, hessian_band=band_of(H, 3 * self.spec.nv), J_s=J_s, J_f=J_f, residual_sensor=rs, residual_force=rf)

    def inputs(self):
        """what the code under test is given: raw residuals, the closed-form blocks of every configuration (nothing zeroed at the ends, evaluated
        where a finite-difference call evaluates them) and the hinge dofs' velocity blocks"""
        T, nv, nr, h = self.T, self.spec.nv, self.spec.nr, self.spec.h
        V, A = self.velacc(self.Q)
        Df = [np.zeros((T, nv, nv)) for _ in range(3)]; Ds = [np.zeros((T, nr, nv)) for _ in range(3)]
        for t in range(T):
            q, v, a = self.Q[t], V[t], A[t]
            ds = self.Ws * (1 - np.tanh(self.Bq @ q + self.Bv @ v + self.Ba @ a + self.b) ** 2)[None, :]
            Ds[0][t], Ds[1][t], Ds[2][t] = ds @ self.Bq, ds @ self.Bv, ds @ self.Ba
            df = self.Wf * (1 - np.tanh(self.Cq @ q + self.Cv @ v + self.c) ** 2)[None, :]
            Df[0][t], Df[1][t], Df[2][t] = df @ self.Cq, df @ self.Cv, self.M
        V0 = np.tile(-np.eye(nv) / h, (T, 1, 1)); V1 = np.tile(np.eye(nv) / h, (T, 1, 1))
        V0[0] = np.nan; V1[0] = np.nan          # index 0 is not to be read
        rs, rf = self.raw_residuals(self.Q)
        rf[0] = np.nan; rf[T - 1] = np.nan          # nor are the force residuals of the ends
        return rs, rf, Df, Ds, V0, V1


class ModelWindow(Window):
    """A window on one of inverse_cases' contact-free hinge models: the predictions are tests/inv_ref.py's forces and inverse_cases.ref_residual's
    rows (tests/acc_ref.py, tests/table_ref.py) at (q_t, v_t, a_t), continuous inverse dynamics; velocities and accelerations are this
    file's own differences.  q_t = q_0 + t h v_0 + a seeded 1e-3 noise, so the force residual is far from zero.  Everything Window derives from
    predictions() (cost, the whole-window Jacobian by centred differences, g and H) is inherited."""

    def __init__(self, spec, T, case, seed, stored=None):
        """stored: dict(Q, y_sensor, y_force) of an earlier construction (the measurements cost two evaluations of the references)"""
        import inv_ref as ir
        rng = np.random.default_rng(seed)
        self.spec, self.T, self.case = spec, T, case
        m = case["model"]
        assert m["nq"] == m["nv"] == spec.nv and m["na"] == 0, "hinge and slide dofs only"
        self.ref = ir.InvRef(m)
        q0, v0 = case["X"][1][:spec.nv], case["X"][1][spec.nv:]
        self.Q = q0 + np.arange(T)[:, None] * spec.h * v0 + 1e-3 * rng.standard_normal((T, spec.nv))
        self.U = np.tile(case["U"][1], (T, 1)); self.time = 0.05 + spec.h * np.arange(T)
        if stored is not None:
            assert np.array_equal(self.Q, stored["Q"]), "the fixture belongs to another window"
            self.y_sensor, self.y_force = np.array(stored["y_sensor"]), np.array(stored["y_force"])
            return
        S, F = self.predictions(self.Q)
        self.y_sensor = S + rng.normal(0, 0.3, S.shape); self.y_force = F + rng.normal(0, 0.3, F.shape)

    def rows(self, Q):
        """(X [T, 2 nv], A [T, nv]) the window's evaluation rows, ends as the optimiser evaluates them"""
        V, A = self.velacc(Q)
        return np.hstack([Q, V]), A

    def predictions(self, Q):
        import inv_ref as ir
        import inverse_cases as ic
        X, A = self.rows(Q)
        sp = self.spec
        S = ic.ref_residual(self.case, X, self.U, A)[:, sp.first_row:sp.first_row + sp.ns]
        F = np.asarray(ir.evaluate(self.ref, self.case["model"], X, self.U, A)["qfrc_inverse"], float)
        return S, F

    def inputs(self, evaluate, differentiate):
        """what the code under test is given, from ITS evaluations: evaluate(X, U, A, time) -> (qfrc_inverse, residual), differentiate(X, U, A,
        time) -> the six blocks (dict), nothing zeroed; hinge velocity blocks"""
        T, nv, h = self.T, self.spec.nv, self.spec.h
        X, A = self.rows(self.Q)
        f, r = evaluate(X, self.U, A, self.time)
        sp = self.spec
        rs = np.asarray(r, float)[:, sp.first_row:sp.first_row + sp.ns] - self.y_sensor
        rf = np.asarray(f, float) - self.y_force
        o = differentiate(X, self.U, A, self.time)
        V0 = np.tile(-np.eye(nv) / h, (T, 1, 1)); V1 = np.tile(np.eye(nv) / h, (T, 1, 1))
        return (rs, rf, o["DfDq"], o["DfDv"], o["DfDa"], o["DsDq"], o["DsDv"], o["DsDa"], V0, V1)


# ------------------------------------------------------------------------------------------------------------------------ quaternion dofs
def quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def rotvec(q0, q1):
    """body-frame rotation vector of q0^-1 q1, angle in (-pi, pi]"""
    d = quat_mul(q0 * np.array([1.0, -1, -1, -1]), q1)
    s = np.linalg.norm(d[1:])
    if s < 1e-15:
        return np.zeros(3)
    ang = 2 * np.arctan2(s, d[0])
    if ang > np.pi:
        ang -= 2 * np.pi
    return d[1:] / s * ang


def joints(model):
    """[(type, qpos address, dof address)]; type 0 free, 1 ball, 2 slide, 3 hinge"""
    return [(int(model["jnt_type"][j]), int(model["jnt_qposadr"][j]), int(model["jnt_dofadr"][j])) for j in range(model["njnt"])]


def differentiate_pos(model, q0, q1, h):
    v = np.zeros(model["nv"])
    for typ, qa, da in joints(model):
        if typ == 0:
            v[da:da + 3] = (q1[qa:qa + 3] - q0[qa:qa + 3]) / h; v[da + 3:da + 6] = rotvec(q0[qa + 3:qa + 7], q1[qa + 3:qa + 7]) / h
        elif typ == 1:
            v[da:da + 3] = rotvec(q0[qa:qa + 4], q1[qa:qa + 4]) / h
        else:
            v[da] = (q1[qa] - q0[qa]) / h
    return v


def integrate_pos(model, q, dq):
    """q (+) dq: quaternions turned by the body-frame rotation vector"""
    out = np.array(q, float)
    for typ, qa, da in joints(model):
        if typ in (0, 1):
            if typ == 0:
                out[qa:qa + 3] += dq[da:da + 3]; qa += 3; da += 3
            w = dq[da:da + 3]; ang = np.linalg.norm(w)
            r = np.array([1.0, 0, 0, 0]) if ang == 0 else np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * w / ang])
            out[qa:qa + 4] = quat_mul(q[qa:qa + 4], r); out[qa:qa + 4] /= np.linalg.norm(out[qa:qa + 4])
        else:
            out[qa] += dq[da]
    return out


def velocity_blocks(model, q0, q1, h, eps=1e-6):
    """dv/dq0, dv/dq1 [nv, nv] of v = differentiate_pos(q0, q1) / h by centred differences over tangent nudges of either configuration"""
    nv = model["nv"]
    V0 = np.zeros((nv, nv)); V1 = np.zeros((nv, nv))
    for j in range(nv):
        d = np.zeros(nv); d[j] = eps
        V0[:, j] = (differentiate_pos(model, integrate_pos(model, q0, d), q1, h) - differentiate_pos(model, integrate_pos(model, q0, -d), q1, h)) / (2 * eps)
        V1[:, j] = (differentiate_pos(model, q0, integrate_pos(model, q1, d), h) - differentiate_pos(model, q0, integrate_pos(model, q1, -d), h)) / (2 * eps)
    return V0, V1


class RolloutWindow(ModelWindow):
    """A window on any of inverse_cases' models, quaternion joints and contacts included: Q [T, nq] is given (a short forward rollout with
    seeded tangent noise, direct_cases.rollout_window), velocities are differentiate_pos, nudges integrate_pos.  Predictions as ModelWindow:
    inv_ref forces (InvRef itself refuses a state within 1e-9 of a contact margin, for the window and for every nudged evaluation: NearMargin)
    and inverse_cases.ref_residual rows, continuous inverse dynamics."""

    def __init__(self, spec, T, case, Q, U, time, seed, stored=None):
        import inv_ref as ir
        rng = np.random.default_rng(seed)
        self.spec, self.T, self.case = spec, T, case
        self.model = case["model"]
        assert self.model["na"] == 0
        self.ref = ir.InvRef(self.model)
        self.Q, self.U, self.time = np.array(Q, float), np.array(U, float).reshape(T, -1), np.array(time, float)
        if stored is not None:
            assert np.array_equal(self.Q, stored["Q"]), "the fixture belongs to another window"
            self.y_sensor, self.y_force = np.array(stored["y_sensor"]), np.array(stored["y_force"])
            return
        S, F = self.predictions(self.Q)
        self.y_sensor = S + rng.normal(0, 0.3, S.shape); self.y_force = F + rng.normal(0, 0.3, F.shape)

    def plus(self, Q, D):
        D = np.asarray(D).reshape(self.T, self.spec.nv)
        return np.stack([integrate_pos(self.model, Q[t], D[t]) for t in range(self.T)])

    def velacc(self, Q):
        T, h, nv = self.T, self.spec.h, self.spec.nv
        V = np.zeros((T, nv)); A = np.zeros((T, nv))
        for t in range(1, T):
            V[t] = differentiate_pos(self.model, Q[t - 1], Q[t], h)
        A[1:T - 1] = (V[2:] - V[1:T - 1]) / h
        return V, A
