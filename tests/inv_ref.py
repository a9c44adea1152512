"""Independent float64 reference of an inverse-dynamics evaluation (TEST INFRASTRUCTURE):

    qfrc_constraint = Jᵀ F(J a − aref)
    qfrc_inverse    = M a + c − passive − qfrc_constraint

from tests/dyn_ref.py (M, the bias c, the forces) and tests/con_ref.py (the constraint rows J, aref, R and the documented force law F
evaluated at a given jar).  Nothing is taken from the oracle or the kernel, nothing is solved or iterated.  The passive force is
DynRef.force of the model without its actuators, the actuator force the difference to DynRef.force of the whole model.

discrete: the given acceleration is the integrator's (v' − v) / h, which satisfies Â a_d = M a_c with Â the matrix of DynRef.step_system
for the model's integrator (Euler: M + h diag(damping); implicitfast: M − h ∂τ/∂v), so a_c = M⁻¹ Â a_d first.
"""
import numpy as np
import torch

from con_ref import NEAR, ConRef, NearMargin
from dyn_ref import DynRef, _t


class InvRef:
    def __init__(self, model):
        self.m = model
        self.dyn = DynRef(model)
        self.con = ConRef(model, self.dyn)
        self.passive_dyn = DynRef(model)
        self.passive_dyn.nu = 0                      # DynRef.force without the actuator terms
        self.h = float(model["timestep"])
        self.integrator = int(model["integrator"])

    def __call__(self, q, v, act, ctrl, a, discrete=False):
        """batched rows; returns dict of numpy arrays: qfrc_inverse, qfrc_constraint, qfrc_actuator, qacc (the continuous one), M,
        and per row ncon (contacts with rows), fmax (largest |constraint force| of a row), nefc"""
        m = self.m
        q = np.atleast_2d(np.asarray(q, float)); B = q.shape[0]
        v = np.asarray(v, float).reshape(B, m["nv"]); act = np.asarray(act, float).reshape(B, m["na"])
        ctrl = np.asarray(ctrl, float).reshape(B, m["nu"]); a = np.asarray(a, float).reshape(B, m["nv"])
        A, _, ex = self.dyn.step_system(q, v, act, ctrl, self.h, self.integrator)
        M, c, tau, jac = ex["M"], ex["c"], ex["tau"], ex["jac"]
        passive = self.passive_dyn.force(_t(q), _t(v), _t(act), _t(ctrl), jac)
        ta = _t(a)
        if discrete:
            ta = torch.linalg.solve(M, (A @ ta.unsqueeze(-1))).squeeze(-1)
        Ma = (M @ ta.unsqueeze(-1)).squeeze(-1)
        fk = self.dyn.fk(_t(q))
        xpos, xmat, xipos = fk["xpos"].numpy(), fk["xmat"].numpy(), fk["xipos"].numpy()
        Jp, Jr = jac["Jp"].numpy(), jac["Jr"].numpy()
        an = ta.numpy()
        qc = np.zeros((B, m["nv"])); ncon = np.zeros(B, int); fmax = np.zeros(B); nefc = np.zeros(B, int)
        for b in range(B):
            r = self.con.rows(q[b], v[b], xpos[b], xmat[b], xipos[b], Jp[b], Jr[b])
            if r["near"] < NEAR:
                raise NearMargin(f"row {b}: a candidate constraint row is {r['near']:.1e} from its margin")
            jar = r["J"] @ an[b] - r["aref"]
            F, _ = self.con.force(r, jar)
            qc[b] = r["J"].T @ F
            ncon[b] = r["ncon"]; nefc[b] = len(F); fmax[b] = np.abs(F).max() if len(F) else 0.0
        inv = Ma.numpy() + c.numpy() - passive.numpy() - qc
        return dict(qfrc_inverse=inv, qfrc_constraint=qc, qfrc_actuator=(tau - passive).numpy(), qacc=an, M=M.numpy(), ncon=ncon, fmax=fmax,
                    nefc=nefc)


def split(model, X):
    nq, nv = model["nq"], model["nv"]
    X = np.atleast_2d(np.asarray(X, float))
    return X[:, :nq], X[:, nq:nq + nv], X[:, nq + nv:]


def evaluate(ref, model, X, U, A, discrete=False):
    q, v, act = split(model, X)
    return ref(q, v, act, U, A, discrete)


def dev(got, want):
    """largest |got − want| / max(1, |want|)"""
    got, want = np.asarray(got, float), np.asarray(want, float)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))) if got.size else 0.0
