"""Independent float64 references of the late residual rows (TEST INFRASTRUCTURE): accelerations of frames and the touch sum, on top of
tests/dyn_ref.py and tests/con_ref.py.  Shares nothing with `csrc/` or `oracle/`.

Kinematic reference.  With p(q), R(q) of DynRef.fk and the curve q(s) = integratePos(q, v, s),

    v_p = d/ds p(q(s))|0                     ω = vee(d/ds R(q(s)) Rᵀ)|0
    a   = d²/ds² p(q(s))|0 + Jp·qacc − g     α = d/ds ω(q(s))|0 + Jr·qacc

all by forward-mode autodiff (Jp·qacc and Jr·qacc as the derivative of fk∘integratePos(q, δ, 1) at δ = 0 along qacc): no spatial
algebra, no recursion over the tree.  a is what framelinacc reports (it carries −gravity), α what frameangacc reports; accelerometer,
velocimeter and gyro are Rᵀ a, Rᵀ v_p, Rᵀ ω of a site.

Touch reference.  ConRef's contact rows of the state and its force law at jar = J·qacc − aref for the qacc that is handed in (the
engine's own, read through a QACC block), then the documented inclusion rule: a contact counts when one of its geoms sits on the site's
body, its normal force is positive and its position lies inside the zone.
"""
from __future__ import annotations

import numpy as np
import torch
from torch.func import jvp

from con_ref import ConRef
from dyn_ref import F64, DynRef, _t, vee

FRAMES = {"xbody": ("xpos", "xmat"), "body": ("xipos", "ximat"), "site": ("site_xpos", "site_xmat")}
EDGE = 1e-9                    # a contact point this close to a zone's boundary: the case is ill-posed (pick another state)


class NearZone(AssertionError):
    """a contact point sits within EDGE of a zone boundary: whether it counts is decided by round-off"""


class AccRef:
    def __init__(self, m, dyn=None):
        self.m = m
        self.dyn = dyn or DynRef(m)

    def qacc_smooth(self, q, v, act, ctrl):
        """M⁻¹ (τ − c): the acceleration of a state without active constraints"""
        _, f, ex = self.dyn.step_system(q, v, act, ctrl, float(self.m["timestep"]), 0)
        return torch.linalg.solve(ex["M"], f.unsqueeze(-1)).squeeze(-1).numpy()

    def frame(self, objtype, i, q, v, qacc):
        """dict(R, linvel, angvel, linacc, angacc) [B, ...] of frame i of `objtype` ("xbody", "body", "site"), world coordinates"""
        d = self.dyn
        q, v, qacc = _t(q), _t(v), _t(qacc)
        kp, kr = FRAMES[objtype]
        s0 = torch.zeros((), dtype=F64); one = torch.ones((), dtype=F64)

        def at(qq):
            f = d.fk(qq)
            return f[kp][..., i, :], f[kr][..., i, :, :]

        def vel(s):
            (p, R), (pd, Rd) = jvp(lambda t: at(d.integrate_pos(q, v, t)), (s,), (one,))
            return pd, vee(Rd, R)
        (pd, w), (pdd, wd) = jvp(vel, (s0,), (one,))
        zero = torch.zeros_like(v)
        (p, R), (pa, Ra) = jvp(lambda dl: at(d.integrate_pos(q, dl, 1.0)), (zero,), (qacc,))
        return dict(R=R.numpy(), linvel=pd.numpy(), angvel=w.numpy(), linacc=(pdd + pa - d.gravity).numpy(), angacc=(wd + vee(Ra, R)).numpy())

    def local(self, fr, key):
        """Rᵀ x: the world vector fr[key] in the frame's own coordinates"""
        return np.einsum("bji,bj->bi", fr["R"], fr[key])


def in_zone(shape, p, size):
    """(inside, distance of the deciding quantity from the boundary) for p in site coordinates; MuJoCo's size conventions"""
    x, y, z = (float(c) for c in p); s = [float(c) for c in size]
    if shape == "sphere":
        g = [np.sqrt(x * x + y * y + z * z) - s[0]]
    elif shape == "box":
        g = [abs(x) - s[0], abs(y) - s[1], abs(z) - s[2]]
    elif shape == "ellipsoid":
        g = [(x / s[0]) ** 2 + (y / s[1]) ** 2 + (z / s[2]) ** 2 - 1.0]
    elif shape == "cylinder":
        g = [np.sqrt(x * x + y * y) - s[0], abs(z) - s[1]]
    elif shape == "capsule":
        dz = z - min(max(z, -s[1]), s[1])
        g = [np.sqrt(x * x + y * y + dz * dz) - s[0]]
    else:
        raise KeyError(shape)
    return all(c <= 0 for c in g), min(abs(c) for c in g)


class TouchRef:
    """zones: [(site id, shape name, size)]"""

    def __init__(self, m, zones, con=None):
        self.m = m
        self.con = con or ConRef(m)
        self.zones = list(zones)

    def contacts(self, xpos, xmat):
        """[(geom1, geom2, pos)] of the contacts that have rows, in the order ConRef.rows appends their groups"""
        m, c = self.m, self.con
        from dyn_ref import qmat
        gb = np.asarray(m["geom_bodyid"], int)
        gx = xpos[gb] + np.einsum("gij,gj->gi", xmat[gb], np.asarray(m["geom_pos"], float))
        gR = xmat[gb] @ qmat(_t(m["geom_quat"])).numpy()
        out = []
        for g1, g2 in c.pairs:
            _, _, _, _, margin, gap = c.contact_param(g1, g2)
            for dist, pos, _, _ in c._narrow(g1, g2, gx, gR):
                if dist < margin - gap:
                    out.append((g1, g2, pos))
        return out

    def __call__(self, q, v, qacc):
        """one state: dict(touch=[per zone], forces=[normal force per contact], included=[per zone: contact indices], near=the
        smallest distance of a contact point of the zone's body with a positive force from a zone boundary)"""
        m, dyn = self.m, self.con.dyn
        qq = _t(np.asarray(q, float)[None])
        fk = dyn.fk(qq); jac = dyn.jacobians(qq)
        xpos, xmat, xipos = fk["xpos"][0].numpy(), fk["xmat"][0].numpy(), fk["xipos"][0].numpy()
        r = self.con.rows(np.asarray(q, float), np.asarray(v, float), xpos, xmat, xipos, jac["Jp"][0].numpy(), jac["Jr"][0].numpy())
        F, _ = self.con.force(r, r["J"] @ np.asarray(qacc, float) - r["aref"])
        cons = self.contacts(xpos, xmat)
        groups = r["groups"][len(r["groups"]) - len(cons):] if cons else []
        assert len(cons) == r["ncon"] and all(g[0] in ("ell", "pyr", "pos") for g in groups)
        normal = [float(F[k0:k0 + n].sum()) if kind == "pyr" else float(F[k0]) for kind, k0, n, _ in groups]
        sx, sR = fk["site_xpos"][0].numpy(), fk["site_xmat"][0].numpy()
        touch, included, near = [], [], np.inf
        for site, shape, size in self.zones:
            body = int(m["site_bodyid"][site]); tot, inc = 0.0, []
            for k, (g1, g2, pos) in enumerate(cons):
                if body not in (int(m["geom_bodyid"][g1]), int(m["geom_bodyid"][g2])) or not normal[k] > 0:
                    continue
                inside, edge = in_zone(shape, sR[site].T @ (pos - sx[site]), size)
                near = min(near, edge)
                if inside:
                    tot += normal[k]; inc.append(k)
            touch.append(tot); included.append(inc)
        return dict(touch=np.array(touch), forces=np.array(normal), included=included, near=near, contacts=cons)
