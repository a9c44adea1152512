"""Independent float64 reference of table-driven residuals (TEST INFRASTRUCTURE): reads the table of a MJPC_TASK_TABLE task as
include/mjpc_hip.h describes its encoding and evaluates it in numpy / torch on top of tests/dyn_ref.py.

Frames come from DynRef.fk (geoms from the body frame and geom_pos / geom_quat), quaternions from a quaternion chain of its own
(the same joint conventions as DynRef.fk, so the sign of a quaternion is the kinematic chain's), velocities from DynRef's
Jacobians: a point p of body b moves at Jp_b v + (Jr_b v) x (p - com_b), its frame turns at Jr_b v; subtree quantities from
DynRef.subtree; actuator forces from tests/task_ref.py: actuator_force.  It shares no code with `csrc/` and none with the Python
builder that wrote the table, so it also checks the builder's encoding against the header's description.
"""
from __future__ import annotations

import numpy as np
import torch

from dyn_ref import F64, DynRef, axis_angle, qmat, qmul, qnormalize
from mujoco_mpc_amd.modelgen.builder import BALL, FREE, SLIDE
from task_ref import actuator_force, sub_quat

# include/mjpc_hip.h
TASK_TABLE, VERSION = 19, 1
OP_SUM, OP_NORM, OP_SUBQUAT = 0, 1, 2
(CONST, PARAM, QPOS, QVEL, ACT, CTRL, ACTUATOR_FORCE, KEY_QPOS, MOCAP_POS, MOCAP_QUAT, MOCAP_MAT, SUBTREE_COM, SUBTREE_LINVEL,
 POS, QUAT, MAT, XAXIS, YAXIS, ZAXIS, LINVEL, ANGVEL) = range(21)
OBJ_BODY, OBJ_XBODY, OBJ_GEOM, OBJ_SITE = 1, 2, 5, 6
VELOCITY_KINDS = (SUBTREE_LINVEL, LINVEL, ANGVEL, ACTUATOR_FORCE)
KIND_NAMES = ["CONST", "PARAM", "QPOS", "QVEL", "ACT", "CTRL", "ACTUATOR_FORCE", "KEY_QPOS", "MOCAP_POS", "MOCAP_QUAT", "MOCAP_MAT",
              "SUBTREE_COM", "SUBTREE_LINVEL", "POS", "QUAT", "MAT", "XAXIS", "YAXIS", "ZAXIS", "LINVEL", "ANGVEL"]


def _t(x):
    return x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, float), dtype=F64)


def decode(task):
    """[(op, row, dim, ncomp, [(coef, kind, objtype, id, off)])] and the dbl_data array"""
    I = [int(x) for x in task["int_data"]]
    D = np.asarray(task["dbl_data"], float)
    assert int(task["task_id"]) == TASK_TABLE and I[0] == VERSION
    nb, nt = I[1], I[2]
    assert len(I) >= 3 + 6 * nb + 4 * nt and len(D) >= nt
    T = I[3 + 6 * nb:]
    blocks = []
    for b in range(nb):
        op, row, dim, ncomp, t0, n = I[3 + 6 * b: 9 + 6 * b]
        blocks.append((op, row, dim, ncomp, [(float(D[j]),) + tuple(T[4 * j: 4 * j + 4]) for j in range(t0, t0 + n)]))
    return blocks, D


def kinds_used(task):
    """{(kind, objtype or 0)} over the table's terms, the operations, whether some term has a non-zero offset"""
    blocks, _ = decode(task)
    kinds = {(k, ty if k >= POS else 0) for b in blocks for _, k, ty, _, _ in b[4]}
    return kinds, {b[0] for b in blocks}, any(off != 0 for b in blocks for *_, off in b[4])


def forces_ok(m):
    """whether task_ref.actuator_force covers the model: no activation states, no medium, no reference-site transmissions"""
    return m["na"] == 0 and not (m.get("density", 0) > 0 or m.get("viscosity", 0) > 0) and not np.any(np.asarray(m["actuator_refsite"]) >= 0)


class TableRef:
    """residual(states [B, nq+nv+na], ctrl [B, nu], mocap [7 nmocap] or None) -> [B, num_residual] numpy"""

    def __init__(self, m, task):
        self.m, self.task = m, task
        self.blocks, self.D = decode(task)
        # the kinematics of a model with a medium or with reference-site transmissions are the plain ones: DynRef only declines
        # their forces, which no source but ACTUATOR_FORCE reads
        plain = dict(m)
        self.forces_ok = forces_ok(m)
        if not self.forces_ok:
            plain["density"] = 0.0; plain["viscosity"] = 0.0; plain["actuator_refsite"] = np.full(m["nu"], -1)
        self.plain = plain
        self.ref = DynRef(plain)
        self.kinds = {k for b in self.blocks for _, k, *_ in b[4]}
        assert ACTUATOR_FORCE not in self.kinds or self.forces_ok, "no independent actuator forces for this model"

    def _qpos_unit(self, q):
        """qpos as the position stage leaves it: the quaternions of free and ball joints normalised (mj_kinematics)"""
        m = self.m
        out = q.clone()
        for j in range(m["njnt"]):
            t, qa = int(m["jnt_type"][j]), int(m["jnt_qposadr"][j])
            if t in (FREE, BALL):
                a = qa + (3 if t == FREE else 0)
                out[:, a:a + 4] = qnormalize(q[:, a:a + 4])
        return out

    def _xquat(self, q):
        """body quaternions [B, nb, 4] along the kinematic chain (the conventions of DynRef.fk)"""
        m, ref = self.m, self.ref
        B = q.shape[0]
        xq = [torch.zeros(B, 4, dtype=F64) + _t([1.0, 0, 0, 0])]
        for i in range(1, m["nbody"]):
            p = int(m["body_parentid"][i]); ja, jn = int(m["body_jntadr"][i]), int(m["body_jntnum"][i])
            if jn == 1 and m["jnt_type"][ja] == FREE:
                qa = int(m["jnt_qposadr"][ja])
                quat = qnormalize(q[:, qa + 3:qa + 7])
            else:
                quat = qmul(xq[p], ref.body_quat[i].expand(B, 4))
                for j in range(ja, ja + jn):
                    qa, t = int(m["jnt_qposadr"][j]), int(m["jnt_type"][j])
                    if t == SLIDE:
                        continue
                    ql = qnormalize(q[:, qa:qa + 4]) if t == BALL else axis_angle(ref.jnt_axis[j].expand(B, 3), q[:, qa:qa + 1] - ref.qpos0[qa])
                    quat = qmul(quat, ql)
                quat = qnormalize(quat)
            xq.append(quat)
        return torch.stack(xq, 1)

    def residual(self, states, ctrl, mocap=None):
        m = self.m
        nq, nv, na = m["nq"], m["nv"], m["na"]
        S = _t(states); q, v, act = S[:, :nq], S[:, nq:nq + nv], S[:, nq + nv:]
        u = _t(ctrl)
        B = q.shape[0]
        if m["nmocap"]:
            # a mocap body is a child of the world whose pose is the plan input's: the reference's kinematics take it as the body's
            # fixed offset (quaternion normalised, as the position stage does)
            mc7 = np.asarray(mocap, float).reshape(-1, 7)
            moved = dict(self.plain, body_pos=np.array(m["body_pos"], float), body_quat=np.array(m["body_quat"], float))
            for b in range(m["nbody"]):
                k = int(m["body_mocapid"][b])
                if k >= 0:
                    moved["body_pos"][b] = mc7[k, :3]; moved["body_quat"][b] = mc7[k, 3:] / np.linalg.norm(mc7[k, 3:])
            self.ref = DynRef(moved)
        f = self.ref.fk(q)
        xpos, xmat, xipos, ximat = f["xpos"], f["xmat"], f["xipos"], f["ximat"]
        gb = torch.as_tensor(np.asarray(m["geom_bodyid"], np.int64)); sb = torch.as_tensor(np.asarray(m["site_bodyid"], np.int64))
        gpos = xpos[:, gb] + (xmat[:, gb] @ _t(m["geom_pos"]).reshape(-1, 3).unsqueeze(-1)).squeeze(-1)
        gmat = xmat[:, gb] @ qmat(_t(m["geom_quat"]).reshape(-1, 4))
        xquat = self._xquat(q) if QUAT in self.kinds else None
        need_vel = bool(self.kinds & set(VELOCITY_KINDS))
        jac = self.ref.jacobians(q) if need_vel else None
        if need_vel:
            lin = (jac["Jp"] @ v[:, None, :, None]).squeeze(-1)           # com velocity of every body
            ang = (jac["Jr"] @ v[:, None, :, None]).squeeze(-1)
        sub = self.ref.subtree(q, v, jac) if (SUBTREE_LINVEL in self.kinds or SUBTREE_COM in self.kinds) else None
        frc = actuator_force(m, self.ref, q, v, u, jac) if ACTUATOR_FORCE in self.kinds else None
        mc = None if mocap is None else _t(mocap).reshape(-1, 7)
        P = _t(self.task["parameters"]) if int(self.task["num_parameter"]) else torch.zeros(0, dtype=F64)

        def frame(ty, i):
            """(origin, rotation matrix, body, quaternion or None) of an object"""
            if ty == OBJ_XBODY:
                return xpos[:, i], xmat[:, i], i, None if xquat is None else xquat[:, i]
            if ty == OBJ_BODY:
                return xipos[:, i], ximat[:, i], i, None if xquat is None else qmul(xquat[:, i], _t(m["body_iquat"][i]).expand(B, 4))
            if ty == OBJ_GEOM:
                b = int(m["geom_bodyid"][i])
                return gpos[:, i], gmat[:, i], b, None if xquat is None else qmul(xquat[:, b], _t(np.asarray(m["geom_quat"]).reshape(-1, 4)[i]).expand(B, 4))
            assert ty == OBJ_SITE, ty
            b = int(m["site_bodyid"][i])
            return f["site_xpos"][:, i], f["site_xmat"][:, i], b, None if xquat is None else qmul(xquat[:, b], _t(np.asarray(m["site_quat"]).reshape(-1, 4)[i]).expand(B, 4))

        def source(kind, ty, i):
            """the whole source vector [B, length]"""
            const = lambda x: _t(x).reshape(1, -1).expand(B, -1)           # noqa: E731
            if kind == CONST: return const(self.D[i:i + ty])
            if kind == PARAM: return P.reshape(1, -1).expand(B, -1)
            if kind == QPOS: return self._qpos_unit(q)
            if kind == QVEL: return v
            if kind == ACT: assert na > 0; return act
            if kind == CTRL: return u
            if kind == ACTUATOR_FORCE: return frc
            if kind == KEY_QPOS: return const(np.asarray(m["key_qpos"], float)[i])
            if kind == MOCAP_POS: return mc[i, :3].reshape(1, 3).expand(B, 3)
            if kind == MOCAP_QUAT: return mc[i, 3:].reshape(1, 4).expand(B, 4)
            if kind == MOCAP_MAT: return qmat(mc[i, 3:]).reshape(1, 9).expand(B, 9)
            if kind == SUBTREE_COM: return sub[0][:, i]
            if kind == SUBTREE_LINVEL: return sub[1][:, i]
            p, R, b, quat = frame(ty, i)
            if kind == POS: return p
            if kind == QUAT: return quat
            if kind == MAT: return R.reshape(B, 9)
            if kind in (XAXIS, YAXIS, ZAXIS): return R[:, :, kind - XAXIS]
            if kind == ANGVEL: return ang[:, b]
            assert kind == LINVEL, kind
            return lin[:, b] + torch.cross(ang[:, b], p - xipos[:, b], dim=-1)

        out = np.full((B, int(self.task["num_residual"])), np.nan)
        for op, row, dim, ncomp, terms in self.blocks:
            if op == OP_SUBQUAT:
                (c0, k0, ty0, i0, _), (_, k1, ty1, i1, _) = terms
                out[:, row:row + 3] = c0 * sub_quat(source(k0, ty0, i0).numpy(), source(k1, ty1, i1).numpy())
                continue
            val = torch.zeros(B, ncomp, dtype=F64)
            for c, k, ty, i, off in terms:
                val = val + c * source(k, ty, i)[:, off:off + ncomp]
            if op == OP_NORM:
                out[:, row] = torch.sqrt((val * val).sum(-1)).numpy()
            else:
                assert op == OP_SUM and ncomp == dim
                out[:, row:row + dim] = val.numpy()
        assert not np.isnan(out).any(), "the blocks do not cover every row"
        return out
