"""Independent float64 reference of the Allegro and OP3 task residuals (TEST INFRASTRUCTURE), restated from the reference's
mjpc/tasks/allegro/allegro.cc:36-77 and mjpc/tasks/op3/stand.cc:34-152 on top of tests/dyn_ref.py.

Frames and site frames come from DynRef.fk, a body's inertial-frame linear velocity from its com Jacobian (Jp v), subtree_com and
subtree_linvel from DynRef.subtree, a frame's quaternion from its rotation matrix, actuator_force from gain·ctrl + bias with the
force range, and the costs from mjpc/norm.cc.  It shares no code with `csrc/` or `oracle/`.
"""
from __future__ import annotations

import numpy as np
import torch

from dyn_ref import F64, DynRef

TASK_ALLEGRO, TASK_OP3 = 17, 18


def _t(x):
    return x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, float), dtype=F64)


def mat2quat(R):
    """unit quaternion (w, x, y, z) of rotation matrices [..., 3, 3] (Shepperd: the branch of the largest diagonal term)"""
    R = R.numpy() if torch.is_tensor(R) else np.asarray(R, float)
    out = np.zeros(R.shape[:-2] + (4,))
    for idx in np.ndindex(R.shape[:-2]):
        m = R[idx]
        tr = m[0, 0] + m[1, 1] + m[2, 2]
        k = int(np.argmax([tr, m[0, 0], m[1, 1], m[2, 2]]))
        if k == 0:
            s = 2.0 * np.sqrt(1.0 + tr); q = [0.25 * s, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s]
        elif k == 1:
            s = 2.0 * np.sqrt(1.0 + m[0, 0] - m[1, 1] - m[2, 2]); q = [(m[2, 1] - m[1, 2]) / s, 0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s]
        elif k == 2:
            s = 2.0 * np.sqrt(1.0 + m[1, 1] - m[0, 0] - m[2, 2]); q = [(m[0, 2] - m[2, 0]) / s, (m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s]
        else:
            s = 2.0 * np.sqrt(1.0 + m[2, 2] - m[0, 0] - m[1, 1]); q = [(m[1, 0] - m[0, 1]) / s, (m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s]
        out[idx] = q
    return out


def sub_quat(qa, qb):
    """mju_subQuat: the rotation vector v with qb * quat(v) = qa, i.e. the angle-axis of conj(qb) qa, angle wrapped to (-pi, pi]"""
    qa, qb = np.asarray(qa, float), np.asarray(qb, float)
    w1, x1, y1, z1 = qb[..., 0], -qb[..., 1], -qb[..., 2], -qb[..., 3]
    w2, x2, y2, z2 = qa[..., 0], qa[..., 1], qa[..., 2], qa[..., 3]
    d = np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                  w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)
    axis = d[..., 1:]
    s = np.linalg.norm(axis, axis=-1)
    angle = 2.0 * np.arctan2(s, d[..., 0])
    angle = np.where(angle > np.pi, angle - 2.0 * np.pi, angle)
    scale = np.where(s > 0, angle / np.where(s > 0, s, 1.0), 2.0)        # s -> 0: angle / s -> 2 / w (|w| = 1)
    return axis * scale[..., None]


def actuator_force(m, ref: DynRef, q, v, ctrl, jac):
    """gain·ctrl (clamped to ctrlrange) + bias0 + bias1·length + bias2·velocity, clamped to the force range (fixed gain, affine
    or no bias, no activations: what the two tasks' position servos need)"""
    assert m["na"] == 0
    u = ref.clamped_ctrl(_t(ctrl))
    length = ref.actuator_lengths(q)
    velocity = (ref.actuator_moments(jac) @ _t(v).unsqueeze(-1)).squeeze(-1)
    gain, bp = _t(m["actuator_gainprm"]), _t(m["actuator_biasprm"])
    affine = torch.as_tensor(np.asarray(m["actuator_biastype"]) == 1)
    f = gain[:, 0] * u + torch.where(affine, bp[:, 0] + bp[:, 1] * length + bp[:, 2] * velocity, torch.zeros_like(u))
    lim = torch.as_tensor(np.asarray(m["actuator_forcelimited"], bool))
    lo, hi = _t(m["actuator_forcerange"][:, 0]), _t(m["actuator_forcerange"][:, 1])
    return torch.where(lim, torch.minimum(torch.maximum(f, lo), hi), f)


class TaskRef:
    """residual(qpos [B, nq], qvel [B, nv], ctrl [B, nu]) -> [B, nr] numpy; cost(residual [..., nr]) -> [...]"""

    def __init__(self, m, task):
        self.m, self.task = m, task
        self.ref = DynRef(m)
        self.id = int(task["task_id"])
        assert self.id in (TASK_ALLEGRO, TASK_OP3)

    def residual(self, qpos, qvel, ctrl):
        q, v = _t(qpos), _t(qvel)
        jac = self.ref.jacobians(q)
        f = self.ref.fk(q)
        return self._allegro(q, v, ctrl, jac, f) if self.id == TASK_ALLEGRO else self._op3(q, v, ctrl, jac, f)

    def _allegro(self, q, v, ctrl, jac, f):
        """allegro.cc:36-77: cube − grasp site (framepos of a body: its inertial frame), subQuat(normalised goal, cube), cube
        inertial-frame linear velocity, actuator_force, qpos[7:23] − key_qpos[7:23], qvel[6:22]"""
        m, I = self.m, [int(x) for x in self.task["int_data"]]
        site, cube, goal, key = I
        xipos, ximat = f["xipos"].numpy(), f["ximat"]
        gq = mat2quat(ximat[:, goal]); gq = gq / np.linalg.norm(gq, axis=-1, keepdims=True)
        cq = mat2quat(ximat[:, cube])
        lin = (jac["Jp"][:, cube] @ v.unsqueeze(-1)).squeeze(-1).numpy()
        frc = actuator_force(m, self.ref, q, v, ctrl, jac).numpy()
        kq = np.asarray(m["key_qpos"], float)[key]
        qn, vn = q.numpy(), v.numpy()
        return np.concatenate([xipos[:, cube] - f["site_xpos"].numpy()[:, site], sub_quat(gq, cq), lin, frc,
                               qn[:, 7:23] - kq[7:23], vn[:, 6:22]], -1)

    def _op3(self, q, v, ctrl, jac, f):
        """stand.cc:34-152, row by row; the mode is int_data[0], the height goal parameters[0]"""
        m, I = self.m, [int(x) for x in self.task["int_data"]]
        mode, head, lf, rf, lh, rh, torso, body = I
        goal = float(self.task["parameters"][0])
        sp, sR = f["site_xpos"].numpy(), f["site_xmat"].numpy()
        com, comvel = self.ref.subtree(q, v, jac)
        com, comvel = com.numpy()[:, body], comvel.numpy()[:, body]
        zax = lambda s: sR[:, s, :, 2]                     # noqa: E731  framezaxis: third column of site_xmat
        yax = lambda s: sR[:, s, :, 1]                     # noqa: E731  frameyaxis: second column
        B = sp.shape[0]
        if mode == 0:
            height = sp[:, head, 2] - 0.5 * (sp[:, lf, 2] + sp[:, rf, 2])
        else:                                              # the reference's minus between the hands, kept
            height = 0.5 * (sp[:, lf, 2] + sp[:, rf, 2]) - 0.5 * (sp[:, lh, 2] - sp[:, rh, 2])
        cp = com + 0.05 * comvel
        a, b = (lf, rf) if mode == 0 else (lh, rh)
        avg = 0.5 * (sp[:, a, :2] + sp[:, b, :2]) - cp[:, :2]
        balance = np.linalg.norm(avg, axis=-1)
        key = np.asarray(m["key_qpos"], float)[mode]
        nu = m["nu"]
        z = np.array([0.0, 0.0, 1.0])
        if mode == 0:
            upright = np.concatenate([0.1 * (zax(rf) - z), 0.1 * (zax(lf) - z), zax(torso)[:, 2:3] - 1.0, np.zeros((B, 6))], -1)
        else:
            upright = np.concatenate([0.1 * (yax(rh) - z), 0.1 * (yax(lh) + z), 0.1 * (zax(rf) + z), 0.1 * (zax(lf) + z),
                                      zax(torso)[:, 2:3] + 1.0], -1)
        return np.concatenate([(height - goal)[:, None], balance[:, None], comvel[:, :2], np.asarray(ctrl, float) - key[7:7 + nu], upright,
                               v.numpy()[:, 6:]], -1)

    def cost(self, residual):
        """CostValue (mjpc/task.cc:71-110) with the norms of mjpc/norm.cc the two cost tables use; risk 0"""
        t = self.task
        r = np.asarray(residual, float)
        total = np.zeros(r.shape[:-1])
        start, pstart = 0, 0
        for k in range(int(t["num_term"])):
            n, norm, w = int(t["dim_norm_residual"][k]), int(t["norm"][k]), float(t["weight"][k])
            np_ = int(t["num_norm_parameter"][k])
            p = list(t["norm_parameter"][pstart:pstart + np_]) + [0.0, 0.0]
            x = r[..., start:start + n]
            if norm == 0:                                  # quadratic
                y = 0.5 * (x * x).sum(-1)
            elif norm == 1:                                # L22: ((|x|^2)^(q/2) + p^q)^(1/q) - p
                y = ((x * x).sum(-1) ** (p[1] / 2) + p[0] ** p[1]) ** (1 / p[1]) - p[0]
            elif norm == 2:                                # L2: sqrt(|x|^2 + p^2) - p
                y = np.sqrt((x * x).sum(-1) + p[0] * p[0]) - p[0]
            elif norm == 6:                                # smooth abs: sum sqrt(x_i^2 + p^2) - p
                y = (np.sqrt(x * x + p[0] * p[0]) - p[0]).sum(-1)
            else:
                raise NotImplementedError(f"norm {norm}")
            total = total + w * y
            start += n; pstart += np_
        assert abs(float(t["risk"])) < 1e-6
        return total
