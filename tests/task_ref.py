"""Independent float64 reference of task residuals and costs (TEST INFRASTRUCTURE), restated from the reference's own sources on top
of tests/dyn_ref.py:

    Allegro (17)             mjpc/tasks/allegro/allegro.cc:36-77
    OP3 (18)                 mjpc/tasks/op3/stand.cc:34-152
    Quadruped flat (2)       mjpc/tasks/quadruped/quadruped.cc:33-221, 602-714 and quadruped.h, Ground() of mjpc/utilities.cc:537-556
    Humanoid tracking (4)    mjpc/tasks/humanoid/tracking/tracking.cc:27-216
    Humanoid walk (6)        mjpc/tasks/humanoid/walk/walk.cc:44-165
    Humanoid interact (15)   mjpc/tasks/humanoid/interact/interact.cc:29-198

Frames and site frames come from DynRef.fk (mocap bodies from the mocap input, quaternion normalised; geom frames from geom_pos /
geom_quat on the body frame), framelinvel of a site from Sp v and of a body from its com Jacobian (Jp v), subtree_com and
subtree_linvel from DynRef.subtree, a frame's quaternion from its rotation matrix, actuator_force from gain*ctrl + bias with the
force range, the ground height from a ray reference of its own (plane by its normal distance, sphere by the closest approach of the
line, box by the slab method), the costs from the nine norms of mjpc/norm.cc and the risk transform of mjpc/task.cc:94-110 (expm1).
It shares no code with `csrc/`, `oracle/` or `modelgen/residual_table.py`.

After residual(), `margin` holds per case the distance of the reference's own numbers to every point where a row may legitimately
flip on a 1-ulp difference (the |value| < 1e-6 snap of the step height, which geom a ray meets first, a ray footprint on a box edge
or a sphere's silhouette, the Scramble min(0, .), the flip's phase boundaries, kMinAngvel, a key-frame index on an integer); a case
generator rejects cases that are close, and a test on undesigned states may skip rows that are closer than 1e-9.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import torch

from dyn_ref import F64, DynRef

TASK_QUADRUPED, TASK_TRACK, TASK_WALK, TASK_INTERACT, TASK_ALLEGRO, TASK_OP3 = 2, 4, 6, 15, 17, 18
MINVAL = 1e-15                # mjMINVAL


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


def quat2mat(q):
    """rotation matrices [..., 3, 3] of unit quaternions (w, x, y, z)"""
    q = np.asarray(q, float)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def mul_quat(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.stack([a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1] - a[..., 2] * b[..., 2] - a[..., 3] * b[..., 3],
                     a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0] + a[..., 2] * b[..., 3] - a[..., 3] * b[..., 2],
                     a[..., 0] * b[..., 2] - a[..., 1] * b[..., 3] + a[..., 2] * b[..., 0] + a[..., 3] * b[..., 1],
                     a[..., 0] * b[..., 3] + a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1] + a[..., 3] * b[..., 0]], -1)


def normalize(v):
    """mju_normalize: v / |v|, or the first unit vector where |v| < mjMINVAL"""
    v = np.asarray(v, float)
    n = np.sqrt((v * v).sum(-1, keepdims=True))
    e0 = np.zeros_like(v); e0[..., 0] = 1.0
    return np.where(n < MINVAL, e0, v / np.where(n < MINVAL, 1.0, n))


def as_int(x):
    """ReinterpretAsInt (mjpc/utilities.cc:100-102) of one double: its low 32 bits, as the select parameters are stored"""
    return int(np.array([x], np.float64).view(np.int32)[0])


def c_fmod(a, b):
    """C fmod: the result has the sign of a (Python's % has the sign of b)"""
    return np.fmod(a, b)


def frames(ref: DynRef, m, q, mocap=None):
    """DynRef.fk with the mocap bodies placed by the mocap input ([nmocap * 7] or [B, nmocap * 7]: position, then the quaternion,
    which is normalised) and the geom frames geom_xpos = xpos + xmat geom_pos, geom_xmat = xmat mat(geom_quat); numpy, batch first"""
    f = {k: x.numpy().copy() for k, x in ref.fk(q).items()}
    B = f["xpos"].shape[0]
    if int(m.get("nmocap", 0)):
        mp = np.broadcast_to(np.asarray(mocap, float).reshape(-1, int(m["nmocap"]), 7), (B, int(m["nmocap"]), 7))
        for b in range(int(m["nbody"])):
            k = int(m["body_mocapid"][b])
            if k >= 0:
                qn = mp[:, k, 3:] / np.linalg.norm(mp[:, k, 3:], axis=-1, keepdims=True)
                f["xpos"][:, b] = mp[:, k, :3]; f["xmat"][:, b] = quat2mat(qn)
        f["mocap_pos"] = mp[:, :, :3].copy()
    gb = np.asarray(m["geom_bodyid"], int)
    gpos, gquat = np.asarray(m["geom_pos"], float).reshape(-1, 3), np.asarray(m["geom_quat"], float).reshape(-1, 4)
    f["geom_xpos"] = f["xpos"][:, gb] + np.einsum("bgij,gj->bgi", f["xmat"][:, gb], gpos)
    f["geom_xmat"] = np.einsum("bgij,gjk->bgik", f["xmat"][:, gb], quat2mat(gquat / np.linalg.norm(gquat, axis=-1, keepdims=True)))
    return f


# ----------------------------------------------------------------------------------- the ground ray
GEOM_PLANE, GEOM_SPHERE, GEOM_BOX = 0, 2, 6


def _ray_geom(pnt, gpos, gmat, size, gtype):
    """distance along (0, 0, -1) from pnt [n, 3] to a geom's surface (-1: no hit at a non-negative distance) and the margin [n]: how
    far the ray is from changing between hit and miss or between the faces it meets (inf where nothing of the kind is near)"""
    lp = np.einsum("nji,nj->ni", gmat, pnt - gpos)                   # the ray in the geom's frame
    lv = -gmat[:, 2, :]                                              # gmat^T (0, 0, -1)
    n = pnt.shape[0]
    if gtype == GEOM_PLANE:                                          # the plane z = 0, met from above only, inside its half sizes
        down = lv[:, 2] < -MINVAL
        x = -lp[:, 2] / np.where(down, lv[:, 2], -1.0)
        p = lp + x[:, None] * lv
        margin = np.where(down, np.abs(x), np.inf)
        hit = down & (x >= 0)
        for i in range(2):
            if size[i] > 0:
                hit &= np.abs(p[:, i]) <= size[i]
                margin = np.minimum(margin, np.abs(np.abs(p[:, i]) - size[i]))
        return np.where(hit, x, -1.0), margin
    if gtype == GEOM_SPHERE:                                         # closest approach of the line to the centre, then half the chord
        tca = -(lp * lv).sum(-1)
        d2 = (lp * lp).sum(-1) - tca * tca
        miss = size[0] * size[0] - d2 < MINVAL
        thc = np.sqrt(np.where(miss, 0.0, size[0] * size[0] - d2))
        x0, x1 = tca - thc, tca + thc
        x = np.where(x0 >= 0, x0, np.where(x1 >= 0, x1, -1.0))
        margin = np.minimum(np.abs(size[0] - np.sqrt(np.maximum(d2, 0.0))), np.minimum(np.abs(x0), np.abs(x1)))
        return np.where(miss, -1.0, x), np.where(miss, np.abs(size[0] - np.sqrt(np.maximum(d2, 0.0))), margin)
    if gtype == GEOM_BOX:                                            # slab method: the ray is inside the box between lo and hi
        lo, hi = np.full(n, -np.inf), np.full(n, np.inf)
        margin = np.full(n, np.inf)
        outside = np.zeros(n, bool)
        for i in range(3):
            par = np.abs(lv[:, i]) < MINVAL
            den = np.where(par, 1.0, lv[:, i])
            t1, t2 = (-size[i] - lp[:, i]) / den, (size[i] - lp[:, i]) / den
            lo = np.where(par, lo, np.maximum(lo, np.minimum(t1, t2)))
            hi = np.where(par, hi, np.minimum(hi, np.maximum(t1, t2)))
            outside |= par & (np.abs(lp[:, i]) > size[i])
            margin = np.where(par, np.minimum(margin, np.abs(np.abs(lp[:, i]) - size[i])), margin)
        hit = ~outside & (lo <= hi) & (hi >= 0)
        x = np.where(lo >= 0, lo, hi)
        margin = np.minimum(margin, np.where(outside, np.inf, np.minimum(np.abs(hi - lo), np.minimum(np.abs(lo), np.abs(hi)))))
        return np.where(hit, x, -1.0), margin
    raise NotImplementedError(f"ground ray at a geom of type {gtype}")


def ground(m, f, pos):
    """Ground() (mjpc/utilities.cc:537-556): a ray straight down from 0.5 above pos [B, 3] at the geoms of group 0 (static ones
    included, no body excluded), the height of the nearest hit; and the margin [B]: the smallest of the geoms' own margins and the gap
    between the nearest hit and the next one.  No hit at all is an error, as it is in the reference."""
    B = pos.shape[0]
    pnt = pos + np.array([0.0, 0.0, 0.5])
    best, second, margin = np.full(B, np.inf), np.full(B, np.inf), np.full(B, np.inf)
    for g in np.flatnonzero(np.asarray(m["geom_group"], int) == 0):
        x, mg = _ray_geom(pnt, f["geom_xpos"][:, g], f["geom_xmat"][:, g], np.asarray(m["geom_size"], float).reshape(-1, 3)[g], int(m["geom_type"][g]))
        x = np.where(x >= 0, x, np.inf)
        second = np.where(x < best, best, np.minimum(second, x))
        best = np.minimum(best, x)
        margin = np.minimum(margin, mg)
    if not np.isfinite(best).all():
        raise ValueError("no group 0 geom detected by raycast")
    return pnt[:, 2] - best, np.minimum(margin, second - best)


GAIT_PHASE = np.array([[0, 0, 0, 0], [0, 0.75, 0.5, 0.25], [0, 0.5, 0.5, 0], [0, 0.33, 0.33, 0.66], [0, 0.4, 0.05, 0.35]])   # quadruped.h:77-85
MODE_QUADRUPED, MODE_BIPED, MODE_WALK, MODE_SCRAMBLE, MODE_FLIP = range(5)
FOOT_FL, FOOT_HL, FOOT_FR, FOOT_HR = range(4)
NORM_NPARAM = {-1: 0, 0: 0, 1: 2, 2: 1, 3: 1, 5: 1, 6: 1, 7: 2, 8: 1}


class TaskRef:
    """residual(qpos [B, nq], qvel [B, nv], ctrl [B, nu], time [B] or scalar, mocap [nmocap * 7] or [B, nmocap * 7]) -> [B, nr] numpy
    (Allegro and OP3 ignore time and mocap); cost(residual [..., nr]) -> [...]; margin: see the module docstring; entered: which
    branches the last residual() took, per case"""

    def __init__(self, m, task):
        self.m, self.task = m, task
        self.ref = DynRef(m)
        self.id = int(task["task_id"])
        assert self.id in (TASK_QUADRUPED, TASK_TRACK, TASK_WALK, TASK_INTERACT, TASK_ALLEGRO, TASK_OP3)
        self.margin, self.entered = None, {}

    def residual(self, qpos, qvel, ctrl, time=0.0, mocap=None, jac=None):
        """jac: DynRef.jacobians(qpos) where the caller has them already (they depend on the model and qpos only)"""
        q, v = _t(qpos), _t(qvel)
        jac = self.ref.jacobians(q) if jac is None else jac
        if self.id in (TASK_ALLEGRO, TASK_OP3):
            f = self.ref.fk(q)
            return self._allegro(q, v, ctrl, jac, f) if self.id == TASK_ALLEGRO else self._op3(q, v, ctrl, jac, f)
        f = frames(self.ref, self.m, q, mocap)
        time = np.broadcast_to(np.asarray(time, float), (q.shape[0],))
        fn = {TASK_QUADRUPED: self._quadruped, TASK_TRACK: self._tracking, TASK_WALK: self._walk, TASK_INTERACT: self._interact}[self.id]
        self.margin = np.full(q.shape[0], np.inf); self.entered = {}
        return fn(q, v, np.asarray(ctrl, float), time, jac, f)

    # ------------------------------------------------------------------------------- quadruped flat
    def _quadruped(self, q, v, ctrl, time, jac, f):
        """quadruped.cc:33-221 row by row.  Task state as the engine receives it: int_data = [trunk, head site, goal mocap id, foot
        geoms FL HL FR HR, parameter indices gait / gait switch / flip direction / biped type / cadence / amplitude / duty / heading, home key,
        crouch key, mode]; dbl_data = [mode_start_time, position_[3], heading_[2], speed_, angvel_, ground_, orientation_[4],
        current_gait_, phase_start_, phase_start_time_, phase_velocity_, gravity, jump_vel_, flight_time_, jump_acc_, crouch_time_,
        leap_time_, jump_time_, crouch_vel_, land_time_, land_acc_, flight_rot_vel_, jump_rot_vel_, jump_rot_acc_, land_rot_acc_]"""
        m = self.m
        I = [int(x) for x in self.task["int_data"]]; D = np.asarray(self.task["dbl_data"], float); P = np.asarray(self.task["parameters"], float)
        trunk, head, goal_id, feet, mode = I[0], I[1], I[2], I[3:7], I[-1]
        p_flip, p_biped, p_amp, p_duty, p_heading, k_home, k_crouch = I[9], I[10], I[12], I[13], I[14], I[15], I[16]
        (t0, position, heading, speed, angvel, ground0, orientation, gait_d, phase0, phase_t0, phase_vel) = (
            D[0], D[1:4], D[4:6], D[6], D[7], D[8], D[9:13], D[13], D[14], D[15], D[16])
        jump_vel, flight, jump_acc, crouch_t, jump_t, crouch_vel, land_t, land_acc = D[18], D[19], D[20], D[21], D[23], D[24], D[25], D[26]
        flight_rot_vel, jump_rot_vel, jump_rot_acc, land_rot_acc = D[27], D[28], D[29], D[30]
        B = q.shape[0]
        qn = q.numpy()
        foot = f["geom_xpos"][:, feet]                                                       # [B, 4, 3]: FL HL FR HR
        R = f["xmat"][:, trunk]
        torso_pos = f["xipos"][:, trunk]
        goal = f["mocap_pos"][:, goal_id]
        com, comvel = self.ref.subtree(q, v, jac)
        com, comvel = com.numpy()[:, trunk], comvel.numpy()[:, trunk]
        handstand = int(as_int(P[p_biped])) != 0
        T = time - t0
        margin = self.margin
        # average foot position (quadruped.cc:603-619)
        if mode == MODE_BIPED:
            avg = 0.5 * ((foot[:, FOOT_FL] + foot[:, FOOT_FR]) if handstand else (foot[:, FOOT_HL] + foot[:, FOOT_HR]))
        else:
            avg = 0.25 * (foot[:, FOOT_HL] + foot[:, FOOT_HR] + foot[:, FOOT_FL] + foot[:, FOOT_FR])
        # flip phases (quadruped.cc:676-714): 0 crouch, 1 leap, 2 flight, 3 land, 4 done
        bounds = np.array([crouch_t, jump_t, jump_t + flight, jump_t + flight + land_t])
        phase_id = (T[:, None] >= bounds[None, :]).sum(-1)
        if mode == MODE_FLIP:
            away = np.abs(T[:, None] - bounds[None, :])
            margin = np.minimum(margin, np.where(away == 0, np.inf, away).min(-1))           # a time ON a boundary compares alike on both sides
            self.entered["flip_phase"] = phase_id
            self.entered["flip_on_boundary"] = (away == 0).any(-1)
        rows = []
        # ---------- upright
        if mode != MODE_FLIP:
            up = (R[:, 2, 0] - (-1 if handstand else 1)) if mode == MODE_BIPED else R[:, 2, 2] - 1
            rows += [up[:, None], np.zeros((B, 2))]
        else:
            angle = np.zeros(B)
            s = T - crouch_t; angle = np.where(phase_id == 1, 0.5 * jump_rot_acc * s * s + jump_rot_vel * s, angle)
            s = T - jump_t; angle = np.where(phase_id == 2, np.pi / 2 + flight_rot_vel * s, angle)
            s = T - (jump_t + flight); angle = np.where(phase_id == 3, 1.75 * np.pi + flight_rot_vel * s - 0.5 * land_rot_acc * s * s, angle)
            angle = np.where(phase_id == 4, 2 * np.pi, angle)
            ay = 1.0 if int(as_int(P[p_flip])) else -1.0
            aq = np.stack([np.cos(angle / 2), np.zeros(B), ay * np.sin(angle / 2), np.zeros(B)], -1)
            rows.append(sub_quat(mat2quat(R), mul_quat(np.broadcast_to(orientation, (B, 4)), aq)))
        # ---------- height
        hgoal = 0.6 if mode == MODE_BIPED else 0.25
        if mode == MODE_SCRAMBLE:
            rows.append(np.zeros((B, 1)))
        elif mode == MODE_FLIP:
            h = 0.25 + T * crouch_vel + 0.5 * T * T * jump_acc                               # before jump_time_, the crouch included
            s = T - jump_t; h = np.where(phase_id == 2, 0.5 + jump_vel * s - 0.5 * 9.81 * s * s, h)
            s = T - (jump_t + flight); h = np.where(phase_id == 3, 0.5 - jump_vel * s + 0.5 * land_acc * s * s, h)
            h = np.where(phase_id == 4, 0.25, h)
            rows.append((torso_pos[:, 2] - (h + ground0))[:, None])
        else:
            rows.append(((torso_pos[:, 2] - avg[:, 2]) - hgoal)[:, None])
        # ---------- position
        target = goal.copy()
        if mode == MODE_WALK:                                                                # quadruped.cc:627-643
            margin = np.minimum(margin, abs(abs(angvel) - 0.01))
            self.entered["walk_turning"] = np.full(B, abs(angvel) >= 0.01)
            if abs(angvel) < 0.01:
                fw = normalize(heading)
                target[:, :2] = position[:2] + heading + (T * speed)[:, None] * fw
            else:
                a = T * angvel
                target[:, 0] = np.cos(a) * heading[0] - np.sin(a) * heading[1] + position[0]
                target[:, 1] = np.sin(a) * heading[0] + np.cos(a) * heading[1] + position[1]
        hd = f["site_xpos"][:, head]
        rows.append(np.stack([hd[:, 0] - target[:, 0], hd[:, 1] - target[:, 1],
                              2 * (hd[:, 2] - target[:, 2]) if mode == MODE_SCRAMBLE else np.zeros(B)], -1))
        # ---------- gait
        gait = 2 if mode == MODE_BIPED else int(as_int(gait_d))
        self.entered["gait"] = np.full(B, gait)
        phase = phase0 + (time - phase_t0) * phase_vel
        amp, duty = P[p_amp], P[p_duty]
        stepped = np.zeros((B, 4), bool)
        for k in range(4):
            if mode == MODE_BIPED and ((not handstand and k in (FOOT_FL, FOOT_FR)) or (handstand and k in (FOOT_HL, FOOT_HR))):
                rows.append(np.zeros((B, 1)))
                continue
            ang = c_fmod(phase + np.pi - 2 * np.pi * GAIT_PHASE[gait][k], 2 * np.pi) - np.pi
            val = np.zeros(B)
            if duty < 1:
                ang = ang * (0.5 / (1 - duty))
                val = np.cos(np.clip(ang, -np.pi / 2, np.pi / 2))
                # cos falls below 1e-6 at |angle| = pi/2 - 1e-6 (slope 1 there) and stays there on the clipped arm: the one place the snap flips
                margin = np.minimum(margin, np.abs(np.abs(ang) - (np.pi / 2 - 1e-6)))
            val = np.where(np.abs(val) < 1e-6, 0.0, val)
            step = amp * val
            query = foot[:, k].copy()
            if mode == MODE_SCRAMBLE:
                to_goal = goal - foot[:, k]
                to_goal[:, 2] = 0
                query = query + 0.15 * normalize(to_goal)
            gh, gm = ground(m, f, query)
            diff = foot[:, k, 2] - (gh + 0.02 + step)
            if mode == MODE_SCRAMBLE:
                margin = np.minimum(margin, np.where(step != 0, np.abs(diff), np.inf))
                self.entered.setdefault("scramble_above", []).append(np.where(step != 0, diff > 0, False))
                self.entered.setdefault("scramble_below", []).append(np.where(step != 0, diff < 0, False))
                diff = np.minimum(0.0, diff)
            margin = np.minimum(margin, np.where(step != 0, gm, np.inf))
            stepped[:, k] = step != 0
            rows.append(np.where(step != 0, diff, 0.0)[:, None])
        self.entered["stepped"] = stepped
        # ---------- balance
        fall_time = np.sqrt(2 * hgoal / 9.81)
        cp = com + comvel * fall_time
        rows.append(cp[:, :2] - avg[:, :2])
        # ---------- effort
        rows.append(2e-2 * actuator_force(m, self.ref, q, v, ctrl, jac).numpy())
        # ---------- posture
        key = np.asarray(m["key_qpos"], float)
        nu = int(m["nu"])
        post = qn[:, 7:7 + nu] - key[k_home][7:7 + nu]
        if mode == MODE_FLIP:
            post = np.where((T < crouch_t)[:, None], qn[:, 7:7 + nu] - key[k_crouch][7:7 + nu], post)
            post = np.where(((T >= crouch_t) & (T < jump_t + flight))[:, None], 0.0, post)
        post = post * np.tile([2.0, 1.0, 1.0], 4)
        if mode == MODE_BIPED:
            post[:, [4, 5, 10, 11] if handstand else [1, 2, 7, 8]] *= 0.03
        rows.append(post)
        # ---------- yaw
        th = np.stack([R[:, 0, 0], R[:, 1, 0]], -1)
        if mode == MODE_BIPED:
            th = (1 if handstand else -1) * np.stack([R[:, 0, 2], R[:, 1, 2]], -1)
        th = normalize(th)
        hg = P[p_heading]
        rows.append(np.stack([th[:, 0] - np.cos(hg), th[:, 1] - np.sin(hg)], -1))
        # ---------- "angular momentum": a subtreelinvel sensor (task_flat.xml:143)
        rows.append(comvel)
        self.margin = margin
        return np.concatenate(rows, -1)

    # ------------------------------------------------------------------------------- humanoid tracking
    def _tracking(self, q, v, ctrl, time, jac, f):
        """tracking.cc:27-216.  int_data = [motion, first key of the motion, its length, 16 tracking sites, 16 mocap ids];
        dbl_data = [reference_time_]; the key frames' marker positions are the model's key_mpos"""
        m = self.m
        I = [int(x) for x in self.task["int_data"]]
        start, length, sites, mids = I[1], I[2], I[3:19], I[19:35]
        kmp = np.asarray(m["key_mpos"], float).reshape(-1, int(m["nmocap"]), 3)
        last = start + length - 1
        ci = (time - float(self.task["dbl_data"][0])) * 30.0 + start
        cl = np.clip(ci, 0.0, float(last))
        k0 = np.floor(cl).astype(int)
        k1 = np.minimum(k0 + 1, last)
        w1 = cl - k0
        w0 = 1.0 - w1
        # the key changes where the index crosses an integer inside the motion.  An index within 1e-9 ABOVE an integer in exact
        # arithmetic is safe: the one subtraction rounds alike everywhere, and the product and sum round monotonically, to that integer or above
        frac = np.abs(ci - np.round(ci))
        inside = (ci > -0.5) & (ci < last + 0.5)
        ref_time = float(self.task["dbl_data"][0])
        on_key = np.array([bool(fr < 1e-9 and Fraction(float(tm) - ref_time) * 30 + start >= int(round(c)))
                           for fr, tm, c in zip(frac, time, ci)])
        self.margin = np.where(inside & ~on_key, frac, np.inf)
        self.entered = dict(clamp_low=ci < 0, clamp_high=ci > last, k1_clamped=k0 + 1 > last, on_key=on_key & inside, k0=k0 - start)
        vn = v.numpy()
        mk = w0[:, None, None] * kmp[k0][:, mids] + w1[:, None, None] * kmp[k1][:, mids]     # [B, 16, 3]
        sp = f["site_xpos"][:, sites]
        sv = np.einsum("bsij,bj->bsi", jac["Sp"].numpy()[:, sites], vn)
        am, asp = mk.sum(1) * (1.0 / 16), sp.sum(1) * (1.0 / 16)
        pos = (mk - am[:, None]) - (sp - asp[:, None])
        vel = (kmp[k1][:, mids] - kmp[k0][:, mids]) * 30.0 - sv
        B = vn.shape[0]
        return np.concatenate([vn[:, 6:], ctrl, am - asp, pos.reshape(B, -1), vel.reshape(B, -1)], -1)

    # ------------------------------------------------------------------------------- humanoid walk
    def _walk(self, q, v, ctrl, time, jac, f):
        """walk.cc:44-165 with the sensors of walk/task.xml:69-86: framepos / framelinvel of a body are its inertial frame's, the
        up and forward axes are the xbody frame's z and x.  int_data = [torso, pelvis, foot_right, foot_left, waist_lower]"""
        torso, pelvis, fr, fl, waist = [int(x) for x in self.task["int_data"][:5]]
        P = np.asarray(self.task["parameters"], float)
        xipos, xmat = f["xipos"], f["xmat"]
        vn = v.numpy()
        com, comvel = self.ref.subtree(q, v, jac)
        com, comvel = com.numpy(), comvel.numpy()
        linvel = lambda b: np.einsum("bij,bj->bi", jac["Jp"].numpy()[:, b], vn)             # noqa: E731
        B = vn.shape[0]
        th = xipos[:, torso, 2]
        r_height = th - P[0]
        r_pelvis = 0.5 * (xipos[:, fl, 2] + xipos[:, fr, 2]) - xipos[:, pelvis, 2] - 0.2
        cp = com[:, torso] + 0.3 * comvel[:, torso]
        cp[:, 2] = 1e-3
        axis = xipos[:, fr] - xipos[:, fl]
        axis[:, 2] = 1e-3
        nrm = np.sqrt((axis * axis).sum(-1))
        axis = normalize(axis)
        length = 0.5 * nrm - 0.05
        centre = 0.5 * (xipos[:, fr] + xipos[:, fl])
        t = ((cp - centre) * axis).sum(-1)
        self.entered = dict(length_negative=length < 0, clamped=np.abs(t) > np.abs(length))
        t = np.maximum(-length, np.minimum(length, t))
        pcp = axis * t[:, None] + centre
        standing = th / np.sqrt(th * th + 0.45 * 0.45) - 0.4
        r_balance = standing[:, None] * (cp[:, :2] - pcp[:, :2])
        z = np.array([0.0, 0.0, 1.0])
        r_up = np.concatenate([(xmat[:, torso, 2, 2] - 1.0)[:, None], 0.3 * (xmat[:, pelvis, 2, 2] - 1.0)[:, None],
                               (0.1 * standing)[:, None] * (xmat[:, fr, :, 2] - z), (0.1 * standing)[:, None] * (xmat[:, fl, :, 2] - z)], -1)
        fwd = xmat[:, torso, :2, 0] + xmat[:, pelvis, :2, 0] + xmat[:, fr, :2, 0] + xmat[:, fl, :2, 0]
        self.entered["forward_guard"] = np.sqrt((fwd * fwd).sum(-1)) < MINVAL
        fwd = normalize(fwd)
        cv = 0.5 * (comvel[:, waist, :2] + linvel(torso)[:, :2])
        r_walk = standing * ((cv * fwd).sum(-1) - P[1])
        feet = cv - 0.5 * linvel(fr)[:, :2] - 0.5 * linvel(fl)[:, :2]
        return np.concatenate([r_height[:, None], r_pelvis[:, None], r_balance, r_up, q.numpy()[:, 7:], r_walk[:, None],
                               standing[:, None] * feet, ctrl], -1).reshape(B, -1)

    # ------------------------------------------------------------------------------- humanoid interact
    def _interact(self, q, v, ctrl, time, jac, f):
        """interact.cc:29-198 with the sensors of interact/task.xml:55-68: positions, torso_forward and "torso_subtreelinvel" (a
        framelinvel) are the bodies' inertial frames', the up axes the xbody frames'.  int_data = [torso, pelvis, foot_right, foot_left,
        head, shin_right, shin_left, facing target set, 5 x (body1, body2)]; dbl_data = [facing target xy, 5 x (local_pos1, local_pos2)]"""
        I = [int(x) for x in self.task["int_data"]]; D = np.asarray(self.task["dbl_data"], float); P = np.asarray(self.task["parameters"], float)
        torso, pelvis, fr, fl, head, kr, kl, facing = I[:8]
        xipos, ximat, xpos, xmat = f["xipos"], f["ximat"], f["xpos"], f["xmat"]
        vn = v.numpy()
        B = vn.shape[0]
        com, _ = self.ref.subtree(q, v, jac)
        rows = [np.abs(xmat[:, b, 2, 2] - 1.0)[:, None] for b in (torso, pelvis, fr, fl)]
        rows.append(np.abs(xipos[:, head, 2] - P[0])[:, None])
        rows.append(np.abs(xipos[:, torso, 2] - P[1])[:, None])
        foot_avg = 0.5 * (xipos[:, fl, :2] + xipos[:, fr, :2])
        knee = 0.5 * (xipos[:, kl, :2] + xipos[:, kr, :2]) - foot_avg
        rows.append(np.sqrt((knee * knee).sum(-1))[:, None])
        cf = com.numpy()[:, torso, :2] - foot_avg
        rows.append(np.sqrt((cf * cf).sum(-1))[:, None])
        if facing:
            tg = D[:2] - xipos[:, torso, :2]
            self.entered["facing_guard"] = np.sqrt((tg * tg).sum(-1)) < MINVAL
            tg = normalize(tg) - ximat[:, torso, :2, 0]
            rows.append(np.sqrt((tg * tg).sum(-1))[:, None])
        else:
            rows.append(np.zeros((B, 1)))
        self.entered["facing"] = np.full(B, bool(facing))
        rows.append(np.einsum("bij,bj->bi", jac["Jp"].numpy()[:, torso], vn)[:, :2])
        rows.append(vn[:, 6:])
        rows.append(ctrl)
        active = []
        for k in range(5):
            b1, b2 = I[8 + 2 * k], I[9 + 2 * k]
            if b1 != -1 and b2 != -1:
                p1, p2 = D[2 + 6 * k:5 + 6 * k], D[5 + 6 * k:8 + 6 * k]
                g1 = np.einsum("bij,j->bi", xmat[:, b1], p1) + xpos[:, b1]
                g2 = np.einsum("bij,j->bi", xmat[:, b2], p2) + xpos[:, b2]
                rows.append(np.abs(g1 - g2))
            else:
                rows.append(np.zeros((B, 3)))
            active.append(b1 != -1 and b2 != -1)
        self.entered["pairs_active"] = active
        return np.concatenate(rows, -1)

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

    def cost(self, residual, task=None):
        """CostValue (mjpc/task.cc:71-110): the weighted norms of mjpc/norm.cc:48-230, all nine types, then the exponential risk
        transform where |risk| >= 1e-6, spelt with expm1; `task` prices with another cost table over the same rows"""
        t = self.task if task is None else task
        r = np.asarray(residual, float)
        total = np.zeros(r.shape[:-1])
        start, pstart = 0, 0
        self.norms_entered = set()
        for k in range(int(t["num_term"])):
            n, norm, w = int(t["dim_norm_residual"][k]), int(t["norm"][k]), float(t["weight"][k])
            np_ = int(t["num_norm_parameter"][k])
            p, q_ = (list(t["norm_parameter"][pstart:pstart + np_]) + [0.0, 0.0])[:2]
            x = r[..., start:start + n]
            if norm == -1:                                 # null: the first entry
                y = x[..., 0]
            elif norm == 0:                                # quadratic
                y = 0.5 * (x * x).sum(-1)
            elif norm == 1:                                # L22: ((|x|^2)^(q/2) + p^q)^(1/q) - p
                y = ((x * x).sum(-1) ** (q_ / 2) + p ** q_) ** (1 / q_) - p
            elif norm == 2:                                # L2: sqrt(|x|^2 + p^2) - p
                y = np.sqrt((x * x).sum(-1) + p * p) - p
            elif norm == 3:                                # cosh: p^2 (cosh(x / p) - 1)
                y = (p * p * (np.cosh(x / p) - 1.0)).sum(-1)
            elif norm == 5:                                # power loss: |x|^p
                y = (np.abs(x) ** p).sum(-1)
            elif norm == 6:                                # smooth abs: sqrt(x^2 + p^2) - p
                y = (np.sqrt(x * x + p * p) - p).sum(-1)
            elif norm == 7:                                # smooth abs 2: (|x|^q + p^q)^(1/q) - p
                y = ((np.abs(x) ** q_ + p ** q_) ** (1 / q_) - p).sum(-1)
            elif norm == 8:                                # rectifier: p log(1 + exp(x / p)), or max(x, 0) at p = 0
                y = (p * np.log(1 + np.exp(x / p))).sum(-1) if p > 0 else np.maximum(x, 0.0).sum(-1)
            else:
                raise NotImplementedError(f"norm {norm}")
            self.norms_entered.add((norm, bool(p > 0)) if norm == 8 else norm)
            total = total + w * y
            start += n; pstart += np_
        risk = float(t["risk"])
        return total if abs(risk) < 1e-6 else np.expm1(risk * total) / risk
