"""Rollout cases for the per-step dynamics check of tests/dyn_ref.py (test infrastructure), shared by the CPU tier (oracle, kernel
source in emulation) and the GPU tier (HIP engine): the models with constraints switched off and fluid forces stripped, initial
states at the edges (quaternions far from identity, 10-20 rad/s on ball / free joints, hinges away from a non-zero qpos0), nominal
controls past ctrlrange (the planner clamps them onto the range, servos then saturate their force ranges) and the plan inputs."""
import numpy as np

from mujoco_mpc_amd.modelgen import REGISTRY
from mujoco_mpc_amd.modelgen.builder import BALL, FREE, HINGE, axisangle2quat, quat_mul

MJPC_DSBL_CONSTRAINT = 1

MODELS = ["particle", "cartpole", "acrobot", "walker", "quadruped", "humanoid_track", "shadow_hand", "ball_chain", "servo_arm",
          "filter_arm", "quadrotor"]


def _unit(rng, n=3):
    x = rng.normal(size=n)
    return x / np.linalg.norm(x)


def smooth(m):
    """the model with every constraint switched off (mjDSBL_CONSTRAINT) and no fluid forces"""
    m = dict(m)
    m["disableflags"] = int(m["disableflags"]) | MJPC_DSBL_CONSTRAINT
    m["density"] = 0.0; m["viscosity"] = 0.0; m["wind"] = np.zeros(3)
    return m


def edge_case(m, d, seed, spin=(10.0, 20.0), qpos0_shift=0.4):
    """(model, state): hinge joints measured from a shifted qpos0, ball / free quaternions rotated by 1-2.5 rad, ball / free angular
    speeds of 10-20 rad/s, hinge velocities of a few rad/s"""
    rng = np.random.default_rng(seed)
    m = dict(m); m["qpos0"] = np.array(m["qpos0"], float)
    nq, nv = m["nq"], m["nv"]
    s = np.array(d["state"], float)
    q, v = s[:nq], s[nq:nq + nv]
    for j in range(m["njnt"]):
        qa, da, t = m["jnt_qposadr"][j], m["jnt_dofadr"][j], m["jnt_type"][j]
        if t == FREE:
            q[qa + 3:qa + 7] = quat_mul(q[qa + 3:qa + 7], axisangle2quat(_unit(rng), rng.uniform(1.0, 2.5)))
            v[da:da + 3] += rng.normal(0, 1.0, 3)
            v[da + 3:da + 6] = _unit(rng) * rng.uniform(*spin)
        elif t == BALL:
            q[qa:qa + 4] = quat_mul(q[qa:qa + 4], axisangle2quat(_unit(rng), rng.uniform(1.0, 2.5)))
            v[da:da + 3] = _unit(rng) * rng.uniform(*spin)
        else:
            if t == HINGE and qpos0_shift:
                m["qpos0"][qa] += rng.uniform(-qpos0_shift, qpos0_shift)
            q[qa] += rng.uniform(-0.2, 0.2)
            v[da] += rng.normal(0, 2.0)
    return m, s


def plan_inputs(m, N, H, P=4, seed=0, sigma=0.4):
    """knot times / values (nominal values up to twice the control range: clamped onto its ends) and the seeded noise"""
    import oracle_lib as ol
    rng = np.random.default_rng(seed)
    lo, hi = m["actuator_ctrlrange"][:, 0], m["actuator_ctrlrange"][:, 1]
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    kv = mid + half * rng.uniform(-2.0, 2.0, (P, m["nu"]))
    kt = np.linspace(0, (H - 1) * m["timestep"], P)
    eps, sel = ol.noise(seed + 1, 0, 0, N, P, m["nu"])
    return dict(knot_times=kt, knot_values=kv, sigma=(sigma, 0.0), noise_eps=eps, noise_sel=sel)


def registry_case(name, seed=0):
    m, task, d = REGISTRY[name]()
    m, state = edge_case(smooth(m), d, seed)
    return m, task, state, (d["mocap"] if len(d["mocap"]) else None)


def random_case(seed, case_seed=0):
    from random_models import random_model
    m, task, d = random_model(seed)
    m, state = edge_case(smooth(m), d, case_seed)
    return m, task, state, None


def run_oracle(m, task, state, mocap, N, H, inp):
    import oracle_lib as ol
    return ol.Oracle(m, task).plan(state, mocap, 0.0, inp["knot_times"], inp["knot_values"], 2, N, H, sigma=inp["sigma"],
                                   noise_eps=inp["noise_eps"], noise_sel=inp["noise_sel"], nthreads=4)


def run_emu(m, task, state, mocap, N, H, inp):
    import emu_lib
    return emu_lib.plan(m, task, state, mocap, 0.0, inp["knot_times"], inp["knot_values"], 2, N, H, sigma=inp["sigma"],
                        noise_eps=inp["noise_eps"], noise_sel=inp["noise_sel"])


def mutate_mass(m, rel=1e-6):
    """the model with the mass and inertia of one mid-tree body (a body with a parent and a child that both move) changed by rel"""
    m = dict(m); nb = m["nbody"]; par = m["body_parentid"]
    moving = [b for b in range(1, nb) if m["body_dofnum"][m["body_weldid"][b]] > 0 and m["body_mass"][b] > 0]
    mid = [b for b in moving if par[b] in moving and any(par[c] == b for c in moving)]
    b = (mid or moving)[len(mid or moving) // 2]
    m["body_mass"] = np.array(m["body_mass"], float); m["body_inertia"] = np.array(m["body_inertia"], float)
    m["body_mass"][b] *= 1 + rel; m["body_inertia"][b] *= 1 + rel
    return m, b


def mutate_frame(m, angle=1e-6):
    """the model with the inertial frame (body_iquat) of the first body on a ball or free joint rotated by `angle` rad"""
    m = dict(m)
    b = next(m["jnt_bodyid"][j] for j in range(m["njnt"]) if m["jnt_type"][j] in (BALL, FREE) and m["body_mass"][m["jnt_bodyid"][j]] > 0)
    ine = m["body_inertia"][b]
    # an axis that really changes the world inertia: the one between the two most different principal moments
    ax = np.eye(3)[int(np.argmax([abs(ine[1] - ine[2]), abs(ine[0] - ine[2]), abs(ine[0] - ine[1])]))]
    m["body_iquat"] = np.array(m["body_iquat"], float)
    m["body_iquat"][b] = quat_mul(m["body_iquat"][b], axisangle2quat(ax, angle))
    return m, b
