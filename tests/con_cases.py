"""Rollout cases for the constrained per-step check of tests/con_ref.py (test infrastructure), shared by the CPU tier (oracle, kernel
source in emulation) and the GPU tier (HIP engine).  Every case keeps its constraints on, carries the solver tolerance TOLERANCE and
the default 100 iterations, has no noslip pass and no fluid forces, and names the row types it claims to exercise (`claims`); the
tests assert the coverage conditions against the reference's own census of the rows.

con_zoo (nv = 31, generic-nv kernels): free spheres and a free capsule on a plane with one sphere–sphere and one sphere–capsule
pair, in contact and moving tangentially (they slip first, then roll), a sphere that falls through its margin and gap zone, a
two-hinge arm with limits and friction loss, a fixed tendon with a limit and friction loss, a limited ball joint held by a connect,
a joint equality and a tendon equality (both polynomial).  Variants: `elliptic` (cone 1, impratio 3), `pyramidal` (cone 0,
impratio 1), both with condim 1 / 3 / 4 / 6, a margin and a gap, unequal solmix and priority, a non-default solimp and one
negative-solref geom; `plain` (cone 1, impratio 1, defaults, condim 3 everywhere)."""
import numpy as np

import dyn_cases as dc
from mujoco_mpc_amd.modelgen import REGISTRY, ModelBuilder
from mujoco_mpc_amd.modelgen.builder import BALL, CAPSULE, FREE, HINGE, PLANE, SPHERE, axisangle2quat, quat_mul
from mujoco_mpc_amd.modelgen.tasks import OBJ_SITE, TASK_COPYSTATE, make_task

# the solver tolerance of every case.  No sampled step ends at the 100-iteration cap with it; smaller values (1e-16, 1e-20, 0) do not
# lower the worst backward error and raise it on the pyramidal cases (figures: tests/test_constraint_reference.py)
TOLERANCE = 1e-12
ZOO_VARIANTS = ("elliptic", "pyramidal", "plain")
CASES = ["zoo_elliptic", "zoo_pyramidal", "zoo_plain", "quadruped_elliptic", "quadruped_pyramidal", "humanoid_track", "shadow_hand",
         "cartpole"]
NV = dict(zoo_elliptic=31, zoo_pyramidal=31, zoo_plain=31, quadruped_elliptic=18, quadruped_pyramidal=18, humanoid_track=27,
          shadow_hand=33, cartpole=2)


def tighten(m):
    m = dict(m)
    m["tolerance"] = TOLERANCE; m["iterations"] = 100; m["noslip_iterations"] = 0
    m["density"] = 0.0; m["viscosity"] = 0.0; m["wind"] = np.zeros(3)
    return m


def only_collidable(m, keep):
    """the model with contype / conaffinity cleared on every geom outside `keep`; the kept body geoms collide with the kept
    world geoms only (contype 0 / conaffinity 1 against contype 1 / conaffinity 0)"""
    m = dict(m)
    ct, ca = np.zeros(m["ngeom"], np.int32), np.zeros(m["ngeom"], np.int32)
    for g in keep:
        if m["geom_bodyid"][g] == 0:
            ct[g] = 1
        else:
            ca[g] = 1
    m["geom_contype"], m["geom_conaffinity"] = ct, ca
    return m


def con_zoo(variant):
    rich = variant != "plain"
    b = ModelBuilder(timestep=0.005, cone=0 if variant == "pyramidal" else 1, impratio=3.0 if variant == "elliptic" else 1.0,
                     tolerance=TOLERANCE, iterations=100)
    b.nconmax = 16; b.nefcmax = 96
    R = dict(rich=rich)

    def pick(rich_value, plain_value):
        return rich_value if R["rich"] else plain_value
    b.geom(0, "floor", PLANE, size=(5, 5, 0.1), condim=3, friction=(0.8, 0.01, 0.002), solmix=pick(2.0, 1.0),
           solimp=pick((0.85, 0.97, 0.004, 0.4, 3.0), (0.9, 0.95, 0.001, 0.5, 2.0)))
    sa = b.body("sa", 0, pos=(0, 0, 0.099)); b.joint(sa, "sa_free", FREE)
    b.geom(sa, "sa", SPHERE, size=(0.1,), mass=1.0, condim=pick(4, 3), friction=(1.0, 0.02, 0.001))
    sa_site = b.site(sa, "sa")
    sb = b.body("sb", 0, pos=(0.19, 0.02, 0.112)); b.joint(sb, "sb_free", FREE)
    b.geom(sb, "sb", SPHERE, size=(0.1,), mass=0.7, condim=3, friction=(0.5, 0.01, 0.001), margin=pick(0.01, 0.0), gap=pick(0.004, 0.0),
           solref=pick((-2000.0, -60.0), (0.02, 1.0)), solmix=pick(0.5, 1.0))
    cp = b.body("cap", 0, pos=(1.0, 0, 0.0495)); b.joint(cp, "cap_free", FREE)
    b.geom(cp, "cap", CAPSULE, size=(0.05, 0.2), zaxis=(0, 1, 0), mass=1.5, condim=pick(6, 3), friction=(0.6, 0.03, 0.004))
    cp_site = b.site(cp, "cap")
    sd = b.body("sd", 0, pos=(1.125, 0.05, 0.0795)); b.joint(sd, "sd_free", FREE)
    b.geom(sd, "sd", SPHERE, size=(0.08,), mass=0.4, condim=pick(1, 3), priority=pick(1, 0), friction=(0.9, 0.01, 0.001))
    off = dict(contype=0, conaffinity=0)
    a1 = b.body("a1", 0, pos=(-1, 0, 1.0))
    b.joint(a1, "a1_j", HINGE, axis=(0, 1, 0), limited=True, range=(-0.5, 0.5), frictionloss=0.3, margin=pick(0.02, 0.0), damping=0.05, armature=0.01)
    b.geom(a1, "a1", CAPSULE, size=(0.03, 0), fromto=(0, 0, 0, 0, 0, -0.3), mass=0.5, **off)
    a2 = b.body("a2", a1, pos=(0, 0, -0.3))
    b.joint(a2, "a2_j", HINGE, axis=(0, 1, 0), limited=True, range=(-0.8, 0.3), frictionloss=0.1, damping=0.02, armature=0.01,
            solreflimit=pick((0.03, 0.8), (0.02, 1.0)))
    b.geom(a2, "a2", CAPSULE, size=(0.025, 0), fromto=(0, 0, 0, 0, 0, -0.25), mass=0.3, **off)
    b.tendon("t_arm", ["a1_j", "a2_j"], [1.0, -0.7], limited=True, range=(-1.0, 1.0), margin=pick(0.01, 0.0), frictionloss=0.15)
    for k, x in ((1, -1.5), (2, -2.0)):
        f = b.body(f"f{k}", 0, pos=(x, 0, 1.0))
        b.joint(f, f"f{k}_j", HINGE, axis=(1, 0, 0), damping=0.02, armature=0.005)
        b.geom(f, f"f{k}", CAPSULE, size=(0.02, 0), fromto=(0, 0, 0, 0, 0.05, -0.2), mass=0.2, **off)
    b.tendon("t_f", ["f1_j"], [1.3])
    b.tendon_equality("t_f", "t_arm", polycoef=(0.0, 0.8, 0.3, 0, 0))
    b.joint_equality("f2_j", "a2_j", polycoef=(0.05, -1.2, 0.4, 0.1, 0), solref=pick((0.03, 0.9), (0.02, 1.0)))
    p = b.body("pend", 0, pos=(-2.5, 0, 1.0))
    b.joint(p, "pend_j", BALL, limited=True, range=(0, 0.6), damping=0.02)
    b.geom(p, "pend", CAPSULE, size=(0.03, 0), fromto=(0, 0, 0, 0, 0, -0.4), mass=0.8, **off)
    b.connect(p, 0, (0, 0, -0.4), solref=(0.08, 1.0), solimp=pick((0.8, 0.95, 0.05, 0.3, 2.5), (0.9, 0.95, 0.001, 0.5, 2.0)))
    b.actuator("a1_m", "a1_j", gear=3.0, ctrlrange=(-1, 1), biastype=1, biasprm=(0, 0, -0.1))      # a velocity term: implicitfast differs from Euler
    b.actuator("a2_m", "a2_j", gear=2.0, ctrlrange=(-1, 1))
    b.actuator("sa_push", site=sa_site, gear6=(2.0, 0.5, 0, 0, 0, 0), ctrlrange=(-1, 1))
    b.actuator("cap_push", site=cp_site, gear6=(0, 1.5, 0, 0, 0, 0.2), ctrlrange=(-1, 1))
    m = b.compile()
    task = make_task(TASK_COPYSTATE, [(m["nq"], 0, 1.0), (m["nv"], 0, 0.1)], traces=[(OBJ_SITE, sa_site)])
    q = np.array(m["qpos0"], float); v = np.zeros(m["nv"])
    J = m["names"]["joint"]

    def qa(n):
        return int(m["jnt_qposadr"][J[n]])

    def da(n):
        return int(m["jnt_dofadr"][J[n]])
    v[da("sa_free"):da("sa_free") + 3] = [1.0, 0.1, 0.0]                        # sliding into sb; no spin: slips, then rolls
    v[da("sb_free"):da("sb_free") + 3] = [0.0, 0.0, -0.6]                       # falls through its margin and gap zone
    v[da("cap_free"):da("cap_free") + 6] = [0.6, 0.2, 0.0, 0.0, 0.0, 2.0]       # slides across its axis and spins on the floor
    v[da("sd_free"):da("sd_free") + 3] = [-0.3, 0.0, 0.0]
    q[qa("a1_j")] = 0.49; v[da("a1_j")] = 3.0               # onto its upper limit; the tendon (1.04 at the start) is past its own
    q[qa("a2_j")] = -0.78; v[da("a2_j")] = -2.0
    q[qa("f1_j")] = 0.1; v[da("f1_j")] = 1.0
    q[qa("f2_j")] = -0.15; v[da("f2_j")] = -1.0
    ax = np.array([1.0, 0.3, 0.0]); ax /= np.linalg.norm(ax)
    q[qa("pend_j"):qa("pend_j") + 4] = quat_mul(q[qa("pend_j"):qa("pend_j") + 4], axisangle2quat(ax, 0.7))      # beyond its 0.6 rad limit
    v[da("pend_j"):da("pend_j") + 3] = [2.0, -1.0, 0.5]
    return m, task, np.concatenate([q, v])


def _low_humanoid(m, state, depth=0.004):
    """the state with the root lowered until the lowest kept geom is `depth` inside the floor"""
    from dyn_ref import DynRef, _t, qmat
    s = np.array(state, float)
    f = DynRef(m).fk(_t(s[None, :m["nq"]]))
    low = np.inf
    for g in range(m["ngeom"]):
        if m["geom_conaffinity"][g] == 0:
            continue
        bb = int(m["geom_bodyid"][g])
        c = f["xpos"][0, bb].numpy() + f["xmat"][0, bb].numpy() @ m["geom_pos"][g]
        ax = f["xmat"][0, bb].numpy() @ qmat(_t(m["geom_quat"][g])).numpy()[:, 2]
        half = m["geom_size"][g][1] if m["geom_type"][g] == CAPSULE else 0.0
        low = min(low, c[2] - abs(ax[2]) * half - m["geom_size"][g][0])
    s[2] -= low + depth
    return s


def case(name):
    """(model, task, state, mocap, claims): claims = the row types (con_ref.ROW_TYPES) that must appear in at least 5 checked pairs"""
    if name.startswith("zoo_"):
        m, task, state = con_zoo(name[4:])
        return tighten(m), task, state, None, ("equality", "friction_dof", "friction_tendon", "limit_joint", "limit_ball", "limit_tendon", "contact")
    if name.startswith("quadruped"):
        m, task, d = REGISTRY["quadruped"]()
        keep = [g for g in range(m["ngeom"]) if g == m["names"]["geom"]["floor"] or g in [m["names"]["geom"][f] for f in ("FR", "FL", "HR", "HL")]]
        m = only_collidable(tighten(m), keep)
        if name.endswith("pyramidal"):
            m["cone"] = 0
        return m, task, np.array(d["state"], float), d["mocap"], ("friction_dof", "contact")
    if name == "humanoid_track":
        m, task, d = REGISTRY["humanoid_track"]()
        keep = [g for g in range(m["ngeom"]) if m["geom_type"][g] in (PLANE, SPHERE, CAPSULE)]
        m = only_collidable(tighten(m), keep)
        return m, task, _low_humanoid(m, d["state"]), d["mocap"], ("limit_joint", "contact")
    if name == "shadow_hand":
        m, task, d = REGISTRY["shadow_hand"]()
        m = tighten(m); m["disableflags"] = int(m["disableflags"]) | (1 << 4)
        _, state = dc.edge_case(m, d, 0, qpos0_shift=0.0)
        return m, task, state, (d["mocap"] if len(d["mocap"]) else None), ("friction_dof", "limit_joint")
    if name == "cartpole":
        m, task, d = REGISTRY["cartpole"]()
        return tighten(m), task, np.array([1.79, 0.3, 3.0, -1.0]), None, ("limit_joint",)
    raise KeyError(name)


def inputs(name, m, N, H):
    """the plan inputs of a case: dyn_cases.plan_inputs (nominal controls up to twice the control range, clamped onto its ends);
    the quadruped gets a fifth of that and less noise, so that its feet also hold on the floor instead of only thrashing over it;
    the cartpole's motor presses the cart onto its slider limit"""
    inp = dc.plan_inputs(m, N, H, sigma=0.1 if name.startswith("quadruped") else 0.4)
    if name.startswith("quadruped"):
        inp["knot_values"] = 0.2 * inp["knot_values"]
    if name == "cartpole":
        inp["knot_values"] = np.abs(inp["knot_values"]) + 1.0        # every nominal control beyond the range's upper end: the motor presses the cart onto its upper limit
    return inp


def sample_pairs(N, H, npairs=120, nfull=8, seed=0):
    """a fixed seeded sample of npairs (candidate, step) pairs plus every step of nfull candidates (for the count check)"""
    rng = np.random.default_rng(seed)
    k = rng.choice(N * (H - 1), npairs, replace=False)
    full = rng.choice(N, nfull, replace=False)
    cc_, tt = np.meshgrid(full, np.arange(H - 1), indexing="ij")
    k = np.unique(np.concatenate([k, cc_.ravel() * (H - 1) + tt.ravel()]))
    return k // (H - 1), k % (H - 1)


def contact_case(name):
    return name.startswith(("zoo_", "quadruped")) or name == "humanoid_track"


def coverage(res, claims, contact):
    """the coverage conditions of a checked case against the reference's own census; returns what was seen"""
    n = len(res["err"])
    seen = {k: sum(1 for c in res["census"] if c[k] > 0) for k in claims}
    slip = sum(1 for z in res["zones"] if "slip" in z); stick = sum(1 for z in res["zones"] if "stick" in z)
    assert 2 * int((res["active"] > 0).sum()) >= n, f"only {(res['active'] > 0).sum()} of {n} pairs have an active row"
    for k, c in seen.items():
        assert c >= 5, f"row type {k} appears in {c} checked pairs"
    if contact:
        assert slip >= 1 and stick >= 1, f"slipping pairs {slip}, sticking pairs {stick}"
    return dict(seen, slip=slip, stick=stick, active=int((res["active"] > 0).sum()), pairs=n)
