"""Every rollout step's smooth dynamics against an independent float64 reference (tests/dyn_ref.py: Kane's equations with autodiff
for the velocity-product terms; no RNE, no CRBA, nothing from oracle/ or csrc/), on the CPU producers: the oracle and the kernel
source in emulation.

A step t → t+1 of a rollout without constraints must satisfy the equations of motion at state t.  The check is a backward error in
force space, ‖A_ref a − f_ref‖∞ / (‖A_ref a‖∞ + ‖f_ref‖∞) with a = (qvel_{t+1} − qvel_t) / h, so it is independent of how well
conditioned M is and of the horizon: it is checked at every step of every candidate to round-off.

BAR: 10× the worst value observed on these producers, rounded up.  Observed worst (oracle and emulation, every case below):
2.0e-14 (filter_arm under implicit), so BAR = 2e-13; the integration (integratePos, activation update) agrees to 7e-16.
"""
import numpy as np
import pytest
import torch

import dyn_cases as dc
from dyn_ref import DynRef, _t, check_steps

BAR = 2e-13
N, H = 3, 25
# the integrators of test_implicit_integrators_kernel_source_matches_oracle: Euler, implicitfast, implicit
INTEGRATORS = (0, 3, 2)
# random_models seeds with nv outside the compile-time nv {2, 18, 27, 33}: several free bodies each, nv from 21 to 40 (seed 4),
# implicitfast (2, 12), activation states (1, 4, 12, 14, 16), joint-level force clamps, gravity compensation, fixed tendons
RANDOM_SEEDS = (0, 1, 2, 4, 7, 12, 14, 16)


# the one case the engine refuses: implicitfast with ball_chain's damped tendon across two branches (outside the factorisation pattern)
EMU_REFUSED = {("ball_chain", 3)}


def _producers(m, task, state, mocap, inp, refused=False):
    """(name, rollout) of the oracle and the kernel source; refused=True: the kernel source must refuse the model, and only the
    oracle's rollout is checked"""
    out = [("oracle", dc.run_oracle(m, task, state, mocap, N, H, inp))]
    if refused:
        with pytest.raises(AssertionError):
            dc.run_emu(m, task, state, mocap, N, H, inp)
    else:
        out.append(("emu", dc.run_emu(m, task, state, mocap, N, H, inp)))
    return out


def _check(m, runs, bar=BAR):
    """one reference evaluation for every producer's steps; each producer's rollout is checked on its own"""
    ref = DynRef(m)
    res = {}
    for name, out in runs:
        assert not out["failure"].any(), name
        if "diag" in out:
            assert (out["diag"][:, 2] == 0).all(), "a constraint row existed"
        res[name] = check_steps(m, out["states"], out["actions"], m["timestep"], m["integrator"], bar, ref=ref)
    return res


# implicit (the slowest reference: ∂c/∂v by nested forward-mode autodiff) here on the models up to 8 dofs (hinges, a free body with
# site actuators, ball joints, activations); walker (9 dofs), quadruped (18), humanoid_track (27) and shadow_hand (33) run it on the
# GPU tier, in every kernel flavour, next to Euler and implicitfast
CASES = [(n, i) for n in dc.MODELS for i in INTEGRATORS if not (i == 2 and n in ("walker", "quadruped", "humanoid_track", "shadow_hand"))]


@pytest.mark.parametrize("name, integrator", CASES)
def test_registry_models_every_step_satisfies_the_reference_dynamics(name, integrator):
    """Also pins the known open point of ADVICE item 1: ball_chain's damped tendon across two branches keeps its non-ancestor
    entries in M − h ∂F/∂v under implicit, which is the exact derivative the reference takes (whether MuJoCo 3.1.4's sparse
    qDeriv drops them cannot be checked here)."""
    m, task, state, mocap = dc.registry_case(name)
    m["integrator"] = integrator
    runs = _producers(m, task, state, mocap, dc.plan_inputs(m, N, H), refused=(name, integrator) in EMU_REFUSED)
    res = _check(m, runs)
    assert len(res) == 2 - ((name, integrator) in EMU_REFUSED)


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_models_every_step_satisfies_the_reference_dynamics(seed):
    m, task, state, mocap = dc.random_case(seed)
    assert m["nv"] not in (2, 18, 27, 33)
    assert sum(1 for t in m["jnt_type"] if t == 0) >= 2              # more than one free body
    runs = _producers(m, task, state, mocap, dc.plan_inputs(m, N, H))
    _check(m, runs)


def test_random_models_reach_forty_dofs_and_every_force_kind():
    """the seeds above cover what the check is for: nv >= 40, activation states, joint-level clamps, gravity compensation, tendons"""
    from random_models import random_model
    ms = [random_model(s)[0] for s in RANDOM_SEEDS]
    assert max(m["nv"] for m in ms) >= 40
    assert any(m["na"] for m in ms) and any(m["jnt_actfrclimited"].any() for m in ms) and any((m["body_gravcomp"] > 0).any() for m in ms)
    assert any(m["ntendon"] for m in ms) and any(m["integrator"] == 3 for m in ms)


def test_rollouts_reach_the_edges():
    """the initial states and controls drive the check where kernels go wrong: quaternions far from identity, 10-20 rad/s on
    ball / free joints, hinges away from a non-zero qpos0, controls on the ends of ctrlrange, forces saturating forcerange and
    jnt_actfrcrange"""
    m, task, state, mocap = dc.registry_case("ball_chain")
    nq = m["nq"]
    quats = [state[m["jnt_qposadr"][j]:m["jnt_qposadr"][j] + 4] for j in range(m["njnt"]) if m["jnt_type"][j] == 1]
    assert quats and min(abs(q[0]) for q in quats) < np.cos(0.5)
    assert np.abs(state[nq:]).max() >= 10
    m, task, state, mocap = dc.registry_case("servo_arm")
    nq = m["nq"]
    assert np.abs(m["qpos0"]).max() > 0
    out = dc.run_oracle(m, task, state, mocap, N, H, dc.plan_inputs(m, N, H))
    lo, hi = m["actuator_ctrlrange"][:, 0], m["actuator_ctrlrange"][:, 1]
    acts = out["actions"][:, :-1]
    assert ((acts == lo) | (acts == hi)).any()
    ref = DynRef(m)
    S = out["states"][:, :-1].reshape(-1, out["states"].shape[-1]); U = acts.reshape(-1, m["nu"])
    q, v = _t(S[:, :nq]), _t(S[:, nq:nq + m["nv"]])
    jac = ref.jacobians(q)
    mom = ref.actuator_moments(jac)
    u = ref.clamped_ctrl(_t(U))
    f = (u * _t(m["actuator_gainprm"][:, 0]) + _t(m["actuator_biasprm"][:, 1]) * ref.actuator_lengths(q)
         + _t(m["actuator_biasprm"][:, 2]) * (mom @ v.unsqueeze(-1)).squeeze(-1))
    assert (f[:, 1].abs() > 1.0).any()                                         # s1 beyond its forcerange (-1, 1)
    unclamped = (mom.transpose(-1, -2) @ f.unsqueeze(-1)).squeeze(-1)
    assert (unclamped[:, 0].abs() > 1.2).any()                                 # j0's total beyond its jnt_actfrcrange


# ------------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("name", ["quadruped", "humanoid_track", "shadow_hand", "ball_chain", "quadrotor"])
def test_reference_mass_matrix_and_kinematics_match_modelgen(name):
    from mujoco_mpc_amd.modelgen import kinematics, mass_matrix
    m, task, state, mocap = dc.registry_case(name, seed=3)
    ref = DynRef(m)
    q = state[:m["nq"]]
    f = ref.fk(_t(q[None]))
    xpos, xquat, xmat, _, _ = kinematics(m, q)
    assert np.abs(f["xpos"][0].numpy() - xpos).max() < 1e-14 and np.abs(f["xmat"][0].numpy() - xmat).max() < 1e-14
    M = ref.mass_matrix(_t(q[None]))[0].numpy()
    Mm = mass_matrix(m, q)[0]
    assert np.abs(M - Mm).max() < 1e-13 * max(1.0, np.abs(Mm).max())


@pytest.mark.parametrize("name", ["particle", "quadruped", "humanoid_track", "shadow_hand"])
def test_reference_subtree_frames_match_the_oracle(name):
    """subtree_com / subtree_linvel (what the GPU tier compares mjpc_hip_get_frame against) equal the oracle's at an edge state,
    world row and massless subtrees (com = xipos) included; mocap bodies left out (the reference does not see their poses)"""
    import oracle_lib as ol
    m, task, state, mocap = dc.registry_case(name, seed=2)
    nq, nv = m["nq"], m["nv"]
    r = ol.Oracle(m, task).forward(state[:nq], state[nq:nq + nv], mocap=mocap)
    com, lin = DynRef(m).subtree(_t(state[None, :nq]), _t(state[None, nq:nq + nv]))
    b = np.asarray(m["body_mocapid"]) < 0
    assert np.abs(r["subtree_com"][b] - com[0].numpy()[b]).max() < 1e-13 * max(1.0, np.abs(r["subtree_com"]).max())
    assert np.abs(r["subtree_linvel"][b] - lin[0].numpy()[b]).max() < 1e-13 * max(1.0, np.abs(r["subtree_linvel"]).max())


def test_reference_cartpole_bias_is_the_textbook_form():
    """c = (−m_p l sin θ θ̇², −m_p g l sin θ) (test_cartpole_equations_of_motion_textbook's form), M = [[m_c + m_p, m_p l cos θ],
    [m_p l cos θ, I_hinge]]"""
    from mujoco_mpc_amd.modelgen import cartpole, mass_matrix
    m, _, _ = cartpole()
    ref = DynRef(m)
    mp, mc, l, g = 0.1, 1.0, 0.5, 9.81
    I_hinge = mass_matrix(m, np.zeros(2))[0][1, 1]
    for th, xd, thd in [(0.3, 0.1, -0.5), (2.5, -0.3, 1.2), (-1.0, 0.0, 0.0), (1.3, 2.0, 7.0)]:
        q, v = _t([[0.2, th]]), _t([[xd, thd]])
        c = ref.bias(q, v)[0].numpy()
        assert np.allclose(c, [-mp * l * np.sin(th) * thd ** 2, -mp * g * l * np.sin(th)], rtol=0, atol=1e-13)
        assert np.allclose(ref.mass_matrix(q)[0].numpy(), [[mc + mp, mp * l * np.cos(th)], [mp * l * np.cos(th), I_hinge]], rtol=0, atol=1e-13)


def test_reference_power_identity_on_a_free_chain():
    """Along the motion a = M⁻¹(τ − c) the kinetic energy T(q, v) = ½ vᵀ M(q) v changes at dT/dt = ∂T/∂s + vᵀ M a, where
    ∂T/∂s = d/ds T(q(s), v) at s = 0 along q(s) = integratePos(q, v, s) (autodiff).  Physically dT/dt = vᵀ τ − dV/dt with the
    gravity potential V = −Σ m g·xipos, dV/dt = vᵀ c(q, 0).  Hence, for every v:

        d/ds T(q(s), v) = vᵀ (c(q, v) − c(q, 0))

    (the velocity-product part of c does no work), checked on a free-floating chain of ball joints at 10-20 rad/s."""
    from torch.func import jvp
    from mujoco_mpc_amd.modelgen import ModelBuilder
    from mujoco_mpc_amd.modelgen.builder import BALL, CAPSULE, FREE
    b = ModelBuilder(contact=False, gravity=(0.3, -1.0, -9.81))
    parent = b.body("root", 0, pos=(0, 0, 1), quat=(0.9, 0.1, -0.3, 0.2))
    b.joint(parent, "free", FREE)
    b.geom(parent, "g0", CAPSULE, size=(0.05, 0.1), pos=(0.03, 0.01, 0), quat=(0.8, 0.2, 0.1, -0.3), mass=1.0)
    for k in range(4):
        parent = b.body(f"l{k}", parent, pos=(0.2, 0.05 * k, 0), quat=(0.9, 0.3 * k, 0.1, 0.2))
        b.joint(parent, f"ball{k}", BALL, pos=(-0.05, 0, 0), armature=0.01)
        b.geom(parent, f"g{k + 1}", CAPSULE, size=(0.04, 0.08), pos=(0.04, -0.02, 0.01), quat=(0.7, 0.1, 0.5, -0.2), mass=0.5 + 0.1 * k)
    m = b.compile()
    m, s = dc.edge_case(m, dict(state=np.concatenate([m["qpos0"], np.zeros(m["nv"])])), 7)
    ref = DynRef(m)
    q, v = _t(s[None, :m["nq"]]), _t(s[None, m["nq"]:])

    def T(sv):
        qq = ref.integrate_pos(q, v, sv)
        return 0.5 * (v.unsqueeze(-2) @ ref.mass_matrix(qq) @ v.unsqueeze(-1)).squeeze()
    dT = jvp(T, (torch.zeros((), dtype=torch.float64),), (torch.ones((), dtype=torch.float64),))[1]
    work = (v * (ref.bias(q, v) - ref.bias(q, torch.zeros_like(v)))).sum()
    assert abs(float(dT)) > 1.0
    assert abs(float(dT - work)) < 1e-12 * abs(float(dT))


@pytest.mark.parametrize("seed", (1, 4, 14))
def test_reference_actuation_matches_the_oracle_beyond_the_ranges(seed):
    """actuator generalized forces with controls beyond ctrlrange, forces past forcerange and the joint-level jnt_actfrcrange clamp
    (the planner clamps its controls, so the rollouts never hand such a control to the physics)"""
    import oracle_lib as ol
    m, task, state, _ = dc.random_case(seed)
    o = ol.Oracle(m, task)
    rng = np.random.default_rng(seed)
    nq, nv, na = m["nq"], m["nv"], m["na"]
    m0 = dict(m); m0["dof_damping"] = np.zeros(nv); m0["jnt_stiffness"] = np.zeros(m["njnt"]); m0["body_gravcomp"] = np.zeros(m["nbody"])
    m0["tendon_stiffness"] = np.zeros(m["ntendon"]); m0["tendon_damping"] = np.zeros(m["ntendon"])
    ref = DynRef(m0)                  # the actuator forces alone: every passive force switched off
    for k in range(4):
        ctrl = rng.uniform(-4, 4, m["nu"])
        act = rng.uniform(-0.5, 0.5, na)
        q, v = state[:nq], state[nq:nq + nv] * (k + 1)
        _, qfrc = o.actuation(q, v, ctrl, act if na else None)
        jac = ref.jacobians(_t(q[None]))
        tau = ref.force(_t(q[None]), _t(v[None]), _t(act[None]), _t(ctrl[None]), jac)[0].numpy()
        assert np.abs(tau - qfrc).max() < 1e-12 * max(1.0, np.abs(qfrc).max())


# ------------------------------------------------------------------------------------------------------ negative controls
@pytest.mark.parametrize("producer", ["oracle", "emu"])
def test_negative_controls_flag_a_wrong_mass_or_inertial_frame(producer):
    """the engine steps a model whose mid-tree body mass / inertia is off by 1e-6 relative, or whose inertial frame on a free or
    ball joint is turned by 1e-6 rad, the reference keeps the true model: the check must exceed the bar by 100× or more.
    Observed on humanoid_track: mass 1.0e-7 (5.1e5× the bar), frame 1.3e-9 (6.6e3×), the same on both producers."""
    run = dc.run_oracle if producer == "oracle" else dc.run_emu
    m, task, state, mocap = dc.registry_case("humanoid_track")
    inp = dc.plan_inputs(m, N, H)
    ref = DynRef(m)
    for mutate in (dc.mutate_mass, dc.mutate_frame):
        bad, body = mutate(m)
        out = run(bad, task, state, mocap, N, H, inp)
        res = check_steps(m, out["states"], out["actions"], m["timestep"], m["integrator"], None, ref=ref)
        assert res["worst"] >= 100 * BAR, (mutate.__name__, body, res["worst"])


def test_joint_level_clamp_keeps_the_velocity_gain_in_the_implicit_step():
    """Pins today's convention: under implicitfast / implicit an actuator's velocity gain (affine bias2) stays in
    M − h ∂F/∂v while jnt_actfrcrange clamps its joint's total actuator force; it drops out only while the actuator's own force sits
    on its forcerange.  The exact derivative of the clamped force is zero there; servo_arm (joint j0: kv = 1.5, clamp ±1.2) shows
    the two conventions apart.  Whether MuJoCo 3.1.4's mjd_actuator_vel looks at the joint-level clamp cannot be checked here."""
    m, task, state, mocap = dc.registry_case("servo_arm")
    out = dc.run_oracle(m, task, state, mocap, N, H, dc.plan_inputs(m, N, H))
    today = check_steps(m, out["states"], out["actions"], m["timestep"], 3, BAR)
    exact = check_steps(m, out["states"], out["actions"], m["timestep"], 3, None, actfrc_in_derivative=True)
    assert today["worst"] < BAR and exact["worst"] > 1e-3
