"""Every constrained rollout step against an independent float64 statement of MuJoCo's soft-constraint model (tests/con_ref.py: the
rows from the model dict, the force law in its dual form; nothing from oracle/ or csrc/, nothing solved or iterated), on the CPU
producers: the oracle and the kernel source in emulation.

A step t → t+1 must satisfy qfrc_c = Jᵀ F(J a_s − aref) at state t, with qfrc_c = A a_int − f_smooth what the constraints
contributed.  The check is the backward error ‖qfrc_c − JᵀF‖∞ / (‖qfrc_c‖∞ + ‖JᵀF‖∞ + ‖f_smooth‖∞), at every step of every candidate.

Solver settings of the cases (con_cases.TOLERANCE): tolerance 1e-12, 100 iterations.  No sampled step ends at the iteration cap
(4 to 6 Newton iterations per step).  What bounds the error is the stopping rule itself: the solve ends when the cost stops
decreasing (improvement < tolerance), and in double precision a cost decrease is lost in round-off once the gradient is near
√ε of the forces.  Smaller tolerances do not help: at 1e-16, 1e-20 and 0 the elliptic worst stays where it is, and the cases
with a piecewise quadratic cost get worse (1e-20: zoo_pyramidal 1.3e-6, cartpole 1.1e-7, after a last step into round-off).

BAR: 10× the worst value observed on these producers (the margin of the smooth-dynamics bar), rounded up.  The worst is reached by
the elliptic cones, whose cost is not piecewise quadratic (Newton's last step is not exact): quadruped_elliptic (impratio 10,
condim 6) 9.04e-5 on the oracle, 6.66e-5 in emulation; zoo_plain 1.84e-6 (implicit, emulation), zoo_elliptic 1.18e-6.  So
BAR = 1e-3.
BAR_QUADRATIC: the same rule over the cases whose cost is piecewise quadratic (pyramidal cones, frictionless contacts, limits,
friction loss, equalities), asserted on those cases in place of the looser BAR: cartpole 2.08e-8 (oracle; 7.3e-15 in emulation),
quadruped_pyramidal 6.7e-12, humanoid_track 7.7e-13, zoo_pyramidal 2.4e-13 (implicit), shadow_hand 4.2e-15.  So
BAR_QUADRATIC = 3e-7.  Integration (integratePos, activation update) agrees to 1e-15.

Negative controls, the stepped model wrong and the reference's right, each against the bar of the case it runs on (which it must
exceed 100×); observed worst, the same on the oracle and in emulation, as a multiple of that bar (and of BAR):
    zoo_pyramidal  floor solimp[0] + 1e-3                3.69e-3   12 295×  (3.7× BAR)
    zoo_pyramidal  floor sliding friction + 1e-3         1.86e-3    6 194×  (1.9× BAR)
    zoo_pyramidal  sb's solmix swapped for the floor's   1.25e-1  416 513×  (125× BAR)
    zoo_pyramidal  iterations = 1                        9.97e-1  3.3e6×    (997× BAR)
    zoo_elliptic   impratio 1 instead of 3               2.53e-1      252×  (its bar is BAR)
The two 1e-3 perturbations stay below 100× BAR: a wrong constant of that size is only visible at the quadratic bar, which is
why the piecewise quadratic cases are not judged at the elliptic cones' level.
"""
import numpy as np
import pytest

import con_cases as cc
import dyn_cases as dc
from con_ref import ConRef, check_constrained_steps, cone_force, elliptic_R, impedance, invweights

BAR = 1e-3
BAR_QUADRATIC = 3e-7
N, H = 3, 25
INTEGRATORS = (0, 3)          # Euler, implicitfast; con_zoo also under implicit (2)
CASES = [(n, i) for n in cc.CASES for i in INTEGRATORS] + [(n, 2) for n in cc.CASES if n.startswith("zoo_")]


def bar_of(m):
    """the bar of a model's solves: BAR where a contact can carry an elliptic cone with friction, else BAR_QUADRATIC"""
    contacts = not (int(m["disableflags"]) & (1 | 16)) and bool(np.any(m["geom_contype"]) or np.any(m["geom_conaffinity"]))
    return BAR if contacts and int(m["cone"]) == 1 and int(np.max(m["geom_condim"])) > 1 else BAR_QUADRATIC


def _runs(m, task, state, mocap, inp, producers=("oracle", "emu")):
    return [(p, (dc.run_oracle if p == "oracle" else dc.run_emu)(m, task, state, mocap, N, H, inp)) for p in producers]


@pytest.mark.parametrize("name, integrator", CASES)
def test_every_constrained_step_satisfies_the_reference_force_law(name, integrator):
    """oracle and emulation; the emulation's diagnostics (most contacts / rows of a state) must equal the reference's census, and the
    coverage conditions of the case hold on the reference's own census: at least half of the pairs have an active row, every
    claimed row type appears in 5 pairs or more, a contact case has slipping and sticking pairs"""
    m, task, state, mocap, claims = cc.case(name)
    assert m["nv"] == cc.NV[name] and m["tolerance"] == cc.TOLERANCE and m["iterations"] == 100 and m["noslip_iterations"] == 0
    m["integrator"] = integrator
    ref = ConRef(m)
    for p, out in _runs(m, task, state, mocap, cc.inputs(name, m, N, H)):
        assert not out["failure"].any(), p
        res = check_constrained_steps(m, out["states"], out["actions"], m["timestep"], integrator, None, diag=out.get("diag"), ref=ref)
        cov = cc.coverage(res, claims, cc.contact_case(name))
        print(f"\n[constraint-reference] {name} integrator={integrator} {p} worst={res['worst']:.3e} pos={res['pos']:.1e} act={res['act']:.1e} "
              f"rows<={res['rows'].max()} contacts<={res['contacts'].max()} {cov}")
        assert res["worst"] <= bar_of(m), (p, res["worst"])
        assert res["pos"] <= 1e-14 and res["act"] <= 1e-14, (p, res["pos"], res["act"])
        assert len(res["err"]) == N * (H - 1)                       # no step left out


def test_zoo_variants_cover_the_parameter_space():
    """cone 0 and 1, condim 1 / 3 / 4 / 6, impratio 1 and 3, a margin and a gap, unequal solmix and priority, a non-default solimp,
    one negative-solref geom; generic nv"""
    ms = [cc.case("zoo_" + v)[0] for v in cc.ZOO_VARIANTS]
    assert {int(m["cone"]) for m in ms} == {0, 1} and {float(m["impratio"]) for m in ms} == {1.0, 3.0}
    for m in ms[:2]:
        assert m["nv"] not in (2, 18, 27, 33)
        assert {1, 3, 4, 6} <= set(int(x) for x in m["geom_condim"])
        assert (m["geom_margin"] > 0).any() and (m["geom_gap"] > 0).any()
        assert len(set(m["geom_solmix"])) > 1 and len(set(m["geom_priority"])) > 1
        assert (m["geom_solref"][:, 0] < 0).sum() == 1
        assert not np.allclose(m["geom_solimp"][0], (0.9, 0.95, 0.001, 0.5, 2.0))
    r = ConRef(ms[0])
    kinds = {(int(ms[0]["geom_type"][a]), int(ms[0]["geom_type"][b])) for a, b in r.pairs}
    assert kinds == {(0, 2), (0, 3), (2, 2), (2, 3)}                # plane–sphere, plane–capsule, sphere–sphere, sphere–capsule


def test_gap_zone_contacts_have_no_rows():
    """a contact between margin − gap and margin is inactive (MuJoCo: the solver does not see it): zoo's sphere `sb` falls at
    0.6 m/s through its gap zone (margin 0.01, gap 0.004) at step 1, and the producers' step there must carry no force of that
    contact (oracle and kernel source used to give such a contact rows: backward error 0.42 there)"""
    m, task, state, mocap, _ = cc.case("zoo_elliptic")
    ref = ConRef(m)
    for p, out in _runs(m, task, state, mocap, cc.inputs("zoo_elliptic", m, N, H)):
        pairs = (np.zeros(4, int), np.arange(4))
        res = check_constrained_steps(m, out["states"], out["actions"], m["timestep"], 0, BAR, pairs=pairs, ref=ref)
        assert res["inactive"].tolist() == [0, 1, 0, 0], (p, res["inactive"])
        assert res["contacts"][2] == res["contacts"][1] + 1, (p, res["contacts"])        # the step after: the contact has its rows


def test_unsupported_models_raise():
    """a noslip pass, a weld, or a collidable pair outside the four colliders makes the reference raise: it never skips silently"""
    from mujoco_mpc_amd.modelgen import REGISTRY
    bad = dict(cc.case("zoo_elliptic")[0]); bad["noslip_iterations"] = 3
    with pytest.raises(NotImplementedError, match="noslip"):
        ConRef(bad)
    with pytest.raises(NotImplementedError, match="geom pair"):
        ConRef(cc.tighten(REGISTRY["quadruped"]()[0]))          # its boxes and cylinders are collidable
    with pytest.raises(NotImplementedError, match="weld"):
        ConRef(cc.tighten(REGISTRY["welded"]()[0]))


# ------------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("name", cc.CASES)
def test_invweights_of_modelgen_match_the_reference_mass_matrix(name):
    """dof_invweight0 / body_invweight0 / tendon_invweight0 (the model inputs behind every row's diagApprox) recomputed from
    DynRef.mass_matrix at qpos0, 1e-12 relative"""
    m = cc.case(name)[0]
    dof, body, ten = invweights(m)
    for got, want in ((dof, m["dof_invweight0"]), (body, m["body_invweight0"]), (ten, m["tendon_invweight0"])):
        want = np.asarray(want, float)
        assert got.shape == want.shape
        if want.size:
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), name


def _brute_force_cone(jar, R, mu, iters=4000):
    """argmin ½ φᵀRφ + φᵀjar over {φ_n ≥ 0, Σ (φ_k / μ_k)² ≤ φ_n²} by projected gradient in z = (φ_n, φ_k / μ_k), where the cone is
    |z_t| ≤ z_n and its Euclidean projection is elementary (the Hessian's condition number is impratio / μ_1² ≤ 34: the iteration
    contracts by 0.97 or better per step)"""
    s = np.concatenate([[1.0], mu])
    D = R * s * s; g0 = jar * s
    z = np.zeros_like(jar); step = 1.0 / D.max()
    for _ in range(iters):
        y = z - step * (D * z + g0)
        yn, yt = y[0], np.linalg.norm(y[1:])
        if yt <= yn:
            z = y
        elif yt <= -yn:
            z = np.zeros_like(y)
        else:
            a = 0.5 * (yn + yt)
            z = np.concatenate([[a], a * y[1:] / yt])
    return z * s


@pytest.mark.parametrize("dim", [3, 4, 6])
def test_cone_force_law_matches_a_brute_force_minimisation(dim):
    """F of the elliptic cone against projected gradient on 36 random jar, 1e-9 of the force scale, with points in each zone"""
    rng = np.random.default_rng(dim)
    zones = {"stick": 0, "slip": 0, "open": 0}
    for k in range(36):
        fri = np.array([1.0, 1.0, 0.05, 0.01, 0.01]) * rng.uniform(0.3, 1.5, 5); fri[1] = fri[0]; fri[4] = fri[3]
        R = elliptic_R(rng.uniform(0.01, 1.0), (1.0, 3.0)[k % 2], fri, dim)
        jar = rng.normal(size=dim) * np.sqrt(R)
        jar[0] = abs(jar[0]) + 0.1 * np.sqrt(R[0])
        if k % 3 == 0:
            jar[0] *= -3; jar[1:] *= 0.05          # pressed hard, little tangential demand: inside the cone
        elif k % 3 == 1:
            jar[0] *= 3; jar[1:] *= 0.05           # pulled apart: the polar cone
        else:
            jar[0] *= -0.3                          # pressed lightly: the boundary
        f, z = cone_force(jar, R, fri)
        zones[z] += 1
        want = _brute_force_cone(jar, R, fri[:dim - 1])
        assert np.abs(f - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), (k, z, f, want)
        assert f[0] >= 0 and ((f[1:] / fri[:dim - 1]) ** 2).sum() <= f[0] ** 2 * (1 + 1e-12)
    assert min(zones.values()) >= 6, zones


def test_impedance_is_the_documented_curve():
    """end values, the midpoint, the clipping of dmin / dmax / midpoint / power and the flat cases"""
    si = (0.8, 0.96, 0.01, 0.3, 3.0)
    assert impedance(si, 0.0) == 0.8 and impedance(si, 0.01) == 0.96 and impedance(si, 1.0) == 0.96
    assert impedance(si, 0.003) == pytest.approx(0.8 + 0.16 * 0.3, rel=1e-14)         # y(midpoint) = midpoint
    assert impedance((0.0, 1.0, 0.01, 0.5, 2), 0.0) == 1e-4 and impedance((0.0, 1.0, 0.01, 0.5, 2), 0.02) == 0.9999
    assert impedance((0.5, 0.9, 0.01, 0.5, 0.2), 0.0025) == pytest.approx(0.6, rel=1e-14)      # power < 1 is 1: linear
    assert impedance((0.7, 0.7, 0.01, 0.5, 2), 0.004) == 0.7 and impedance((0.5, 0.9, 0.0, 0.5, 2), 0.004) == 0.7
    xs = np.linspace(0, 0.01, 41)
    ys = [impedance(si, x) for x in xs]
    assert all(b > a for a, b in zip(ys, ys[1:]))


# ------------------------------------------------------------------------------------------------------ negative controls
def _with(m, **kw):
    m = dict(m)
    for k, v in kw.items():
        m[k] = v
    return m


def mutants(name):
    """(label, case the control runs on, the wrong model that is stepped); the reference keeps the true model"""
    m = cc.case(name)[0]
    g = m["names"]["geom"]
    if name == "zoo_elliptic":
        return [("impratio 1 instead of 3", _with(m, impratio=1.0))]
    solimp = np.array(m["geom_solimp"], float); solimp[g["floor"], 0] += 1e-3
    fri = np.array(m["geom_friction"], float); fri[g["floor"], 0] += 1e-3
    mix = np.array(m["geom_solmix"], float); mix[g["sb"]] = mix[g["floor"]]
    return [("floor solimp[0] + 1e-3", _with(m, geom_solimp=solimp)), ("floor sliding friction + 1e-3", _with(m, geom_friction=fri)),
            ("sb's solmix swapped for the floor's", _with(m, geom_solmix=mix)), ("iterations = 1", _with(m, iterations=1))]


CONTROLS = [("zoo_pyramidal", k) for k in range(4)] + [("zoo_elliptic", 0)]


@pytest.mark.parametrize("producer", ["oracle", "emu"])
@pytest.mark.parametrize("name, k", CONTROLS)
def test_negative_controls(name, k, producer):
    """the stepped model differs from the reference's: the check must exceed the bar of its case by 100× or more (observed
    margins: module docstring)"""
    m, task, state, mocap, _ = cc.case(name)
    label, bad = mutants(name)[k]
    out = _runs(bad, task, state, mocap, cc.inputs(name, m, N, H), (producer,))[0][1]
    res = check_constrained_steps(m, out["states"], out["actions"], m["timestep"], m["integrator"], None)
    print(f"\n[constraint-reference] negative {name} {label} {producer}: worst={res['worst']:.3e} = {res['worst'] / bar_of(m):.0f}x its bar, "
          f"{res['worst'] / BAR:.1f}x BAR")
    assert res["worst"] >= 100 * bar_of(m), (label, res["worst"])
