"""CPU tier of the inverse-dynamics tests: the inverse kernel (csrc/inverse.h) and its finite-difference kernels (csrc/inverse_fd.h) in
the 1-lane emulation (tests/emu/emu_inverse.cpp) against the independent reference of tests/inv_ref.py (forces) and tests/acc_ref.py
(residual rows, through tests/late_checks.py).  Cases and bars: tests/inverse_cases.py; every figure is printed before it is asserted
(pytest -s shows them; they are the *_MEASURED constants there)."""
import functools

import numpy as np
import pytest

import emu_inverse_lib as el
import inv_ref as ir
import inverse_cases as ic
import late_checks as lk
from dyn_ref import _t

WARN_BADQACC = 4


# ---------------------------------------------------------------------------------------------------------------- measurements
def measure_reference(name, run):
    """run(case, X, U, A, T, discrete) -> (qfrc_inverse, qfrc_constraint, residual, failure).  Returns (force deviation, residual
    deviation) after the coverage checks"""
    c = ic.case(name); m = c["model"]
    w = ir.evaluate(ir.InvRef(m), m, c["X"], c["U"], c["A"])                      # raises NearMargin: no state may sit on a margin
    if c["contact"]:
        assert (w["ncon"] > 0).any() and w["fmax"].max() > 1.0, f"{name}: contacts {w['ncon']}, largest force {w['fmax'].max():.3g} N"
        assert ((w["ncon"] > 0) & (w["fmax"] > 1.0)).any()
    fi, fc, res, fail = run(c, c["X"], c["U"], c["A"], c["T"], False)
    assert not fail.any(), fail
    assert np.array_equal(res[:, ic.qacc_rows(c)], c["A"]), "the QACC rows are the given acceleration"
    if c["contact"]:
        worst, refs = lk.touch_deviation(c["late"], res)
        assert all(len(r["forces"]) > 0 for r in refs)
    else:
        worst = lk.kinematic_deviation(c["late"], res)[0]
    force = max(ir.dev(fi, w["qfrc_inverse"]), ir.dev(fc, w["qfrc_constraint"]))
    print(f"{name}: forces {force:.2e} residual {worst:.2e}")
    return force, worst


def roundtrip_wants(c, nxt):
    """(a_d, qfrc_actuator, qfrc_constraint = A a_d - (tau - c)) of the forward steps X -> nxt, from DynRef alone"""
    m = c["model"]; nq, nv = m["nq"], m["nv"]; h = float(m["timestep"])
    ad = (nxt[:, nq:nq + nv] - c["X"][:, nq:nq + nv]) / h
    ref = ir.InvRef(m)
    q, v, act = ir.split(m, c["X"])
    A, f, ex = ref.dyn.step_system(q, v, act, c["U"], h, ref.integrator)
    want_con = ((A @ _t(ad).unsqueeze(-1)).squeeze(-1) - f).numpy()
    want_act = (ex["tau"] - ref.passive_dyn.force(_t(q), _t(v), _t(act), _t(c["U"]), ex["jac"])).numpy()
    return ad, want_act, want_con


def measure_roundtrip(name, step, run, forward_forces=None):
    """step(case) -> next states of the forward steps.  No noslip model among the cases: the inverse has no noslip pass, so the
    identity does not hold behind one (ConRef refuses such a model).  The QACC rows of the residual must be the CONVERTED continuous
    acceleration (the reference's M^-1 A a_d): late rows under discrete = 1 are evaluated there.  forward_forces(case): the forward
    steps' own qfrc_constraint where the tier can read it (the emulation's LDS image): the literal identity"""
    c = ic.case(name); m = c["model"]
    assert int(m.get("noslip_iterations", 0)) <= 0
    nxt = step(c)
    ad, want_act, want_con = roundtrip_wants(c, nxt)
    fi, fc, res, fail = run(c, c["X"], c["U"], ad, c["T"], True)
    assert not fail.any(), fail
    ac = ir.evaluate(ir.InvRef(m), m, c["X"], c["U"], ad, discrete=True)["qacc"]
    figures = dict(actuator=ir.dev(fi, want_act), constraint=ir.dev(fc, want_con), qacc_rows=ir.dev(res[:, ic.qacc_rows(c)], ac))
    if forward_forces is not None:
        figures["forward"] = ir.dev(fc, forward_forces(c))
    d = max(figures.values())
    print(f"{name}: round trip {d:.2e} " + " ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    return d


def measure_fd(name, centered, fd, T=1):
    """fd(case, rows, centered) -> dict of the six blocks + failure.  Returns (largest block deviation, DfDa against M, the QACC block
    of DsDa against the identity)"""
    c = ic.case(name); nv = c["model"]["nv"]
    want = ic.fd_reference(name, centered, T)
    o = fd(c, slice(1, 1 + T), centered)
    assert not o["failure"].any(), o["failure"]
    if "table" in o:
        assert np.array_equal(o["table"], want["table"]), "the nudged table is not the documented one bit for bit"
    worst = max(ir.dev(o[k], want[k]) for k in ic.BLOCKS)
    dm = ir.dev(o["DfDa"], want["M"])
    di = ir.dev(o["DsDa"][:, ic.qacc_rows(c)], np.broadcast_to(np.eye(nv), (T, nv, nv)))
    print(f"{name} {'centred' if centered else 'one-sided'} T={T}: blocks {worst:.2e} DfDa-M {dm:.2e} DsDa-I {di:.2e}")
    return worst, dm, di


def emu_run(c, X, U, A, T, discrete):
    return el.inverse_batch(c["model"], c["task"], X, U, A, T, c["mocap"], discrete=discrete)


def emu_step(c):
    return el.step_batch(c["model"], c["task"], c["X"], c["U"], c["T"], c["mocap"])[0]


def emu_forward_forces(c):
    return np.array([el.step_forces(c["model"], c["task"], c["X"][i], c["U"][i], c["T"][i], c["mocap"])[0] for i in range(len(c["X"]))])


def emu_fd(c, rows, centered, **kw):
    return el.inverse_fd(c["model"], c["task"], c["X"][rows], c["U"][rows], c["A"][rows], c["T"][rows], c["mocap"], eps=ic.FD_EPS, centered=centered, **kw)


# ---------------------------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize("name", ic.CASES)
def test_against_reference(name):
    force, res = measure_reference(name, emu_run)
    assert force <= ic.bar(ic.FORCE_MEASURED, name) and res <= ic.bar(ic.RESIDUAL_MEASURED, name)


# ---------------------------------------------------------------------------------------------------------------- 2. round trip
@pytest.mark.parametrize("name", ic.CASES)
def test_round_trip(name):
    assert measure_roundtrip(name, emu_step, emu_run, emu_forward_forces) <= ic.bar(ic.ROUNDTRIP_MEASURED, name)


def continuous_vs_discrete(step_res, run):
    """on a model with damping: the continuous acceleration (a step's QACC rows) with discrete = 0 gives back qfrc_actuator; fed to
    discrete = 1 it is taken for (v' - v) / h and must give something else"""
    c = ic.case(ic.DAMPED)
    assert np.asarray(c["model"]["dof_damping"]).max() > 0
    nxt, res = step_res(c)
    a = res[:, ic.qacc_rows(c)]
    _, want_act, _ = roundtrip_wants(c, nxt)
    f0 = run(c, c["X"], c["U"], a, c["T"], False)[0]
    f1 = run(c, c["X"], c["U"], a, c["T"], True)[0]
    d0, d1 = ir.dev(f0, want_act), ir.dev(f1, want_act)
    print(f"{ic.DAMPED}: continuous a, discrete=0 {d0:.2e}, discrete=1 {d1:.2e}")
    return d0, d1


def test_continuous_acceleration_and_the_flag():
    d0, d1 = continuous_vs_discrete(lambda c: el.step_batch(c["model"], c["task"], c["X"], c["U"], c["T"], c["mocap"])[:2], emu_run)
    assert d0 <= ic.bar(ic.ROUNDTRIP_MEASURED, ic.DAMPED)
    assert d1 > 1000 * ic.bar(ic.ROUNDTRIP_MEASURED, ic.DAMPED), "discrete = 1 changes nothing"


# ---------------------------------------------------------------------------------------------------------------- 3. FD blocks
@pytest.mark.parametrize("centered", [False, True], ids=["onesided", "centred"])
@pytest.mark.parametrize("name", ic.CASES)
def test_fd_blocks(name, centered):
    worst, dm, di = measure_fd(name, centered, lambda c, rows, cen: emu_fd(c, rows, cen))
    assert worst <= ic.bar(ic.FD_MEASURED, name)
    if not ic.case(name)["contact"]:
        assert dm <= ic.bar(ic.FD_MASS_MEASURED, name) and di <= ic.bar(ic.FD_MASS_MEASURED, name)


def test_fd_three_configurations_and_null_blocks():
    """T = 3 in one call equals three calls at T = 1; a block that is not asked for is not written and the others do not change"""
    c = ic.case("chain3_euler")
    o3 = emu_fd(c, slice(1, 4), False)
    for t in range(3):
        o1 = emu_fd(c, slice(1 + t, 2 + t), False)
        for k in ic.BLOCKS:
            assert np.array_equal(o3[k][t], o1[k][0]), (k, t)
    worst, _, _ = measure_fd("chain3_euler", False, lambda c_, rows, cen: emu_fd(c_, rows, cen), T=3)
    assert worst <= ic.bar(ic.FD_MEASURED, "chain3_euler")
    part = emu_fd(c, slice(1, 4), False, want=(0, 1, 0, 1, 0, 0))
    assert part["DfDq"] is None and part["DsDa"] is None
    assert np.array_equal(part["DfDv"], o3["DfDv"]) and np.array_equal(part["DsDq"], o3["DsDq"])


# ---------------------------------------------------------------------------------------------------------------- 4. errors and failures
def test_discrete_refused_on_dense_implicit_model():
    from mujoco_mpc_amd.modelgen import REGISTRY
    m, task, d = REGISTRY["swimmer"]()
    x = np.asarray(d["state"], float)[None]
    with pytest.raises(ValueError, match="dense implicit"):
        el.inverse_batch(m, task, x, np.zeros((1, m["nu"])), np.zeros((1, m["nv"])), [0.0], d["mocap"] if len(d["mocap"]) else None, discrete=True)
    fi, fc, res, fail = el.inverse_batch(m, task, x, np.zeros((1, m["nu"])), np.zeros((1, m["nv"])), [0.0], d["mocap"] if len(d["mocap"]) else None)
    assert fail[0] == 0 and np.isfinite(fi).all()           # discrete = 0 works for it


def nan_row(run):
    c = ic.case("chain3_euler")
    A = c["A"].copy(); A[2, 1] = np.nan
    fi, fc, res, fail = run(c, c["X"], c["U"], A, c["T"], False)
    ok = [0, 1, 3, 4]
    f0 = run(c, c["X"], c["U"], c["A"], c["T"], False)[0]
    assert fail[2] & WARN_BADQACC and not fail[ok].any(), fail
    assert np.array_equal(fi[ok], f0[ok])
    A[2, 1] = np.inf
    assert run(c, c["X"], c["U"], A, c["T"], False)[3][2] & WARN_BADQACC


def test_nan_acceleration_fails_its_row_only():
    nan_row(emu_run)


def test_bad_state_reports_nan_forces():
    c = ic.case("chain3_euler")
    X = c["X"].copy(); X[1, 0] = np.nan
    fi, fc, res, fail = emu_run(c, X, c["U"], c["A"], c["T"], False)
    assert fail[1] & 1 and np.isnan(fi[1]).all() and np.isnan(fc[1]).all() and np.isnan(res[1]).all() and not fail[[0, 2, 3, 4]].any()


# ---------------------------------------------------------------------------------------------------------------- 5. unchanged behaviour
@pytest.mark.parametrize("name", ["particle", "particle_copystate", "quadruped", "filter_arm", "humanoid_spill"])
def test_step_kernels_unchanged_next_to_the_inverse_kernel(name):
    """the one-step kernel and its finite-difference derivatives compiled in the translation unit that also holds the inverse kernel
    give the bits of the build that does not know it (tests/emu/emu_transition.cpp), on the models of transition_cases"""
    import emu_transition_lib as et
    import transition_cases as tc
    m, task, mocap, X, U, T = tc.batch(name, n=3)
    for x, y in zip(et.step_batch(m, task, X, U, T, mocap), el.step_batch(m, task, X, U, T, mocap)):
        assert np.array_equal(x, y, equal_nan=True)
    for centered in ((False,) if name == "humanoid_spill" else (False, True)):          # (the humanoid: 76 emulated steps per knot)
        kw = dict(eps=1e-6, centered=centered, last_is_terminal=True)
        a = et.transition_fd(m, task, X[:2], U[:2], T[:2], mocap, **kw); b = el.transition_fd(m, task, X[:2], U[:2], T[:2], mocap, **kw)
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True) and x.size


# ---------------------------------------------------------------------------------------------------------------- the spill flavour's model
@functools.lru_cache(maxsize=None)
def humanoid_spill_case():
    """(case, reference) of the humanoid of con_cases (its low-standing state: feet in the floor) at 64 contacts / 192 rows, the
    capacity at which it needs the spill flavour on the device; three rows that differ in velocity, control and acceleration"""
    import con_cases as cc
    from spill_common import with_capacity
    m, task, state, mocap, _ = cc.case("humanoid_track")
    m = with_capacity((m, task, None), 64, 192)[0]
    rng = np.random.default_rng(77)
    nq, nv = m["nq"], m["nv"]
    X = np.tile(np.asarray(state, float), (3, 1)); X[1:, nq:nq + nv] += 0.05 * rng.standard_normal((2, nv))
    U = rng.uniform(-0.3, 0.3, (3, m["nu"])); A = rng.uniform(-2.0, 2.0, (3, nv)); A[0] = 0.0
    c = dict(model=m, task=task, mocap=mocap, X=X, U=U, T=np.zeros(3), A=A, contact=True)
    return c, ir.evaluate(ir.InvRef(m), m, X, U, A)


def test_humanoid_spill_model_in_emulation():
    c, w = humanoid_spill_case()
    assert (w["ncon"] > 0).all() and w["fmax"].max() > 1.0
    fi, fc, res, fail = emu_run(c, c["X"], c["U"], c["A"], c["T"], False)
    d = max(ir.dev(fi, w["qfrc_inverse"]), ir.dev(fc, w["qfrc_constraint"]))
    print(f"humanoid at spill capacity: forces {d:.2e}, contacts {w['ncon']}, largest force {w['fmax'].max():.1f}")
    assert not fail.any() and d <= 10 * ic.HUMANOID_SPILL_MEASURED


# ---------------------------------------------------------------------------------------------------------------- row stages (host only)
def test_row_stages_come_from_the_table():
    """position blocks 0, velocity blocks 1, every late block 2 (the stage a window end keeps or drops, InverseDerivatives)"""
    from mujoco_mpc_amd.derivatives import InverseDerivatives
    c = ic.case("chain3_euler"); rows = c["late"]["rows"]
    idv = InverseDerivatives(c["model"], c["task"], T=2)
    st = idv.row_stages()
    assert (st[rows["qpos"]] == 0).all() and (st[rows["qvel"]] == 1).all()
    for k in ("qacc", "accelerometer", "gyro", "velocimeter", "linacc_site", "angacc_site", "norm", "mixed"):
        assert (st[rows[k]] == 2).all(), k
    idv.set_row_stages(np.zeros_like(st)); assert not idv.row_stages().any()
    idv.close()
    from mujoco_mpc_amd.modelgen import REGISTRY
    m, task, _ = REGISTRY["cartpole"]()                       # not a table: every row counts as acceleration stage
    idv = InverseDerivatives(m, task)
    assert (idv.row_stages() == 2).all()
    idv.close()


# ---------------------------------------------------------------------------------------------------------------- the particle, bit for bit
def particle_numpy_loop(run):
    """no quaternion, unit joint axes, unit gear and damping: the kernel's sum written out in numpy in the kernel's own order,
    ((M a - qfrc_smooth) + qfrc_actuator) - qfrc_constraint with qfrc_smooth = (actuator - bias) - damping v, gives its bits"""
    c = ic.case("particle_imu"); m = c["model"]; nq, nv = m["nq"], m["nv"]
    assert m["nu"] == nv and not np.asarray(m["actuator_biastype"]).any()
    v = c["X"][:, nq:nq + nv]
    mass = float(np.asarray(m["body_mass"]).ravel()[-1]) + np.asarray(m["dof_armature"], float)
    lo, hi = np.asarray(m["actuator_ctrlrange"], float).reshape(-1, 2).T
    act = np.asarray(m["actuator_gear"], float).ravel()[:nv] * (np.asarray(m["actuator_gainprm"], float).reshape(-1, 3)[:, 0] * np.clip(c["U"], lo, hi))
    smooth = (act - 0.0) - np.asarray(m["dof_damping"], float) * v
    want = ((mass * c["A"] - smooth) + act) - 0.0
    fi, fc, _, fail = run(c, c["X"], c["U"], c["A"], c["T"], False)
    assert not fail.any() and np.array_equal(fi, want) and not fc.any() and np.abs(want).max() > 0.1


def test_particle_forces_equal_the_numpy_loop_bit_for_bit():
    particle_numpy_loop(emu_run)


# ---------------------------------------------------------------------------------------------------------------- site transmissions
@functools.lru_cache(maxsize=None)
def zoo_case():
    """con_cases' zoo (nv = 31: the generic kernels): two actuators push through site transmissions, two through joints, with every row
    type of the constraint reference active; three rows that differ in velocity, control and acceleration.  The reference takes the
    actuator forces out of its passive term and the kernel puts its own back, so a wrong moment shows in qfrc_inverse"""
    import con_cases as cc
    m, task, state, mocap, _ = cc.case("zoo_plain")
    assert sum(int(t) == 4 for t in m["actuator_trntype"]) == 2
    rng = np.random.default_rng(78)
    nq, nv = m["nq"], m["nv"]
    X = np.tile(np.asarray(state, float), (3, 1)); X[1:, nq:nq + nv] += 0.05 * rng.standard_normal((2, nv))
    U = rng.uniform(-0.9, 0.9, (3, m["nu"])); A = rng.uniform(-2.0, 2.0, (3, nv)); A[0] = 0.0
    c = dict(model=m, task=task, mocap=mocap, X=X, U=U, T=np.zeros(3), A=A, contact=True)
    return c, ir.evaluate(ir.InvRef(m), m, X, U, A)


def measure_zoo(run):
    c, w = zoo_case()
    m = c["model"]; site = [i for i in range(m["nu"]) if int(m["actuator_trntype"][i]) == 4]
    assert np.abs(w["qfrc_actuator"]).max() > 0.5 and np.abs(c["U"][:, site]).min() > 0.01
    fi, fc, _, fail = run(c, c["X"], c["U"], c["A"], c["T"], False)
    d = max(ir.dev(fi, w["qfrc_inverse"]), ir.dev(fc, w["qfrc_constraint"]))
    print(f"zoo with site transmissions: forces {d:.2e}, rows {w['nefc']}, largest force {w['fmax'].max():.1f}")
    assert not fail.any()
    return d


def test_site_transmissions_on_the_zoo():
    assert measure_zoo(emu_run) <= 10 * ic.ZOO_MEASURED
