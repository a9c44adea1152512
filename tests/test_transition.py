"""CPU tier of the batched one-step evaluation and the finite-difference transition derivatives: the kernel source
(csrc/transition.h, csrc/transition_fd.h) in the 1-lane emulation against the oracle, the numpy mirror and the particle's closed form;
mjpc_hip::ModelDerivatives' host halves; and the rollout translation units' independence of the new header.

Emulated transition_fd against the mirror over ORACLE steps (test_fd_matches_mirror_over_oracle_steps): two independent step functions
compared through a 1 / eps amplifier, so the bar cannot be derived.  Centred, eps = 1e-4, largest deviation over every entry of
A, B, C, D relative to max(1, |entry|), measured on the CPU:
    particle 4.4e-15   cartpole 6.9e-14   quadruped (A1 standing) 1.4e-11   filter_arm 1.1e-12
The bar is 10 x that per model (FD_ORACLE_BAR below).  At the same states the oracle against itself under a one-ulp change of qpos
stays inside the bar (checked in the test)."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import emu_transition_lib as et
import transition_cases as tc
import transition_mirror as tm
from mujoco_mpc_amd.derivatives import ModelDerivatives

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mujoco_mpc_amd", "csrc")

# one-step parity bars: those of tests/test_kernel_emu.py for the same models
STEP_BAR = {"particle": 1e-12, "cartpole": 1e-12, "quadruped": 1e-5, "filter_arm": 1e-9}
FD_ORACLE_MEASURED = {"particle": 4.4e-15, "cartpole": 6.9e-14, "quadruped": 1.4e-11, "filter_arm": 1.1e-12}
FD_ORACLE_BAR = {k: 10 * v for k, v in FD_ORACLE_MEASURED.items()}
QUAT_BAR = 1e-8


def _rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-300)


def _emu_step(m, task, mocap):
    return lambda S, U, T: et.step_batch(m, task, S, U, T, mocap)


def _dev(got, want):
    return np.nanmax(np.abs(got - want) / np.maximum(1.0, np.abs(want))) if got.size else 0.0


@pytest.mark.parametrize("name", ["particle", "cartpole", "quadruped", "filter_arm"])
def test_emulated_step_batch_matches_oracle(name):
    m, task, mocap, X, U, T = tc.batch(name, n=5)
    nxt, res, fail = et.step_batch(m, task, X, U, T, mocap)
    onxt, ores, ofail = tc.oracle_step(m, task, mocap)(X, U, T)
    print(name, "next", _rel(nxt, onxt), "residual", _rel(res, ores))
    assert _rel(nxt, onxt) < STEP_BAR[name] and _rel(res, ores) < STEP_BAR[name]
    assert not fail.any() and not ofail.any()
    assert len({r.tobytes() for r in nxt}) == 5                       # distinct states, controls and times gave distinct rows
    # a row does not depend on its neighbours: the batch in another order
    p = np.array([3, 0, 4, 2, 1])
    nxt2, res2, _ = et.step_batch(m, task, X[p], U[p], T[p], mocap)
    assert np.array_equal(nxt2, nxt[p]) and np.array_equal(res2, res[p])


@pytest.mark.parametrize("centered", [False, True])
def test_particle_closed_form(centered):
    """Two slide joints, damping d, mass m, gear g, limits inactive near the origin, Euler with implicit damping:
    a = 1 - h d / (m + h d), A = [[I, h a I], [0, a I]], B = g [[h^2 / (m + h d) I], [h / (m + h d) I]]; copy-state residual: C = I, D = 0.
    Linear, so the differences are exact up to ulp / eps: 1e-8 absolute at eps = 1e-6."""
    m, task, mocap, X, U, T = tc.batch("particle_copystate", n=2, spread=0.5)
    h = m["timestep"]; d = float(np.asarray(m["dof_damping"])[0])
    mass = float(np.asarray(m["body_mass"]).ravel()[-1]) + float(np.asarray(m["dof_armature"])[0]); gear = float(np.asarray(m["actuator_gear"]).ravel()[0])
    assert (h, d, mass, gear) == (0.1, 1.0, 0.3, 1.0)
    a = 1 - h * d / (mass + h * d)
    I2, Z2 = np.eye(2), np.zeros((2, 2))
    A = np.block([[I2, h * a * I2], [Z2, a * I2]]); B = gear * np.vstack([h * h / (mass + h * d) * I2, h / (mass + h * d) * I2])
    gA, gB, gC, gD, fail = et.transition_fd(m, task, X, U, T, mocap, 1e-6, centered)
    for t in range(2):
        for got, want in ((gA[t], A), (gB[t], B), (gC[t], np.eye(4)), (gD[t], np.zeros((4, 2)))):
            assert np.abs(got - want).max() <= 1e-8
    assert not fail.any()


@pytest.mark.parametrize("name", ["particle", "cartpole", "quadruped", "filter_arm"])
@pytest.mark.parametrize("centered", [False, True])
def test_emulated_fd_matches_mirror_over_emulated_steps(name, centered):
    """entries on plain coordinates bit-equal; ball / free-rotation rows within 1e-8 max(1, |entry|)"""
    m, task, mocap, X, U, T = tc.batch(name, n=2)
    A, B, C, D, fail = et.transition_fd(m, task, X, U, T, mocap, 1e-6, centered)
    rA, rB, rC, rD, rfail, q = tm.Mirror(m, task).fd(_emu_step(m, task, mocap), X, U, T, 1e-6, centered)
    assert q.any() == (name == "quadruped")
    assert np.array_equal(A[:, ~q], rA[:, ~q]) and np.array_equal(B[:, ~q], rB[:, ~q]) and np.array_equal(C, rC) and np.array_equal(D, rD)
    assert _dev(A[:, q], rA[:, q]) <= QUAT_BAR and _dev(B[:, q], rB[:, q]) <= QUAT_BAR
    assert np.isfinite(A).all() and np.isfinite(B).all() and np.isfinite(C).all() and np.isfinite(D).all()
    assert np.array_equal(fail, rfail) and not fail.any()


@pytest.mark.parametrize("name", ["particle", "cartpole", "quadruped", "filter_arm"])
def test_fd_matches_mirror_over_oracle_steps(name):
    m, task, mocap, X, U, T = tc.batch(name, n=2)
    eps = 1e-4
    mir = tm.Mirror(m, task)
    ostep = tc.oracle_step(m, task, mocap)
    got = et.transition_fd(m, task, X, U, T, mocap, eps, True)
    ref = mir.fd(ostep, X, U, T, eps, True)
    dev = max(_dev(g, r) for g, r in zip(got[:4], ref[:4]))
    print(name, "largest deviation", dev, "bar", FD_ORACLE_BAR[name])
    assert dev <= FD_ORACLE_BAR[name]                                    # every entry, none excluded
    # the states are not on a knife's edge: the oracle against itself with qpos moved by one ulp stays inside the same bar
    X1 = X.copy(); nq = m["nq"]
    X1[:, :nq] = np.nextafter(X[:, :nq], np.inf)
    ref1 = mir.fd(ostep, X1, U, T, eps, True)
    self_dev = max(_dev(a, b) for a, b in zip(ref1[:4], ref[:4]))
    print(name, "oracle against itself, one ulp of qpos", self_dev)
    assert self_dev <= FD_ORACLE_BAR[name]


@pytest.mark.parametrize("centered", [False, True])
def test_control_nudges_and_terminal_knot(centered):
    """one actuator at hi, one at lo, one inside, one with hi - lo < eps (a zero column); the last knot terminal: C only"""
    m, task, mocap, X, U, T = tc.batch("filter_arm", n=3)
    m, U, eps = tc.nudge_case(m, U)
    mir = tm.Mirror(m, task)
    assert mir.flags(U[0], eps, centered)[:4] == [(False, True), (True, False), (True, centered), (False, False)]
    A, B, C, D, fail = et.transition_fd(m, task, X, U, T, mocap, eps, centered, last_is_terminal=True, fill=np.nan)
    rA, rB, rC, rD, rfail, q = mir.fd(_emu_step(m, task, mocap), X, U, T, eps, centered, last_is_terminal=True)
    for got, want in ((A, rA), (B, rB), (C, rC), (D, rD)):
        assert np.array_equal(got, want, equal_nan=True)
    assert np.all(B[:2, :, 3] == 0) and np.all(D[:2, :, 3] == 0) and np.abs(B[:2, :, :3]).max(axis=(0, 1)).min() > 0
    assert np.isnan(A[2]).all() and np.isnan(B[2]).all() and np.isnan(D[2]).all() and np.isfinite(C).all() and np.isfinite(A[:2]).all()
    # the one-sided columns against the steps themselves: backward-only is (base - y(-eps)) / eps, forward-only (y(+eps) - base) / eps
    step = _emu_step(m, task, mocap)
    base = step(X[:1], U[:1], T[:1])[0][0]
    for k, sgn in ((0, -1.0), (1, 1.0)):
        Uk = U[:1].copy(); Uk[0, k] += sgn * eps
        y = step(X[:1], Uk, T[:1])[0][0]
        col = (y - base) / eps if sgn > 0 else (base - y) / eps
        nq = m["nq"]
        assert np.array_equal(B[0, m["nv"]:, k], col[nq:])               # velocity and activation rows: plain differences
    assert np.array_equal(fail, rfail)


def test_nan_state_is_flagged_in_its_row_only():
    m, task, mocap, X, U, T = tc.batch("quadruped", n=4)
    good = et.step_batch(m, task, X, U, T, mocap)
    Xb = X.copy(); Xb[1, 2] = np.nan
    nxt, res, fail = et.step_batch(m, task, Xb, U, T, mocap)
    assert fail[1] & 1 and not fail[[0, 2, 3]].any() and np.isnan(res[1]).all()
    for i in (0, 2, 3):
        assert np.array_equal(nxt[i], good[0][i]) and np.array_equal(res[i], good[1][i])
    A, B, C, D, f = et.transition_fd(m, task, Xb[:2], U[:2], T[:2], mocap, 1e-6, False)
    assert f[0] == 0 and f[1] & 1


# ----------------------------------------------------------------------------- ModelDerivatives: index sets and interpolation
@pytest.mark.parametrize("T", [2, 3, 4, 5, 9])
@pytest.mark.parametrize("skip", [0, 1, 2, 7])
def test_model_derivatives_index_sets_and_interpolation(T, skip):
    nd, nu, nr = 5, 2, 3
    md = ModelDerivatives(dims=(6, nd, nu, nr), T=T)
    ev, it = md.index_sets(T, skip)
    want_ev, plan = tm.interpolate_plan(T, skip)
    assert list(ev) == want_ev and list(it) == [p[0] for p in plan] and sorted(list(ev) + list(it)) == list(range(T))
    assert len(set(ev)) == len(ev) and {0, T - 2, T - 1} <= set(ev)                    # an index the reference lists twice: once
    rng = np.random.default_rng(T * 10 + skip)
    blocks = [rng.standard_normal((T, nd, nd)), rng.standard_normal((T, nd, nu)), rng.standard_normal((T, nr, nd)), rng.standard_normal((T, nr, nu))]
    md.set_blocks(*blocks)
    md.interpolate()
    out = md.blocks(T)
    for k, src in zip("ABCD", blocks):
        for t in ev:
            assert np.array_equal(out[k][t], src[t])
        for t, lo, up, tt in plan:
            assert 0 < tt < 1 and np.array_equal(out[k][t], tm.interpolate(src[lo], src[up], tt)), (k, t)
    md.close()


def test_model_derivatives_refuses_short_trajectories():
    from mujoco_mpc_amd import cplanner
    md = ModelDerivatives(dims=(4, 4, 2, 4), T=2)
    for T in (1, 0):
        with pytest.raises(cplanner.PlannerError, match="T < 2"):
            md.index_sets(T, 0)
    md.close()


# ----------------------------------------------------------------------------- the rollout kernels are not touched
ROLLOUT_TUS = ["rollout_cached", "rollout_direct", "rollout_dense2", "rollout_dense2h", "rollout_spill"]


@pytest.mark.parametrize("tu", ROLLOUT_TUS)
def test_rollout_translation_units_do_not_reach_the_transition_headers(tu):
    """the dependency list of each existing rollout translation unit (host side) names neither transition.h nor what includes it"""
    import __graft_entry__ as g
    deps = subprocess.check_output([g.HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-M", os.path.join(CSRC, tu + ".hip")], cwd=CSRC).decode()
    names = {os.path.basename(p) for p in deps.replace("\\\n", " ").split()}
    assert "core.h" in names and "rollout_tu.inc" in names
    assert not names & {"transition.h", "transition_fd.h", "step_tu.h"}


def test_step_translation_units_use_their_rollout_flavours_switches():
    """each step TU sets the macros of the rollout TU of its flavour (same MJPC_TU_NVT_LIST, same flavour switches)"""
    import re
    for fl in ("cached", "direct", "spill"):
        def macros(path):
            out = {}
            for line in open(os.path.join(CSRC, path)):
                mm = re.match(r"#define\s+(\w+)(?:\(\w+\))?\s*(.*?)\s*(//.*)?$", line)
                if mm:
                    out[mm.group(1)] = mm.group(2)
            return out
        a, b = macros(f"rollout_{fl}.hip"), macros(f"rollout_step_{fl}.hip")
        a.pop("MJPC_MIN_BLOCKS", None)                 # 1 in both: the step header fixes it
        assert a == b, fl


def test_rollout_and_step_objects_are_built():
    """sha256 of the built rollout objects, printed for the record (the parent's hashes are in the commit message: they cannot be a
    fixture without a parent build); here only that the five objects exist next to the three new ones after a build"""
    import __graft_entry__ as g
    g.build_engine()
    objdir = os.path.join(CSRC, "_obj")
    for tu in ROLLOUT_TUS + ["rollout_step_cached", "rollout_step_direct", "rollout_step_spill"]:
        p = os.path.join(objdir, tu + ".o")
        assert os.path.exists(p), tu
        print(tu, hashlib.sha256(open(p, "rb").read()).hexdigest())
