"""The constrained per-step check of tests/test_constraint_reference.py on the HIP engine (HipBackend.fetch_all), for every kernel flavour
and compile-time nv the engine has: each case asserts the flavour it ran on, plans 32 candidates over 12 steps and checks a fixed
seeded sample of 120 (candidate, step) pairs plus every step of 8 candidates (about 190 pairs) against the independent statement of
the constraint rows and the force law (tests/con_ref.py).  For the 8 whole candidates the engine's diagnostics (most contacts and most
rows of a state) must equal the reference's own census; the coverage conditions of each case are asserted on the sample.

BAR / BAR_QUADRATIC: the CPU tier's bars, imported (10× the worst oracle / emulation value; the second, tighter one on the cases
whose cost is piecewise quadratic).  Observed GPU maxima (Euler and implicitfast agree except on the zoo, the one case with a
velocity-dependent actuator): with elliptic cones 4.38e-6 (generic31_zoo_elliptic, implicitfast; Euler 2.69e-6), 1.04e-6
(zoo_plain), 7.5e-7 (cached18 / dense2h18 quadruped), 4.7e-7 (no_model_cache); piecewise quadratic 6.3e-13 (humanoid: cached27,
dense2, spill), 1.3e-13 (zoo_pyramidal), 5.4e-14 (quadruped_pyramidal), 1.9e-14 (direct33 hand), 7.3e-15 (cartpole); integration
9e-16.  Negative controls on the engine: floor solimp[0] + 1e-3 3.68e-3 (12 250× its bar), iterations = 1 0.998 (3.3e6×).
"""
import numpy as np
import pytest

import con_cases as cc
from con_ref import check_constrained_steps
from test_constraint_reference import BAR, BAR_QUADRATIC, bar_of, mutants

pytestmark = pytest.mark.gpu

N, H = 32, 12
INTEGRATORS = (0, 3)         # Euler, implicitfast


def _spill_flag(be):
    import ctypes as C
    n = C.c_int(0)
    return be.lib.mjpc_hip_debug_spill(be.h, C.byref(n)) == 1


def _run(name, m, task, state, mocap, knobs=(), debug_knobs=None):
    from mujoco_mpc_amd.planner import HipBackend
    for k, v in knobs:
        debug_knobs(k, v)
    inp = cc.inputs(name, m, N, H)
    be = HipBackend(m, task, max_samples=N, max_horizon=H)
    try:
        out = be.plan(state=state, mocap=mocap, time=0.0, knot_times=inp["knot_times"], knot_values=inp["knot_values"], interpolation=2,
                      num_trajectory=N, horizon=H, sigma=inp["sigma"], noise_eps=inp["noise_eps"], noise_sel=inp["noise_sel"])
        allc = be.fetch_all(N, H, len(inp["knot_times"]))
        flav = dict(spill=_spill_flag(be), dense_bytes=be.dense_tier()[0], dense_used=be.dense_tier()[1], dense_hot=be.dense_capacity()[2], lds=be.lds_bytes())
    finally:
        be.close()
    assert not out["failure"].any()
    return allc, flav


def _check(name, m, allc, claims):
    res = check_constrained_steps(m, allc["states"], allc["actions"], m["timestep"], m["integrator"], None, pairs=cc.sample_pairs(N, H),
                                  diag=allc["diag"])
    assert res["counted"] == 8
    return res, cc.coverage(res, claims, cc.contact_case(name))


# (case id, case of con_cases, knobs, flavour expected): spill / dense (hot) / plain
CASES = [
    ("cached2_cartpole", "cartpole", (), "plain"),
    ("cached18_quadruped_elliptic", "quadruped_elliptic", (), "plain"),
    ("cached18_quadruped_pyramidal", "quadruped_pyramidal", (), "plain"),
    ("cached27_humanoid", "humanoid_track", (), "plain"),
    ("direct33_hand", "shadow_hand", (), "plain"),
    ("dense2h18_quadruped", "quadruped_elliptic", (("tier", "B"),), "dense_hot"),
    ("dense2_27_humanoid", "humanoid_track", (("tier", "B"),), "dense"),
    ("spill27_knob", "humanoid_track", (("spill", "all"),), "spill"),
    ("no_model_cache_quadruped", "quadruped_elliptic", (("no_model_cache", "1"),), "plain"),
    ("dense_factor_quadruped", "quadruped_pyramidal", (("dense_factor", "1"),), "plain"),
    ("generic31_zoo_elliptic", "zoo_elliptic", (), "plain"),
    ("generic31_zoo_pyramidal", "zoo_pyramidal", (), "plain"),
    ("generic31_zoo_plain", "zoo_plain", (), "plain"),
]


@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("cid, name, knobs, flavour", CASES, ids=[c[0] for c in CASES])
def test_engine_constrained_steps_satisfy_the_reference_force_law(cid, name, knobs, flavour, integrator, debug_knobs):
    """Every flavour under Euler and implicitfast.  The knob cases show that the knob took effect: no_model_cache runs with fewer LDS
    bytes than the engine without it, dense_factor's rollouts differ in round-off from the elimination-tree order's."""
    from mujoco_mpc_amd.planner import HipBackend
    m, task, state, mocap, claims = cc.case(name)
    m["integrator"] = integrator
    assert m["nv"] == cc.NV[name]
    if cid.startswith(("no_model_cache", "dense_factor")):
        be = HipBackend(m, task, max_samples=N, max_horizon=H)
        try:
            plain_lds = be.lds_bytes()
        finally:
            be.close()
        plain, _ = _run(name, m, task, state, mocap, (), debug_knobs)
    allc, flav = _run(name, m, task, state, mocap, knobs, debug_knobs)
    assert flav["spill"] == (flavour == "spill"), flav
    assert flav["dense_used"] == flavour.startswith("dense"), flav
    if flavour.startswith("dense"):
        assert flav["dense_hot"] == (flavour == "dense_hot"), flav
    if cid.startswith("no_model_cache"):
        assert flav["lds"] < plain_lds, (flav["lds"], plain_lds)
    if cid.startswith("dense_factor"):
        assert not np.array_equal(allc["states"], plain["states"])
    res, cov = _check(name, m, allc, claims)
    print(f"\n[constraint-reference] {cid} integrator={integrator} nv={m['nv']} worst={res['worst']:.3e} pos={res['pos']:.1e} pairs={len(res['err'])} "
          f"rows<={res['rows'].max()} contacts<={res['contacts'].max()} {cov}")
    assert res["worst"] <= bar_of(m), res["worst"]
    assert res["pos"] <= 1e-14 and res["act"] <= 1e-14


@pytest.mark.parametrize("k", [0, 3], ids=["solimp", "iterations1"])
def test_engine_negative_controls(k, debug_knobs):
    """the engine steps a zoo whose floor has solimp[0] off by 1e-3, or whose solver stops after one iteration (an ordinary, valid
    option value); the reference keeps the true model: the check exceeds the bar of the case by 100× or more"""
    m, task, state, mocap, _ = cc.case("zoo_pyramidal")
    label, bad = mutants("zoo_pyramidal")[k]
    allc, _ = _run("zoo_pyramidal", bad, task, state, mocap, (), debug_knobs)
    res = check_constrained_steps(m, allc["states"], allc["actions"], m["timestep"], m["integrator"], None, pairs=cc.sample_pairs(N, H))
    print(f"\n[constraint-reference] negative {label}: worst={res['worst']:.3e} = {res['worst'] / bar_of(m):.0f}x its bar, {res['worst'] / BAR:.1f}x BAR")
    assert bar_of(m) == BAR_QUADRATIC
    assert res["worst"] >= 100 * bar_of(m)
