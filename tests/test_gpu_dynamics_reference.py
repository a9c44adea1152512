"""The per-step dynamics check of tests/test_dynamics_reference.py on the HIP engine (HipBackend.fetch_all), for every kernel flavour
and compile-time nv the engine has: each case asserts the flavour it ran on, plans 64 candidates (more than one workgroup and wave-role
mix) and checks a fixed seeded sample of 200 (candidate, step) pairs against the independent reference (tests/dyn_ref.py).

BAR: the CPU tier's bar (10× the worst oracle / emulation value).  Observed GPU maxima over every case below, per integrator:
Euler 1.23e-14, implicitfast 1.23e-14, implicit 1.23e-14 (each on random seed 12, generic nv = 26); on the compile-time-nv
flavours Euler 4.6e-15, implicitfast 4.6e-15, implicit 6.8e-15 (cached<18>): the lane-parallel RNE / CRBA and FMA contraction keep
the CPU's round-off level.  Negative controls on the engine: mass 1.1e-7 (5.4e5× the bar), frame 1.2e-9 (5.8e3×).
"""
import numpy as np
import pytest

import dyn_cases as dc
from dyn_ref import DynRef, _t, check_steps
from test_dynamics_reference import BAR

pytestmark = pytest.mark.gpu

N, H, PAIRS = 64, 20, 200


INTEGRATORS = (0, 3, 2)      # Euler, implicitfast, implicit


def _lds_bytes(m, task):
    """LDS bytes per candidate of the engine mjpc_hip_create builds for this model under the knobs set now"""
    from mujoco_mpc_amd.planner import HipBackend
    be = HipBackend(m, task, max_samples=N, max_horizon=H)
    try:
        return be.lds_bytes()
    finally:
        be.close()


def _run(m, task, state, mocap, knobs=(), debug_knobs=None):
    from mujoco_mpc_amd.planner import HipBackend
    for k, v in knobs:
        debug_knobs(k, v)
    inp = dc.plan_inputs(m, N, H)
    be = HipBackend(m, task, max_samples=N, max_horizon=H)
    try:
        out = be.plan(state=state, mocap=mocap, time=0.0, knot_times=inp["knot_times"], knot_values=inp["knot_values"], interpolation=2,
                      num_trajectory=N, horizon=H, sigma=inp["sigma"], noise_eps=inp["noise_eps"], noise_sel=inp["noise_sel"])
        allc = be.fetch_all(N, H, len(inp["knot_times"]))
        flav = dict(spill=_spill_flag(be), dense_bytes=be.dense_tier()[0], dense_used=be.dense_tier()[1], dense_hot=be.dense_capacity()[2], lds=be.lds_bytes())
        frame = _frame(be, m)
    finally:
        be.close()
    assert not out["failure"].any()
    assert (allc["diag"][:, 2] == 0).all(), "a constraint row existed"
    return allc, flav, frame


def _spill_flag(be):
    import ctypes as C
    n = C.c_int(0)
    return be.lib.mjpc_hip_debug_spill(be.h, C.byref(n)) == 1


def _frame(be, m):
    from mujoco_mpc_amd import capi
    nb, ns = m["nbody"], m["nsite"]
    f = dict(xpos=np.zeros((nb, 3)), xmat=np.zeros((nb, 9)), site_xpos=np.zeros((max(ns, 1), 3)), subtree_com=np.zeros((nb, 3)),
             subtree_linvel=np.zeros((nb, 3)))
    assert be.lib.mjpc_hip_get_frame(be.h, *[f[k].ctypes.data_as(capi.c_double_p) for k in ("xpos", "xmat", "site_xpos", "subtree_com", "subtree_linvel")]) == 0
    f["site_xpos"] = f["site_xpos"][:ns]
    return f


def _pairs(seed=0):
    rng = np.random.default_rng(seed)
    k = rng.choice(N * (H - 1), PAIRS, replace=False)
    return k // (H - 1), k % (H - 1)


def _check(m, allc, bar=BAR):
    return check_steps(m, allc["states"], allc["actions"], m["timestep"], m["integrator"], bar, pairs=_pairs())


def _check_frame(m, state, frame):
    """mjpc_hip_get_frame (the handed-in state) against the reference's forward kinematics, 1e-13 relative; mocap bodies and their
    sites left out (the reference does not see the mocap poses).  Also the world's row of subtree_linvel (total momentum / total
    mass), which used to carry residual scratch"""
    ref = DynRef(m)
    q, v = _t(state[None, :m["nq"]]), _t(state[None, m["nq"]:m["nq"] + m["nv"]])
    f = ref.fk(q)
    com, lin = ref.subtree(q, v)
    body = np.asarray(m["body_mocapid"]) < 0
    site = body[np.asarray(m["site_bodyid"], int)]
    want = dict(xpos=f["xpos"][0].numpy()[body], xmat=f["xmat"][0].numpy().reshape(-1, 9)[body], site_xpos=f["site_xpos"][0].numpy()[site],
                subtree_com=com[0].numpy()[body], subtree_linvel=lin[0].numpy()[body])
    for k, w in want.items():
        got = frame[k][site] if k == "site_xpos" else frame[k][body]
        assert np.abs(got - w).max() <= 1e-13 * max(1.0, np.abs(w).max()), k


def _case(name):
    if name == "hand":
        name = "shadow_hand"
    return dc.registry_case(name)


# (case id, model, knobs, capacity, flavour expected): spill / dense (hot) / plain
CASES = [
    ("cached2_particle", "particle", (), None, "plain"),
    ("cached18_quadruped", "quadruped", (), None, "plain"),
    ("cached27_humanoid", "humanoid_track", (), None, "plain"),
    ("direct33_hand", "hand", (), None, "plain"),
    ("dense2h18_quadruped", "quadruped", (("tier", "B"),), None, "dense_hot"),
    ("dense2_27_humanoid", "humanoid_track", (("tier", "B"),), None, "dense"),
    ("dense2_33_hand", "hand", (("tier", "B"),), None, "dense"),
    ("spill27_knob", "humanoid_track", (("spill", "all"),), None, "spill"),
    ("spill33_knob", "hand", (("spill", "all"),), None, "spill"),
    ("spill27_capacity", "humanoid_track", (), (64, 192), "spill"),
    ("spill33_capacity", "hand", (), (64, 192), "spill"),
    ("no_model_cache_humanoid", "humanoid_track", (("no_model_cache", "1"),), None, "plain"),
    ("dense_factor_humanoid", "humanoid_track", (("dense_factor", "1"),), None, "plain"),
    ("generic9_walker", "walker", (), None, "plain"),
]


@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("cid, name, knobs, cap, flavour", CASES, ids=[c[0] for c in CASES])
def test_engine_steps_satisfy_the_reference_dynamics(cid, name, knobs, cap, flavour, integrator, debug_knobs):
    """Every case under each integrator: Euler's implicit-damping solve, implicitfast's M − h ∂τ/∂v and implicit's LU-solved
    M − h ∂(τ − c)/∂v (bias derivative in a scratch carved from the constraint rows, whose layout differs per flavour).  The knob
    cases show the knob took effect: no_model_cache runs with fewer LDS bytes than the engine without it (the model tables are not
    copied), dense_factor's rollouts differ in round-off from the elimination-tree order's (Euler and implicitfast: implicit's step
    is the dense LU solve either way, and without constraints M's own factor is not used).  The engine builds no dense tier under
    implicit (host.h: the dense integrator path has no dense-tier layout): the dense cases then assert that and check the
    full-capacity flavour."""
    m, task, state, mocap = _case(name)
    m["integrator"] = integrator
    if cap:
        m["nconmax"], m["nefcmax"] = cap
    if cid.startswith(("no_model_cache", "dense_factor")):
        plain_lds = _lds_bytes(m, task)
        plain, _, _ = _run(m, task, state, mocap, (), debug_knobs)
    allc, flav, frame = _run(m, task, state, mocap, knobs, debug_knobs)
    if flavour.startswith("dense") and integrator == 2:
        assert flav["dense_bytes"] == 0, flav
        flavour = "plain"
    assert flav["spill"] == (flavour == "spill"), flav
    assert flav["dense_used"] == flavour.startswith("dense"), flav
    if flavour.startswith("dense"):
        assert flav["dense_hot"] == (flavour == "dense_hot"), flav
    if cid.startswith("no_model_cache"):
        assert flav["lds"] < plain_lds, (flav["lds"], plain_lds)
    if cid.startswith("dense_factor") and integrator != 2:
        assert not np.array_equal(allc["states"], plain["states"])
    res = _check(m, allc)
    print(f"\n[dynamics-reference] {cid} integrator={integrator} nv={m['nv']} worst={res['worst']:.3e} pos={res['pos']:.1e}")
    _check_frame(m, state, frame)


@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("seed", (0, 4, 12, 14))
def test_engine_generic_nv_random_models(seed, integrator, debug_knobs):
    """generic NVT=0 kernels: random models with nv outside {2, 18, 27, 33} (seed 4: 40 dofs), under each integrator"""
    m, task, state, mocap = dc.random_case(seed)
    m["integrator"] = integrator
    assert m["nv"] not in (2, 18, 27, 33)
    allc, flav, frame = _run(m, task, state, mocap, (), debug_knobs)
    assert not flav["spill"]
    res = _check(m, allc)
    print(f"\n[dynamics-reference] random{seed} integrator={integrator} nv={m['nv']} worst={res['worst']:.3e}")
    _check_frame(m, state, frame)


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_engine_generic_spill_refused_seed(integrator, debug_knobs):
    """generic spill flavour: the first random seed whose layout does not fit LDS at 32 contacts / 128 rows, under each integrator"""
    from spill_common import refused_seeds
    seed = refused_seeds(1)[0]
    m, task, state, mocap = dc.random_case(seed)
    m["integrator"] = integrator
    m["nconmax"], m["nefcmax"] = 32, 128
    allc, flav, frame = _run(m, task, state, mocap, (), debug_knobs)
    assert flav["spill"]
    res = _check(m, allc)
    print(f"\n[dynamics-reference] spill_generic seed={seed} integrator={integrator} nv={m['nv']} worst={res['worst']:.3e}")
    _check_frame(m, state, frame)


@pytest.mark.parametrize("mutate", ["mass", "frame"])
def test_engine_negative_controls(mutate, debug_knobs):
    """the engine steps a humanoid whose mid-tree body mass / inertia is off by 1e-6 relative, or whose free root's inertial frame is
    turned by 1e-6 rad; the reference keeps the true model: the check exceeds the bar by 100× or more"""
    m, task, state, mocap = _case("humanoid_track")
    bad, body = (dc.mutate_mass if mutate == "mass" else dc.mutate_frame)(m)
    allc, _, _ = _run(bad, task, state, mocap, (), debug_knobs)
    res = _check(m, allc, bar=None)
    print(f"\n[dynamics-reference] negative {mutate} body={body} worst={res['worst']:.3e} margin={res['worst'] / BAR:.0f}x")
    assert res["worst"] >= 100 * BAR
