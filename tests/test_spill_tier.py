"""GPU tier of the spill flavour (rollout_spill.hip): models whose per-candidate state exceeds 160 KiB of LDS run with their
row- and contact-sized blocks in a per-candidate HBM slab instead of being refused.  Against the oracle, and bit for bit against
the in-LDS kernel of the same compile-time nv with every eligible block forced into the slab (knob "spill" = "all")."""
import numpy as np
import pytest

import oracle_lib as ol
from mujoco_mpc_amd.modelgen import REGISTRY, humanoid_track, quadruped, shadow_hand
from random_models import random_model
from spill_common import LDS_LIMIT, chosen_layout, refused_seeds, with_capacity
from test_random_models import _check, _oracle_is_reproducible, _plan_inputs

pytestmark = pytest.mark.gpu

TRAJ = ("states", "actions", "times", "residual", "costs", "trace", "knots")


def _plan(m, task, d, N, H, P, sigma, seed=0x5EED, stream=3, state=None):
    from mujoco_mpc_amd.planner import HipBackend
    kt = np.linspace(0, (H - 1) * m["timestep"], P); kv = np.zeros((P, m["nu"]))
    be = HipBackend(m, task, max_samples=N, max_horizon=H)
    try:
        out = be.plan(state=d["state"] if state is None else state, mocap=d["mocap"] if len(d["mocap"]) else None, time=0.0,
                      knot_times=kt, knot_values=kv, interpolation=2, num_trajectory=N, horizon=H, sigma=(sigma, 0.0), seed=seed, stream=stream)
        return out, be.fetch_all(N, H, P), be.lds_bytes(), be.spill_bytes()
    finally:
        be.close()


def _identical(a, b):
    assert np.array_equal(a[0]["returns"], b[0]["returns"]) and np.array_equal(a[0]["failure"], b[0]["failure"])
    assert a[0]["winner"] == b[0]["winner"]
    for k in TRAJ:
        assert np.array_equal(a[1][k], b[1][k]), k


@pytest.mark.parametrize("make", [humanoid_track, shadow_hand])
def test_models_refused_before_now_plan_and_match_the_oracle(make):
    from mujoco_mpc_amd.planner import HipBackend
    m, task, d = with_capacity(make(), 64, 192)
    be = HipBackend(m, task, max_samples=64, max_horizon=30)          # raised "exceeds 160 KiB" before the spill tier
    assert be.lds_bytes() <= LDS_LIMIT and be.spill_bytes() > 0
    be.close()
    N, H, P = 64, 30 if make is humanoid_track else 24, 4
    kt = np.linspace(0, (H - 1) * m["timestep"], P); kv = np.random.default_rng(0).uniform(-0.2, 0.2, (P, m["nu"]))
    eps, sel = ol.noise(7, 0, 0, N, P, m["nu"])
    mocap = d["mocap"] if len(d["mocap"]) else None
    a = ol.Oracle(m, task).plan(d["state"], mocap, 0.0, kt, kv, 2, N, H, sigma=(0.1, 0.0), noise_eps=eps, noise_sel=sel, nthreads=8)
    be = HipBackend(m, task, max_samples=N, max_horizon=H)
    out = be.plan(state=d["state"], mocap=mocap, time=0.0, knot_times=kt, knot_values=kv, interpolation=2, num_trajectory=N,
                  horizon=H, sigma=(0.1, 0.0), noise_eps=eps, noise_sel=sel)
    b = be.fetch_all(N, H, P)
    be.close()
    b["returns"] = out["returns"]; b["failure"] = out["failure"]
    _check(a, b)
    assert out["winner"] == a["winner"]


@pytest.mark.parametrize("case", ["quadruped", "shadow_hand", "fingers"])
def test_forced_spill_is_bit_identical_to_the_in_lds_kernel(case, debug_knobs):
    """quadruped: generic kernels (no_model_cache = the direct flavour); shadow_hand 32/128: direct<33> against spill<33>;
    fingers: its noslip table moves to the slab too"""
    if case == "quadruped":
        m, task, d = quadruped(); ref = {"no_model_cache": "1"}
    elif case == "shadow_hand":
        m, task, d = shadow_hand(); ref = {}
    else:
        m, task, d = REGISTRY["fingers"](); ref = {}
    N, H, P, sigma = (64, 40, 3, 0.3)
    res = {}
    for name, env in (("lds", ref), ("spill", {"spill": "all"})):
        for k in ("no_model_cache", "spill"):
            debug_knobs(k, None)
        for k, v in env.items():
            debug_knobs(k, v)
        res[name] = _plan(m, task, d, N, H, P, sigma)
    assert res["lds"][3] == 0 and res["spill"][3] > 0 and res["spill"][2] < res["lds"][2]
    if case != "fingers":
        assert res["lds"][1]["diag"][:, 2].max() > 0                 # constraint rows were in use
    _identical(res["lds"], res["spill"])


def test_capacity_tiers_over_the_spill_flavour_are_bit_identical(debug_knobs):
    """more candidates than CUs: the dense tier runs first and its overflow resumes on the spill kernel (the same compile-time
    nv); full capacity only, automatic and a tiny dense tier (most candidates retried) agree bit for bit"""
    m, task, d = with_capacity(humanoid_track(), 64, 192)
    N, H, P = 300, 40, 6
    res = {}
    for name, env in (("full", {"tier": "A"}), ("auto", {}), ("tiny", {"dense_tier_cap": "24,8"})):
        for k in ("tier", "dense_tier_cap"):
            debug_knobs(k, None)
        for k, v in env.items():
            debug_knobs(k, v)
        res[name] = _plan(m, task, d, N, H, P, 0.15)
        assert res[name][3] > 0
    assert not res["full"][0]["failure"].any()
    assert res["full"][1]["diag"][:, 2].max() > 24                   # rows per step exceed the tiny tier: its candidates were retried
    for name in ("auto", "tiny"):
        _identical(res["full"], res[name])


def test_fuzz_models_refused_before_match_the_oracle():
    from mujoco_mpc_amd.planner import HipBackend
    seeds = refused_seeds(8)
    assert len(seeds) == 8
    for seed in seeds:
        m, task, d = with_capacity(random_model(seed), 32, 128)
        assert chosen_layout(m, task)[2]
        P, H, N, kt, kv, eps, sel = _plan_inputs(m, seed)
        a = ol.Oracle(m, task).plan(d["state"], None, 0.0, kt, kv, 2, N, H, sigma=(0.3, 0.0), noise_eps=eps, noise_sel=sel, nthreads=8)
        be = HipBackend(m, task, max_samples=N, max_horizon=H)
        out = be.plan(state=d["state"], mocap=None, time=0.0, knot_times=kt, knot_values=kv, interpolation=2, num_trajectory=N, horizon=H,
                      sigma=(0.3, 0.0), noise_eps=eps, noise_sel=sel)
        b = be.fetch_all(N, H, P)
        b["returns"] = out["returns"]; b["failure"] = out["failure"]
        be.close()
        if _oracle_is_reproducible(m, task, d, a, kt, kv, N, H, eps, sel, nthreads=8):
            _check(a, b)
            assert out["winner"] == a["winner"], seed
        else:                                    # (the oracle differs from itself by more than 1e-6: test_random_models' loose bar)
            _check(a, b, 1e-2, 20)
            assert np.array_equal(a["failure"], b["failure"])


def test_no_state_leaks_through_the_slab():
    """plan A, plan B from another state, plan A again on one engine: the two A plans are bit-identical; and a two-engine
    HipMultiBackend on device 0 equals one engine"""
    from mujoco_mpc_amd.planner import HipBackend, HipMultiBackend
    m, task, d = with_capacity(humanoid_track(), 64, 192)
    N, H, P = 64, 30, 4
    kt = np.linspace(0, (H - 1) * m["timestep"], P); kv = np.zeros((P, m["nu"]))
    other = d["state"].copy(); other[m["nq"]:m["nq"] + m["nv"]] += 0.5
    kw = dict(mocap=d["mocap"], time=0.0, knot_times=kt, knot_values=kv, interpolation=2, num_trajectory=N, horizon=H, sigma=(0.15, 0.0),
              seed=11, stream=0)
    be = HipBackend(m, task, max_samples=N, max_horizon=H)
    assert be.spill_bytes() > 0
    a1 = be.plan(state=d["state"], **kw); f1 = be.fetch_all(N, H, P)
    b = be.plan(state=other, **kw)
    a2 = be.plan(state=d["state"], **kw); f2 = be.fetch_all(N, H, P)
    be.close()
    assert not np.array_equal(a1["returns"], b["returns"])
    _identical((a1, f1), (a2, f2))
    mb = HipMultiBackend(m, task, [0, 0], max_samples=N, max_horizon=H)
    mo = mb.plan(state=d["state"], **kw)
    mc = mb.candidate(mo["winner"], H, P)
    mb.close()
    assert np.array_equal(mo["returns"], a1["returns"]) and mo["winner"] == a1["winner"]
    assert np.array_equal(mc["states"].reshape(f1["states"][a1["winner"]].shape), f1["states"][a1["winner"]])
