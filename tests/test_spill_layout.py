"""CPU tier of the spill flavour (rollout_spill.hip: the row- and contact-sized blocks of a candidate's state in an HBM slab when
the state does not fit 160 KiB of LDS): the host-only flavour query, and the kernel source in its 1-lane emulation built like the
spill flavour (tests/emu/emu_spill.cpp) against today's emulation and against the oracle."""
import ctypes as C

import numpy as np
import pytest

import emu_lib
import emu_spill_lib as es
import oracle_lib as ol
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.modelgen import REGISTRY, cartpole, humanoid_track, quadruped, shadow_hand
from random_models import random_model
from spill_common import LDS_LIMIT, chosen_layout, plain_layout, refused_seeds, with_capacity


@pytest.mark.parametrize("make", [cartpole, quadruped, humanoid_track, shadow_hand])
def test_models_that_fit_keep_their_flavour(make):
    m, task, _ = make()
    lds, slab, spill = chosen_layout(m, task)
    assert not spill and slab == 0 and lds == plain_layout(m, task)


def test_host_only_queries_refuse_a_view_of_the_wrong_struct_size():
    """mjpc_hip_layout_bytes and mjpc_hip_debug_spill_layout read the views like mjpc_hip_create does: a model view whose struct_size
    is not the library's is refused by both before anything is read out of it; the unmodified view answers as it did"""
    lib = capi.load_engine()
    m, task, _ = quadruped()
    cm = capi.CModel(m, task)
    a = C.c_int(0); b = C.c_int(0)

    def ask():
        rc = lib.mjpc_hip_debug_spill_layout(C.byref(cm.c_model), C.byref(cm.c_task), C.byref(a), C.byref(b))
        return [lib.mjpc_hip_layout_bytes(C.byref(cm.c_model), C.byref(cm.c_task), u) for u in (0, 1, 2)] + [rc, a.value, b.value]
    good = ask()
    assert min(good[:3]) > 0 and good[3:] == [0, plain_layout(m, task), 0] and good[4] == chosen_layout(m, task)[0]
    cm.c_model.struct_size -= 8
    for u in (0, 1, 2):
        assert lib.mjpc_hip_layout_bytes(C.byref(cm.c_model), C.byref(cm.c_task), u) < 0
        assert b"mjpc_hip_layout_bytes" in lib.mjpc_hip_last_error() and b"struct_size" in lib.mjpc_hip_last_error()
    assert lib.mjpc_hip_debug_spill_layout(C.byref(cm.c_model), C.byref(cm.c_task), C.byref(a), C.byref(b)) < 0
    assert b"mjpc_hip_debug_spill_layout" in lib.mjpc_hip_last_error() and b"struct_size" in lib.mjpc_hip_last_error()
    cm.c_model.struct_size += 8
    cm.c_task.struct_size -= 8
    assert lib.mjpc_hip_layout_bytes(C.byref(cm.c_model), C.byref(cm.c_task), 1) < 0 and b"struct_size" in lib.mjpc_hip_last_error()
    cm.c_task.struct_size += 8
    assert ask() == good


@pytest.mark.parametrize("capacity", [(32, 128), (64, 192)])
def test_spill_exactly_where_the_plain_layout_is_refused(capacity):
    models = [with_capacity(humanoid_track(), 64, 192), with_capacity(shadow_hand(), 64, 192)] if capacity == (64, 192) else []
    models += [with_capacity(random_model(s), *capacity) for s in range(300)]
    nspill = 0
    for m, task, _ in models:
        plain = plain_layout(m, task)
        if plain < 0:                            # refused by build() for another reason
            continue
        got = chosen_layout(m, task)
        assert got is not None
        lds, slab, spill = got
        assert lds <= LDS_LIMIT and slab % 256 == 0
        assert spill == (plain > LDS_LIMIT)          # the spill flavour exactly where the engine refused the model before
        if not spill:
            assert slab == 0 and lds == plain
        elif slab == 0:
            # (a few 27- / 33-dof models: the spill flavour's compile-time-nv layout has no scaled-row table and fits as it is)
            assert m["nv"] in (27, 33)
        nspill += slab > 0
    assert nspill >= (55 if capacity == (32, 128) else 200)      # the tier is no corner case at these capacities


def _inputs(m, P, H, N, seed=0):
    kt = np.linspace(0, (H - 1) * m["timestep"], P); kv = np.random.default_rng(seed).uniform(-0.3, 0.3, (P, m["nu"]))
    eps, sel = ol.noise(1, 0, 0, N, P, m["nu"])
    return kt, kv, eps, sel


def _same(a, b):
    for k in ("knots", "failure", "states", "actions", "times", "residual", "costs", "trace", "returns", "diag"):
        assert np.array_equal(a[k], b[k]), k


EMU_REGISTRY = ["particle", "cartpole", "quadruped", "walker", "acrobot", "quadruped_hill", "terrain_balls", "cylinder_pile",
                "particle_timevarying", "particle_fixed", "swimmer", "quadrotor", "linkage", "welded", "fingers", "fingers_grasp",
                "site_servo", "noslip_elliptic3", "noslip_elliptic4", "noslip_elliptic6", "noslip_pyramidal3", "noslip_pyramidal6",
                "servo_arm", "filter_arm", "ball_chain", "humanoid_track", "humanoid_stand", "humanoid_walk", "humanoid_interact"]


@pytest.mark.parametrize("name", EMU_REGISTRY)
def test_all_spilled_emulation_is_bit_identical_registry(name):
    """every eligible block in the slab (NaN-poisoned per candidate) against today's in-LDS emulation: a block whose pointer
    was not re-based reads poison or another candidate's data"""
    m, task, d = REGISTRY[name]()
    P, H, N = 3, 24, 3
    kt, kv, eps, sel = _inputs(m, P, H, N)
    mocap = d["mocap"] if len(d["mocap"]) else None
    a = emu_lib.plan(m, task, d["state"], mocap, 0.0, kt, kv, 2, N, H, sigma=(0.3, 0.0), noise_eps=eps, noise_sel=sel)
    b = es.plan(m, task, d["state"], mocap, 0.0, kt, kv, 2, N, H, sigma=(0.3, 0.0), noise_eps=eps, noise_sel=sel, mode=es.SPILL_ALL)
    assert b["slab_doubles"] > 0
    _same(a, b)


@pytest.mark.parametrize("seed,portal", [(s, p) for p in (False, True) for s in range(24)])
def test_all_spilled_emulation_is_bit_identical_random(seed, portal):
    m, task, d = random_model(seed, portal)
    P, H, N = 4, 24, 3
    kt, kv, eps, sel = _inputs(m, P, H, N, 1000 + seed)
    a = emu_lib.plan(m, task, d["state"], None, 0.0, kt, kv, 2, N, H, sigma=(0.3, 0.0), noise_eps=eps, noise_sel=sel)
    b = es.plan(m, task, d["state"], None, 0.0, kt, kv, 2, N, H, sigma=(0.3, 0.0), noise_eps=eps, noise_sel=sel, mode=es.SPILL_ALL)
    _same(a, b)


def _oracle_cases():
    cases = [("humanoid_track", lambda: with_capacity(humanoid_track(), 64, 192)), ("shadow_hand", lambda: with_capacity(shadow_hand(), 64, 192))]
    return cases + [(f"seed{s}", lambda s=s: with_capacity(random_model(s), 32, 128)) for s in refused_seeds(4)]


@pytest.mark.parametrize("name,make", _oracle_cases())
def test_spill_emulation_matches_oracle(name, make):
    """models refused before the spill tier, on the automatic spill layout, against the oracle at the usual bar"""
    m, task, d = make()
    P, H, N = 4, 30, 4
    kt, kv, eps, sel = _inputs(m, P, H, N)
    mocap = d["mocap"] if len(d["mocap"]) else None
    a = ol.Oracle(m, task).plan(d["state"], mocap, 0.0, kt, kv, 2, N, H, sigma=(0.15, 0.0), noise_eps=eps, noise_sel=sel, nthreads=4)
    b = es.plan(m, task, d["state"], mocap, 0.0, kt, kv, 2, N, H, sigma=(0.15, 0.0), noise_eps=eps, noise_sel=sel, mode=es.SPILL_AUTO)
    assert b["slab_doubles"] > 0 and b["lds_doubles"] * 8 <= LDS_LIMIT
    assert np.array_equal(a["knots"], b["knots"]) and np.array_equal(a["failure"], b["failure"])
    for k in ("states", "residual", "costs", "trace", "returns"):
        if a[k].size:
            assert np.abs(b[k] - a[k]).max() / (np.abs(a[k]).max() + 1e-300) < 1e-5, k
    assert int(np.argmin(b["returns"])) == a["winner"]
