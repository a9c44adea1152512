"""Rollouts under a feedback policy on the CPU: the kernel source (csrc/feedback.h, feedback_resample.h) in the 1-lane emulation against
the host C++ iLQGPolicy::Action and the numpy mirror bit for bit, against the open-loop emulated rollout (K = 0, alpha = 0), and against a
closed loop over the independent C oracle."""
import ctypes as C

import numpy as np
import pytest

import emu_feedback_lib as ef
import feedback_cases as fc
import oracle_lib as ol
import oracle_loop_lib as oloop
import riccati_mirror as rm
from mujoco_mpc_amd import capi

CASES = [("particle", 8), ("filter_arm", 10), ("quadruped", 10)]
ALPHA = fc.STEPS
SCALE = fc.STEPS[::-1].copy()


def _run(c, pol, mode, rep=1, alpha=ALPHA, scale=SCALE, x0=None, use_feedback=True, improvement=True):
    return ef.plan_feedback(c["m"], c["task"], c["x0"] if x0 is None else x0, fc.T0, c["H"], pol["times"], pol["states"], pol["actions"], pol["K"],
                            alpha, scale, action_improvement=pol["k"] if improvement else None, mode=mode, representation=rep,
                            use_feedback=use_feedback, mocap=c["mocap"])


def _indexed(c):
    return dict(times=c["times"], states=c["xs"], actions=c["us"], K=c["K"], k=c["k"])


# ----------------------------------------------------------------------------- 1. action bits
def _check_bits(c, out, pol, mode, rep, alpha, scale, use_feedback=True, improvement=True):
    assert not out["failure"].any(), out["failure"]
    host, mirror, blas = fc.host_actions(c, out, pol, mode, rep, alpha, scale, use_feedback, improvement)
    got = out["actions"][:, :c["H"] - 1]
    db = np.abs(got - blas).max()
    print(c["name"], "mode", mode, "rep", rep, "max |kernel - host|", np.abs(got - host).max(), "|kernel - policy_action under the rule|", np.abs(got - mirror).max(),
          "|kernel - policy_action with numpy's product|", db)
    assert np.array_equal(got, host)
    # riccati_mirror.policy_action itself, its gain product and its atan2 under the summation rule (feedback_cases.summation_rule): every
    # case, nd = 36 included
    assert np.array_equal(got, mirror)
    # the same function with numpy's `@` (BLAS order and fusing, not the rule) and glibc's atan2: a last place off here and there
    # (measured: 0.0 on most cases, 1.7e-18 on the A1, 1.1e-16 with the x400 gains), inside the action bar of DESIGN 4
    assert db <= 1e-14 * max(1.0, np.abs(blas).max())


@pytest.mark.parametrize("name,H", CASES)
def test_action_bits_indexed(name, H):
    """ActionRollouts' form: tables indexed by the step, every candidate its own alpha and feedback scale, start off the nominal"""
    c = fc.case(name, H)
    pol = _indexed(c)
    x0 = fc.displaced(c)
    out = _run(c, pol, capi.FEEDBACK_INDEXED, x0=x0)
    assert np.abs(out["states"][:, 1:] - c["xs"][None, 1:]).max() > 0
    _check_bits(c, out, pol, 0, 0, ALPHA, SCALE)
    assert not np.array_equal(out["actions"][0], out["actions"][3])          # the candidates differ


@pytest.mark.parametrize("name,H", CASES)
@pytest.mark.parametrize("rep", [0, 1, 2])
def test_action_bits_time_interpolated(name, H, rep):
    """FeedbackRollouts' form: alpha = 0, the policy on its own time grid interpolated at the step's time (zero / linear / cubic), steps
    before the first and after the last knot included; the resampled tables are read back and every entry was written"""
    c = fc.case(name, H)
    pol = fc.time_policy(c)
    alpha = np.zeros(4)
    out = _run(c, pol, capi.FEEDBACK_TIME, rep=rep, alpha=alpha, x0=fc.displaced(c))
    for k in ("xbar", "ubar", "kbar", "Kbar"):
        assert np.isfinite(out[k]).all(), k
    assert out["times"][0, 0] < pol["times"][0] and out["times"][0, -2] > pol["times"][-1]
    _check_bits(c, out, pol, 1, rep, alpha, SCALE)


@pytest.mark.parametrize("name,H", CASES[:2])
def test_action_bits_special_cases(name, H):
    """use_feedback = 0 skips the feedback term, action_improvement = NULL the alpha term: the host called without a state / with the plain
    actions gives the same bits, and the feedback-free candidates are all the same rollout"""
    c = fc.case(name, H)
    pol = _indexed(c)
    x0 = fc.displaced(c)
    out = _run(c, pol, capi.FEEDBACK_INDEXED, x0=x0, use_feedback=False)
    _check_bits(c, out, pol, 0, 0, ALPHA, SCALE, use_feedback=False)
    out = _run(c, pol, capi.FEEDBACK_INDEXED, x0=x0, improvement=False)
    _check_bits(c, out, pol, 0, 0, ALPHA, SCALE, improvement=False)
    out = _run(c, pol, capi.FEEDBACK_INDEXED, x0=x0, use_feedback=False, improvement=False)
    assert all(np.array_equal(out["states"][0], out["states"][i]) for i in range(1, 4))
    tp = fc.time_policy(c)
    out = _run(c, tp, capi.FEEDBACK_TIME, rep=1, alpha=np.zeros(4), x0=x0, use_feedback=False, improvement=False)
    _check_bits(c, out, tp, 1, 1, np.zeros(4), SCALE, use_feedback=False, improvement=False)


def test_clamp_is_active_and_last():
    """gains large enough to saturate: some control of some step sits on its bound, and the bits are still the host's (clamp last, once)"""
    c = fc.case("particle", 8)
    pol = _indexed(c); pol = dict(pol, K=pol["K"] * 400.0)
    out = _run(c, pol, capi.FEEDBACK_INDEXED, x0=fc.displaced(c, scale=4.0))
    a = out["actions"][:, :c["H"] - 1]
    on_bound = (a == c["cr"][:, 0]) | (a == c["cr"][:, 1])
    assert on_bound.any() and not on_bound.all()
    _check_bits(c, out, pol, 0, 0, ALPHA, SCALE)


# ----------------------------------------------------------------------------- 2. open-loop anchor
@pytest.mark.parametrize("name,H", CASES)
def test_open_loop_anchor(name, H):
    """K = 0, alpha = 0, indexed tables from the nominal rollout: the emulated open-loop rollout with P = H zero-order knots at the same
    times, bit for bit (states, actions, residuals, costs, returns)"""
    c = fc.case(name, H)
    pol = dict(_indexed(c), K=np.zeros_like(c["K"]))
    out = _run(c, pol, capi.FEEDBACK_INDEXED, alpha=np.zeros(2), scale=np.ones(2))
    nom = c["nominal"]
    for i in range(2):
        assert out["failure"][i] == 0
        for k in ("states", "times", "residual", "costs"):
            assert np.array_equal(out[k][i], nom[k][0]), k
        assert np.array_equal(out["actions"][i, :H - 1], nom["actions"][0, :H - 1])
        assert out["returns"][i] == nom["returns"][0]


# ----------------------------------------------------------------------------- 3. independent physics: a closed loop over the oracle
def _oracle_loop(c, pol, alpha, scale, x0):
    o = ol.Oracle(c["m"], c["task"])
    acts = pol["actions"] + pol["k"] * alpha

    def policy(t, time, x):
        return rm.policy_action(c["m"], c["times"], pol["states"], acts, pol["K"], time, x, 0, feedback_scaling=scale)
    return oloop.closed_loop(o, x0, fc.T0, c["H"], policy, mocap=c["mocap"])


def _bar(c):
    return 1e-5 if c["name"] == "quadruped" else 1e-9          # with contacts (relative) / contact-free


@pytest.mark.parametrize("name,H", CASES)
def test_against_oracle_closed_loop(name, H):
    c = fc.case(name, H)
    pol = _indexed(c)
    x0 = fc.displaced(c)
    out = _run(c, pol, capi.FEEDBACK_INDEXED, x0=x0)
    if name == "quadruped":
        # precondition of the contact bar, for every candidate compared below: the oracle loop reproduces itself from a start moved by one ulp
        x1 = x0.copy(); x1[2] = np.nextafter(x1[2], np.inf)
        for i in range(4):
            a = _oracle_loop(c, pol, ALPHA[i], SCALE[i], x0); b = _oracle_loop(c, pol, ALPHA[i], SCALE[i], x1)
            self_err = np.abs(a["states"] - b["states"]).max()
            print("oracle self-reproduction under one ulp, candidate", i, ":", self_err)
            assert self_err <= 1e-6, (i, self_err)
    for i in range(4):
        ref = _oracle_loop(c, pol, ALPHA[i], SCALE[i], x0)
        assert ref["failure"] == 0 and out["failure"][i] == 0
        for k in ("states", "actions", "residual", "costs"):
            g = out[k][i] if k != "actions" else out[k][i, :H - 1]
            r = ref[k] if k != "actions" else ref[k][:H - 1]
            scale_ = max(1.0, np.abs(r).max()) if name == "quadruped" else 1.0
            err = np.abs(g - r).max() / scale_
            print(name, "candidate", i, k, err)
            assert err <= _bar(c), (i, k, err)
        assert abs(out["returns"][i] - ref["ret"]) <= _bar(c) * max(1.0, abs(ref["ret"]))
    # the feedback matters: candidates with different scales end in different states
    assert np.abs(out["states"][0, -1] - out["states"][3, -1]).max() > 1e-6


# ----------------------------------------------------------------------------- 4. sizes
def test_sizeof_feedback_policy():
    lib = capi.load_engine()          # checks every sizeof at load, the new struct's among them
    assert lib.mjpc_hip_sizeof_feedback_policy() == C.sizeof(capi.MjpcHipFeedbackPolicy)
    assert "mjpc_hip_plan_feedback" in capi.EXPORTED_SYMBOLS and "mjpc_hip_sizeof_feedback_policy" in capi.EXPORTED_SYMBOLS


# ----------------------------------------------------------------------------- 5. the shared atan2
def test_atan2_cr_matches_the_high_precision_fixture():
    """csrc/atan2_cr.h against tests/golden/atan2_cr.json (tests/golden/make_atan2_fixture.py: the double nearest to atan2(y, x) from 300-bit
    arithmetic): small rotations (the usual argument of the quaternion tangent), general arguments in all of y >= 0, wide magnitudes and eight
    arguments that glibc's atan2 rounds the other way; then the special values.  With mpmath at hand the expected values are recomputed too."""
    import json
    import math
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "atan2_cr.json")) as f:
        fx = json.load(f)
    assert len(fx["points"]) >= 2000 and fx["hard"] == 8
    pts = [tuple(float.fromhex(v) for v in row) for row in fx["points"]]
    for y, x, want in pts:
        assert ef.atan2_cr(y, x) == want, (y.hex(), x.hex())
    for y, x in ((0.0, 1.0), (0.0, -1.0), (1.0, 0.0), (0.0, 0.0)):
        assert ef.atan2_cr(y, x) == math.atan2(y, x)
    try:
        import mpmath as mp
    except ImportError:
        return
    mp.mp.prec = 300
    for y, x, want in pts[::7] + pts[-8:]:
        assert float(mp.atan2(mp.mpf(y), mp.mpf(x))) == want


def test_candidate_offset_selects_the_tail_of_the_batch():
    """candidate_offset = 2 of a batch of 4: the engine's rows are candidates 2 and 3 of the whole batch, steps indexed globally"""
    c = fc.case("particle", 8)
    pol = _indexed(c)
    x0 = fc.displaced(c)
    full = _run(c, pol, capi.FEEDBACK_INDEXED, x0=x0)
    tail = ef.plan_feedback(c["m"], c["task"], x0, fc.T0, c["H"], pol["times"], pol["states"], pol["actions"], pol["K"], ALPHA, SCALE,
                            action_improvement=pol["k"], mode=capi.FEEDBACK_INDEXED, mocap=c["mocap"], candidate_offset=2)
    assert tail["states"].shape[0] == 2
    for k in ("states", "actions", "residual", "costs", "returns"):
        assert np.array_equal(tail[k], full[k][2:]), k
