"""The pre-solve window of a step (csrc/core.h: ph_constraints on the owner wave beside ph_smooth, ph_inertia and ph_noncontact on the
other three) may be shared out differently among the four waves of a candidate; which wave computes a value never changes the
expression or its operands, so no bit of any result may move.  The fixture tests/golden/presolve_split/bits.npz holds the outputs of
the commit before the window was rebalanced (tools/record_presolve_bits.py, which also defines the cases, so recorder and test feed
the same inputs); returns, failure flags, the winner, the winner's states and every candidate's summed Newton iterations
(MISC_SUM_ITER) are compared as uint64 words.

Cases: the A1 dropped from 2 cm (steps with no contact, then touch-down), standing (8 contacts in its first 12 steps), pressed into
the floor (more than the headline's 14 contacts), with a contact buffer and with a row buffer too small (WARN_CONTACTFULL /
WARN_CNSTRFULL: the layout cuts ncon back), the pyramidal humanoid, a frictionless A1, the linkage (connect equalities), the filter
arm (activation states), the walker (generic-nv kernel), the spill flavour and the dense tier."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_presolve_bits", os.path.join(ROOT, "tools", "record_presolve_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

WARN_CONTACTFULL, WARN_CNSTRFULL = 8, 16


@pytest.fixture(scope="module")
def parent_bits():
    with np.load(rec.FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", rec.CASES, ids=[c[0] for c in rec.CASES])
def test_presolve_bits_equal_parent(case, parent_bits, debug_knobs):
    key, N, H = case[0], case[5], case[6]
    assert 4 <= N <= 8 and H <= 12
    got = rec.run_case(case, debug_knobs)
    diag = got["diag"]
    assert diag.shape == (N, 4)
    print(f"{key}: failure {got['failure'].tolist()} Newton iterations {diag[:, 0].tolist()} most contacts {diag[:, 1].tolist()} "
          f"most rows {diag[:, 2].tolist()} dense tier used {got['dense_used']}")
    for k in rec.KEYS:
        want = parent_bits[f"{key}_{k}"]
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, k
        print(f"{key} {k}: {int((got[k] != want).sum())} of {want.size} words differ")
    for k in rec.KEYS:
        assert np.array_equal(got[k], parent_bits[f"{key}_{k}"]), k
    # the run is the one the case is named after
    assert bool(got["dense_used"]) == (key == "a1_dense_tier")
    assert (got["spill_bytes"] > 0) == (key == "a1_spill")
    if key == "a1_contactfull":
        assert (got["failure"] & WARN_CONTACTFULL).any()
    elif key == "a1_cnstrfull":
        assert (got["failure"] & WARN_CNSTRFULL).any()
    else:
        assert not got["failure"].any()
    if key == "a1_drop":
        z = got["states"].view(np.float64)[..., 2].ravel()          # starts in the air, comes down and touches
        assert z.size == H and z[0] > 0.27 and z[-1] < z[0]
        assert (diag[:, 1] >= 1).all()
    if key in ("a1_stand", "a1_spill", "a1_dense_tier", "a1_frictionless"):
        assert (diag[:, 1] >= 4).all() and (diag[:, 0] >= 1).all()
    if key == "a1_pressed":
        assert (diag[:, 1] >= 14).all()
    if key == "a1_frictionless":
        assert (diag[:, 2] <= diag[:, 1] + 24).all()                 # one row per contact beside the friction-loss and limit rows
    if key in ("humanoid_pyramidal", "walker_generic_nv", "linkage_connect"):
        assert (diag[:, 2] >= 1).all()
