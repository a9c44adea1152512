"""The worker waves' cone-block job (csrc/solver_reg.h, worker_job) keeps what does not change between the Newton iterates of a step
- the item of the worker's first pass, its dofs and Jacobian columns - in registers instead of re-reading it from LDS in every job.
The sequence of ds_add_f64 instructions into a worker's partial and every operand of them stay what they were, so no bit of any
result may move.  The fixture tests/golden/cone_job/bits.npz holds the outputs of the commit before the change
(tools/record_cone_job_bits.py, which also defines the cases, so recorder and test feed the same inputs); returns, failure flags,
the winner and the winner's states are compared as uint64.

Cases: the elliptic hand (33 dofs, direct flavour, rows longer than the register cap), the fingers model with noslip off (18 dofs,
condim-6 and condim-3 contacts side by side), the A1 dropped from 4 cm (steps with nefc = 0, the first touch-down, iterates with and
without a contact in its cone zone: preloaded but never posted, and the release path) and the headline flavour three times in one
process.  The engine's diagnostics (summed Newton iterations, most contacts of a step) show that every candidate was in contact and
iterating.

What the recorded runs reach: the hand sees at most 2 contacts in its 6 steps (rows of 14 columns, but far fewer than 128 (contact,
row) pairs) and the dropped A1 at most 10, so neither gives a worker a second pass.  The case quadruped_pressed is there for that:
the A1 pushed 15 cm into the floor has 24 contacts, every one on at least the 6 dofs of the trunk."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_cone_job_bits", os.path.join(ROOT, "tools", "record_cone_job_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def parent_bits():
    with np.load(rec.FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", rec.CASES, ids=[c[0] for c in rec.CASES])
def test_cone_job_bits_equal_parent(case, parent_bits):
    key, N, H, plans = case[0], case[3], case[4], case[8]
    outs = rec.run_case(case)
    assert len(outs) == plans
    for n, got in enumerate(outs):
        for k in rec.KEYS:
            want = parent_bits[f"{key}_{k}"]
            assert got[k].dtype == want.dtype and got[k].shape == want.shape
            print(f"{key} plan {n} {k}: {int((got[k] != want).sum())} of {want.size} words differ")
        diag = got["diag"]
        print(f"{key} plan {n}: Newton iterations {diag[:, 0].tolist()} most contacts {diag[:, 1].tolist()} warnings {diag[:, 3].tolist()}")
        # every candidate touched something and its solver iterated (elliptic model: iterates with a cone-zone contact post the job)
        assert diag.shape == (N, 4)
        assert (diag[:, 1] >= 1).all() and (diag[:, 0] >= 1).all()
        assert not got["failure"].any()
        for k in rec.KEYS:
            assert np.array_equal(got[k], parent_bits[f"{key}_{k}"]), (n, k)
    if key == "quadruped_pressed":
        # >= 22 contacts x >= 6 dofs (every geom of the A1 hangs on the free joint) > 128 pairs: a second pass for worker 0
        assert (outs[0]["diag"][:, 1] >= 22).all()
    if key == "quadruped_drop":
        # the drop starts in the air (root height 0.26 + 0.04) and comes down: the first steps have no contact at all
        z = outs[0]["states"].view(np.float64)[..., 2].ravel()
        assert z.size == H and z[0] > 0.29 and z[-1] < z[0]
