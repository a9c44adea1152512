"""The register L^T D L of csrc/linalg.h broadcasts pivots with a 64-bit row DPP move where every consumer lane sits in the
pivot's 16-lane row, and with v_readlane otherwise.  Lanes of other rows then see a different value than before, always times an
exact zero, so no bit of any result may move.  The fixture tests/golden/row_broadcast/bits.npz holds the outputs of the commit
before the change (tools/record_ldl_bits.py, which also defines the cases, so recorder and test feed the same inputs); everything
is compared as uint64.

Shapes: n = 18 has exactly two pivots whose ancestors sit across the row boundary, 27 splits a leg across rows, 33 spans three
rows with the hub link; tree = 0 is the dense elimination order, tree = 1 the level order on matrices with the model's pattern."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_ldl_bits", os.path.join(ROOT, "tools", "record_ldl_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def parent_bits():
    with np.load(rec.FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("tree", [0, 1])
@pytest.mark.parametrize("n", rec.LDL_NS)
def test_ldl_hook_bits_equal_parent(n, tree, parent_bits):
    """fused and split factor + solve of 8 seeded SPD systems through the hook library (mjpc_hip_debug_ldl)"""
    got = rec.run_ldl(rec.load_hooks(), n, tree, rec.dof_parents(n))
    want = parent_bits[f"ldl_{n}_{tree}"]
    assert want.dtype == np.uint64 and want.shape == (rec.LDL_SEEDS, 2 * n)
    # the recorded solutions solve the systems (the fixture belongs to these inputs)
    for seed in range(rec.LDL_SEEDS):
        A, b = rec.ldl_system(n, tree, seed, rec.dof_parents(n))
        assert np.allclose(want[seed].view(np.float64)[:n], np.linalg.solve(A, b), rtol=1e-12, atol=1e-13)
    print(f"n={n} tree={tree}: {int((got != want).sum())} of {want.size} words differ")
    assert np.array_equal(got, want)


@pytest.mark.parametrize("case", rec.ROLLOUT_CASES, ids=[c[0] for c in rec.ROLLOUT_CASES])
def test_rollout_bits_equal_parent(case, parent_bits, debug_knobs):
    """returns, failure flags and the winner's states of a small plan on every kernel family that calls the register L^T D L
    (one per CU, two per CU, dense elimination order, 27 and 33 dofs), and the LU path of the implicit integrator"""
    got, dense_used = rec.run_rollout(case, debug_knobs)
    key = case[0]
    assert dense_used == (key == "quadruped_dense_tier")
    for k in ("returns", "failure", "states", "winner"):
        want = parent_bits[f"rollout_{key}_{k}"]
        assert got[k].dtype == want.dtype and got[k].shape == want.shape
        print(f"{key} {k}: {int((got[k] != want).sum())} of {want.size} words differ")
    for k in ("returns", "failure", "states", "winner"):
        assert np.array_equal(got[k], parent_bits[f"rollout_{key}_{k}"]), k
    assert not got["failure"].any()
