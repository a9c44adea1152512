"""GPU tier of the inverse dynamics (mjpc_hip_inverse_batch, mjpc_hip_inverse_fd): the CPU tier's cases (tests/test_inverse.py) through
HipBackend with the bars measured there between the emulation and the references (tests/inverse_cases.py; none derived from device
output), the A1 on the direct and the spill flavour, the humanoid that only fits with its rows in HBM, a batch across a launch boundary,
repeatability, and the refusals of the C ABI.

Kernels: the particle (nv = 2) and the A1 (nv = 18) run compile-time-nv instantiations of the cached flavour, the chains (nv = 3), the
sphere and the two-ball body (nv = 6) and the arm its generic <0> kernel; the A1 on the direct flavour that flavour's <0> kernel, the
humanoid (nv = 27) the spill flavour's <27>.

The zoo of con_cases (nv = 31, two site transmissions) runs the generic kernel as well."""
import ctypes as C

import numpy as np
import pytest

import inv_ref as ir
import inverse_cases as ic
from mujoco_mpc_amd.planner import HipBackend
from test_inverse import continuous_vs_discrete, measure_fd, measure_reference, measure_roundtrip, measure_zoo, nan_row, particle_numpy_loop

pytestmark = pytest.mark.gpu


def backend(c, max_samples=64):
    return HipBackend(c["model"], c["task"], max_samples=max_samples, max_horizon=2)


def device_run(c, X, U, A, T, discrete, max_samples=64):
    be = backend(c, max_samples)
    o = be.inverse_batch(X, U, A, T, mocap=c["mocap"], discrete=discrete)
    be.close()
    return o["qfrc_inverse"], o["qfrc_constraint"], o["residual"], o["failure"]


def device_step(c):
    be = backend(c)
    o = be.step_batch(c["X"], c["U"], c["T"], mocap=c["mocap"])
    be.close()
    assert not o["failure"].any()
    return o["next_states"]


def device_fd(c, rows, centered):
    be = backend(c)
    o = be.inverse_fd(c["X"][rows], c["U"][rows], c["A"][rows], c["T"][rows], mocap=c["mocap"], eps=ic.FD_EPS, centered=centered, fill=np.nan)
    be.close()
    return o


# ---------------------------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize("name", ic.CASES)
def test_against_reference(name):
    force, res = measure_reference(name, device_run)
    print("bars", ic.bar(ic.FORCE_MEASURED, name), ic.bar(ic.RESIDUAL_MEASURED, name))
    assert force <= ic.bar(ic.FORCE_MEASURED, name) and res <= ic.bar(ic.RESIDUAL_MEASURED, name)


@pytest.mark.parametrize("knob,value", [("no_model_cache", "1"), ("spill", "all")])
def test_a1_on_the_direct_and_spill_flavours(debug_knobs, knob, value):
    """the engine forced onto the flavour that reads the tables from HBM (its generic-nv kernel: 18 is not in its list), and onto the one
    that keeps the constraint rows, contacts and efc_force in the HBM slab"""
    debug_knobs(knob, value)
    name = "quadruped_elliptic"
    c = ic.case(name)
    be = backend(c); n = C.c_int(0)
    assert (be.lib.mjpc_hip_debug_spill(be.h, C.byref(n)) == 1) == (knob == "spill")
    be.close()
    force, res = measure_reference(name, device_run)
    assert force <= ic.bar(ic.FORCE_MEASURED, name) and res <= ic.bar(ic.RESIDUAL_MEASURED, name)


def test_humanoid_that_needs_the_spill_flavour():
    """the humanoid at 64 contacts / 192 rows does not fit 160 KiB of LDS (tests/spill_common.py): constraint rows and contacts in the
    slab, compile-time nv = 27.  Forces against inv_ref at the low-standing state of con_cases; the bar is ten times the emulation's
    deviation there (HUMANOID_SPILL_MEASURED, tests/test_inverse.py::test_humanoid_spill_model_in_emulation)"""
    from test_inverse import humanoid_spill_case
    c, w = humanoid_spill_case()
    be = backend(c, 8); n = C.c_int(0)
    assert be.lib.mjpc_hip_debug_spill(be.h, C.byref(n)) == 1
    o = be.inverse_batch(c["X"], c["U"], c["A"], c["T"], mocap=c["mocap"])
    be.close()
    assert not o["failure"].any() and (w["ncon"] > 0).all() and w["fmax"].max() > 1.0
    d = max(ir.dev(o["qfrc_inverse"], w["qfrc_inverse"]), ir.dev(o["qfrc_constraint"], w["qfrc_constraint"]))
    print("humanoid on the spill flavour: forces", d, "bar", 10 * ic.HUMANOID_SPILL_MEASURED)
    assert d <= 10 * ic.HUMANOID_SPILL_MEASURED


def test_particle_forces_equal_the_numpy_loop_bit_for_bit():
    particle_numpy_loop(device_run)


def test_site_transmissions_on_the_zoo():
    assert measure_zoo(device_run) <= 10 * ic.ZOO_MEASURED


# ---------------------------------------------------------------------------------------------------------------- 2. round trip
@pytest.mark.parametrize("name", ic.CASES)
def test_round_trip(name):
    assert measure_roundtrip(name, device_step, device_run) <= ic.bar(ic.ROUNDTRIP_MEASURED, name)


def test_continuous_acceleration_and_the_flag():
    def step_res(c):
        be = backend(c)
        o = be.step_batch(c["X"], c["U"], c["T"], mocap=c["mocap"])
        be.close()
        return o["next_states"], o["residual"]
    d0, d1 = continuous_vs_discrete(step_res, device_run)
    assert d0 <= ic.bar(ic.ROUNDTRIP_MEASURED, ic.DAMPED)
    assert d1 > 1000 * ic.bar(ic.ROUNDTRIP_MEASURED, ic.DAMPED)


# ---------------------------------------------------------------------------------------------------------------- 3. FD blocks
FD_GPU = [(n, cen) for n in ic.CASES for cen in (False, True)]


@pytest.mark.parametrize("name,centered", FD_GPU, ids=[f"{n}-{'centred' if cen else 'onesided'}" for n, cen in FD_GPU])
def test_fd_blocks(name, centered):
    worst, dm, di = measure_fd(name, centered, device_fd)
    assert worst <= ic.bar(ic.FD_MEASURED, name)
    if not ic.case(name)["contact"]:
        assert dm <= ic.bar(ic.FD_MASS_MEASURED, name) and di <= ic.bar(ic.FD_MASS_MEASURED, name)


def test_fd_three_configurations_null_blocks_and_launch_boundaries():
    """T = 3 in one call (30 evaluations) against the references and against three calls at T = 1; the same through an engine that
    launches 4 workgroups at a time; blocks that are not asked for stay untouched"""
    c = ic.case("chain3_euler")
    worst, _, _ = measure_fd("chain3_euler", False, device_fd, T=3)
    assert worst <= ic.bar(ic.FD_MEASURED, "chain3_euler")
    kw = dict(mocap=c["mocap"], eps=ic.FD_EPS, centered=False)
    be = backend(c); small = backend(c, 4)
    o3 = be.inverse_fd(c["X"][1:4], c["U"][1:4], c["A"][1:4], c["T"][1:4], **kw)
    s3 = small.inverse_fd(c["X"][1:4], c["U"][1:4], c["A"][1:4], c["T"][1:4], **kw)
    part = be.inverse_fd(c["X"][1:4], c["U"][1:4], c["A"][1:4], c["T"][1:4], want=(0, 1, 0, 1, 0, 0), **kw)
    for t in range(3):
        o1 = be.inverse_fd(c["X"][1 + t:2 + t], c["U"][1 + t:2 + t], c["A"][1 + t:2 + t], c["T"][1 + t:2 + t], **kw)
        assert all(np.array_equal(o3[k][t], o1[k][0]) for k in ic.BLOCKS), t
    assert all(np.array_equal(o3[k], s3[k]) for k in ic.BLOCKS)
    assert part["DfDq"] is None and part["DsDa"] is None and np.array_equal(part["DfDv"], o3["DfDv"]) and np.array_equal(part["DsDq"], o3["DsDq"])
    be.close(); small.close()


# ---------------------------------------------------------------------------------------------------------------- 4. errors and failures
def test_discrete_refused_on_dense_implicit_model_outputs_untouched():
    from mujoco_mpc_amd.modelgen import REGISTRY
    m, task, d = REGISTRY["swimmer"]()
    be = HipBackend(m, task, max_samples=4, max_horizon=2)
    x = np.asarray(d["state"], float)[None]; u = np.zeros((1, m["nu"])); a = np.zeros((1, m["nv"]))
    mocap = d["mocap"] if len(d["mocap"]) else None
    with pytest.raises(RuntimeError, match="dense implicit integrator"):
        be.inverse_batch(x, u, a, [0.0], mocap=mocap, discrete=True)
    with pytest.raises(RuntimeError, match="dense implicit integrator"):
        be.inverse_fd(x, u, a, [0.0], mocap=mocap, discrete=True)
    # the same refusal straight through the C ABI: outputs keep what they held
    dp = C.POINTER(C.c_double)
    f = np.full((1, m["nv"]), 7.0); fc = np.full((1, m["nv"]), 7.0); r = np.full((1, max(task["num_residual"], 1)), 7.0); fl = np.full(1, 7, np.int32)
    t = np.zeros(1); mo = np.zeros(max(7 * m["nmocap"], 1))
    rc = be.lib.mjpc_hip_inverse_batch(be.h, 1, x.ctypes.data_as(dp), u.ctypes.data_as(dp), a.ctypes.data_as(dp), t.ctypes.data_as(dp), mo.ctypes.data_as(dp),
                                       None, 1, f.ctypes.data_as(dp), fc.ctypes.data_as(dp), r.ctypes.data_as(dp), fl.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc != 0 and (f == 7).all() and (fc == 7).all() and (r == 7).all() and fl[0] == 7
    o = be.inverse_batch(x, u, a, [0.0], mocap=mocap)                # discrete = 0 works for every model
    assert not o["failure"].any() and np.isfinite(o["qfrc_inverse"]).all()
    be.close()


def test_nan_acceleration_fails_its_row_only():
    nan_row(device_run)


def test_calls_during_a_pending_plan_and_bad_arguments_are_refused():
    import transition_cases as tc
    m, task, mocap, X, U, T = tc.batch("particle", n=3)
    A = np.zeros((3, m["nv"]))
    be = HipBackend(m, task, max_samples=4, max_horizon=4)
    kt = np.array([0.0, 0.2]); kv = np.zeros((2, m["nu"]))
    kw = dict(state=X[0], mocap=mocap, time=0.0, knot_times=kt, knot_values=kv, interpolation=1, num_trajectory=4, horizon=4, sigma=(0.1, 0.0), seed=3)
    ref = be.plan(**kw)
    inp = be.make_input(**kw)
    be.plan_async(inp)
    with pytest.raises(RuntimeError, match="in flight"):
        be.inverse_batch(X, U, A, T, mocap=mocap)
    with pytest.raises(RuntimeError, match="in flight"):
        be.inverse_fd(X, U, A, T, mocap=mocap)
    got = be.plan_fetch(inp)
    assert np.array_equal(got["returns"], ref["returns"]) and got["winner"] == ref["winner"]
    for eps in (0.0, -1e-6):
        with pytest.raises(RuntimeError, match="eps"):
            be.inverse_fd(X, U, A, T, mocap=mocap, eps=eps)
    with pytest.raises(RuntimeError, match="n < 1"):
        be.inverse_batch(X[:0], U[:0], A[:0], T[:0], mocap=mocap)
    be.close()
    one = HipBackend(m, task, max_samples=4, max_horizon=1)
    with pytest.raises(RuntimeError, match="max_horizon"):
        one.inverse_batch(X, U, A, T, mocap=mocap)
    one.close()


# ---------------------------------------------------------------------------------------------------------------- launches, repeatability
def test_batch_across_a_launch_boundary_and_twice_the_same_bits():
    """the particle with max_local = 4: 11 rows are three launches; the rows are those of an engine that takes them in one, and a second
    call repeats the first bit for bit"""
    c = ic.case("particle_imu")
    idx = np.arange(11) % ic.ROWS
    A = np.vstack([c["A"], 0.5 * c["A"], -c["A"]])[:11]
    args = (c["X"][idx], c["U"][idx], A, c["T"][idx])
    small = backend(c, 4); big = backend(c, 64)
    a = small.inverse_batch(*args, mocap=c["mocap"]); b = big.inverse_batch(*args, mocap=c["mocap"]); a2 = small.inverse_batch(*args, mocap=c["mocap"])
    small.close(); big.close()
    assert not a["failure"].any() and len({r.tobytes() for r in a["qfrc_inverse"]}) == 9          # (rows 0, 5 and 10 are the row at rest: zero acceleration)
    assert all(np.array_equal(a[k], b[k]) and np.array_equal(a[k], a2[k]) for k in a)


def test_two_identical_calls_on_the_a1_are_bit_equal():
    c = ic.case("quadruped_elliptic")
    be = backend(c)
    a = be.inverse_batch(c["X"], c["U"], c["A"], c["T"], mocap=c["mocap"], discrete=True)
    b = be.inverse_batch(c["X"], c["U"], c["A"], c["T"], mocap=c["mocap"], discrete=True)
    be.close()
    assert all(np.array_equal(a[k], b[k]) for k in a) and np.isfinite(a["qfrc_inverse"]).all()


# ---------------------------------------------------------------------------------------------------------------- the window's ends
def test_inverse_derivatives_zeroes_the_ends_of_the_window():
    """T = 4 on the chain: the interior blocks are mjpc_hip_inverse_fd's; t = 0 is evaluated at v = a = 0 and keeps the position rows
    of DsDq only; t = 3 is evaluated at a = 0 and keeps DsDq and DsDv without their acceleration-stage rows"""
    from mujoco_mpc_amd.derivatives import InverseDerivatives
    c = ic.case("chain3_euler"); m = c["model"]; nq, nv = m["nq"], m["nv"]
    X, U, A, T = c["X"][:4], c["U"][:4], c["A"][:4], c["T"][:4]
    be = backend(c)
    idv = InverseDerivatives(m, c["task"], T=4)
    st = idv.row_stages()
    assert set(st) == {0, 1, 2}
    o = idv.compute(be, X, U, A, T, tol=ic.FD_EPS, mode=0, discrete=False, mocap=c["mocap"])
    Xe, Ae = X.copy(), A.copy(); Xe[0, nq:nq + nv] = 0; Ae[0] = 0; Ae[3] = 0
    d = be.inverse_fd(Xe, U, Ae, T, mocap=c["mocap"], eps=ic.FD_EPS)
    for k in ic.BLOCKS:
        assert np.array_equal(o[k][1:3], d[k][1:3]) and np.abs(o[k][1:3]).max() > 0, k
    for k in ("DfDq", "DfDv", "DfDa", "DsDa"):
        assert not o[k][0].any() and not o[k][3].any(), k
    assert not o["DsDv"][0].any()
    assert np.array_equal(o["DsDq"][0][st == 0], d["DsDq"][0][st == 0]) and o["DsDq"][0][st == 0].any() and not o["DsDq"][0][st > 0].any()
    for k in ("DsDq", "DsDv"):
        assert np.array_equal(o[k][3][st < 2], d[k][3][st < 2]) and not o[k][3][st == 2].any(), k
    assert o["DsDv"][3][st == 1].any() and d["DsDq"][3][st == 2].any()
    assert not o["failure"].any()
    one = idv.compute(be, X[:1], U[:1], A[:1], T[:1], tol=ic.FD_EPS, discrete=False, mocap=c["mocap"])       # a window of one configuration is a first one
    assert np.array_equal(one["DsDq"][0], o["DsDq"][0]) and not one["DsDv"].any()
    idv.close(); be.close()
