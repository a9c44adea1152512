"""GPU tier of the direct optimiser's window cost (mjpc_hip_direct_assemble): the CPU tier's cases (tests/test_direct_cost.py) through
HipBackend with the bars measured there between the emulation and the references (tests/direct_cases.py; none derived from device
output), the device against the host mirror bit for bit, repeatability, a window of many more blocks than one launch's first, and the
refusals of the C ABI.  The engine lends its device and stream only, so one small engine (a 3-hinge chain) serves every case."""
import ctypes as C

import numpy as np
import pytest

import direct_cases as dc
import emu_direct_lib as ed
import inverse_cases as ic
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.planner import HipBackend
from test_direct_cost import check_algebra, check_model, check_window, direction, host

pytestmark = pytest.mark.gpu
NAMES = list(dc.CASES)


@pytest.fixture(scope="module")
def be():
    c = ic.case(dc.MODEL)
    b = HipBackend(c["model"], c["task"], max_samples=4, max_horizon=2)
    yield b
    b.close()


def device(be, c, **override):
    return be.direct_assemble(dc.settings(c["spec"], **override), *c["inputs"], fill=np.nan)


# ---------------------------------------------------------------------------------------------------------------- 1. reference bars
@pytest.mark.parametrize("name", NAMES)
def test_against_the_references(be, name):
    o = check_window(name, lambda c: device(be, c))
    check_algebra(name, lambda c: device(be, c))
    mine, reference = direction(name, o["gradient"])
    assert mine <= 10.0 * max(reference, dc.ULP)


@pytest.mark.parametrize("T", dc.MODEL_T)
def test_chain_window_from_device_inverse_derivatives(be, T):
    """the engine's own model: mjpc_hip_inverse_batch and mjpc_hip_inverse_fd feed mjpc_hip_direct_assemble, nothing from the CPU in between but
    the subtraction of the measurements"""
    mocap = ic.case(dc.MODEL)["mocap"]

    def evaluate(X, U, A, t):
        o = be.inverse_batch(X, U, A, t, mocap=mocap, discrete=False)
        assert not o["failure"].any()
        return o["qfrc_inverse"], o["residual"]
    check_model(T, evaluate, lambda X, U, A, t: be.inverse_fd(X, U, A, t, mocap=mocap, discrete=False, eps=dc.MODEL_FD_EPS),
                lambda s, *ins: be.direct_assemble(s, *ins, fill=np.nan))


# ---------------------------------------------------------------------------------------------------------------- 2. device against host
@pytest.mark.parametrize("name", NAMES)
def test_device_gives_the_host_mirrors_bits(be, name):
    for c in (dc.case(name), dc.algebra_case(name)):
        h = host(c["spec"])
        od, oh = h.assemble(be, *c["inputs"]), h.assemble_host(*c["inputs"])
        raw = device(be, c)
        for k in ed.OUTPUTS:
            assert np.array_equal(od[k], oh[k]), k
            assert np.array_equal(raw[k], oh[k]), k


def test_a_long_window_gives_the_host_mirrors_bits(be):
    """T = 200 on 3 dofs: 600 band rows, the entry kernels' grids of several hundred workgroups, every interior block overlapping two others"""
    sp = dc.spec("nv3_T5")
    T = 200
    sp.mask = np.ones((T, len(sp.dim)), int); sp.mask[::7, 2] = 0
    w = dc.dr.Window(sp, T, seed=9)
    rs, rf, Df, Ds, V0, V1 = w.inputs()
    ins = (rs, rf, *Df, *Ds, V0, V1)
    od, oh = be.direct_assemble(dc.settings(sp), *ins, fill=np.nan), host(sp).assemble_host(*ins)
    for k in ed.OUTPUTS:
        assert np.array_equal(od[k], oh[k]), k


# ---------------------------------------------------------------------------------------------------------------- 3. repeatability
def test_two_calls_give_the_same_bits(be):
    c = dc.algebra_case("nv18_T4")
    a, b = device(be, c), device(be, c)
    assert all(np.array_equal(a[k], b[k]) for k in ed.OUTPUTS)


def test_a_masked_sensor_changes_nothing(be):
    c = dc.case("nv3_T5")
    sp = c["spec"]
    base = device(be, c)
    rs = c["inputs"][0].copy(); rs[1, sp.first[1]:sp.first[1] + sp.dim[1]] += 1.0e6
    moved = device(be, dict(c, inputs=(rs,) + c["inputs"][1:]))
    for k in ("cost", "gradient", "hessian_band", "block_sensor", "block_force"):
        assert np.array_equal(base[k], moved[k]), k


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_of_the_c_abi(be):
    c = dc.case("nv3_T3")
    sp, ins = c["spec"], c["inputs"]

    def refused(what, settings=None, arrays=ins):
        with pytest.raises(RuntimeError, match=what):
            be.direct_assemble(settings if settings is not None else dc.settings(sp), *arrays)
    refused("T < 3", arrays=[a[:2] for a in ins])
    s = dc.settings(sp); s.struct_size -= 4
    refused("struct_size", s)
    kw = dict(sensor_dim=sp.dim, sensor_stage=sp.stage, sensor_norm=sp.norm_type, sensor_norm_parameter=sp.prm, noise_sensor=sp.noise_sensor,
              noise_process=sp.noise_process, timestep=sp.h, sensor_first_row=sp.first_row)
    bad = lambda **over: capi.direct_settings(**{**kw, **over})      # noqa: E731
    refused("sensor noise value <= 0", bad(noise_sensor=[1.0, 0.0, 1.0, 1.0]))
    refused("process noise value <= 0", bad(noise_process=[1.0, -1.0, 1.0]))
    refused("outside the residual", bad(sensor_first_row=sp.nr - sp.ns + 1))
    refused("outside the residual", bad(sensor_first_row=-1))
    refused("stage outside", bad(sensor_stage=[0, 1, 3, 0]))
    refused("timestep <= 0", bad(timestep=0.0))
    s = bad(); s.num_sensor_rows += 1
    refused("do not sum", s, arrays=[np.zeros((3, sp.ns + 1))] + list(ins[1:]))
    s = bad(); s.noise_process = None
    refused("null input", s)
    # a null required array, straight through the C ABI; the outputs keep what they held
    s = dc.settings(sp)
    out = np.full(3, 7.0); g = np.full(9, 7.0); band = np.full((9, 9), 7.0)
    dp = capi.c_double_p
    args = [np.ascontiguousarray(a, dtype=np.float64) for a in ins]
    ptrs = [a.ctypes.data_as(dp) for a in args]
    ptrs[9] = None          # dvdq1
    rc = be.lib.mjpc_hip_direct_assemble(be.h, 3, sp.nv, sp.nr, C.byref(s), *ptrs, out.ctypes.data_as(dp), g.ctypes.data_as(dp), band.ctypes.data_as(dp),
                                         *[None] * 6)
    assert rc == -1 and b"null input" in be.lib.mjpc_hip_last_error()
    assert np.all(out == 7.0) and np.all(g == 7.0) and np.all(band == 7.0)
    # the engine still works
    assert np.isfinite(device(be, c)["cost"]).all()


# ---------------------------------------------------------------------------------------------------------------- the window calls
from test_direct_cost import check_rows      # noqa: E402

WINDOWS = list(dc.WINDOW_MODELS)


def window_backend(c, max_samples=64):
    return HipBackend(c["model"], c["task"], max_samples=max_samples, max_horizon=2)


def derivatives(b, c, Q=None, **kw):
    kw.setdefault("centered", c.get("centered", False))
    return b.direct_cost_derivatives(dc.settings(c["spec"]), c["Q"] if Q is None else Q, None, c["U"], c["time"], c["y_sensor"], c["y_force"], mocap=c["mocap"],
                                     eps=dc.MODEL_FD_EPS, fill=np.nan, **kw)


def value(b, c, Q, **kw):
    return b.direct_cost(dc.settings(c["spec"]), Q, None, c["U"], c["time"], c["y_sensor"], c["y_force"], mocap=c["mocap"], fill=np.nan, **kw)


@pytest.mark.parametrize("name", WINDOWS)
def test_fused_window_call_equals_its_stages_one_by_one(name):
    """mjpc_hip_direct_cost_derivatives against: the window's rows and velocity blocks (reference bars, and the emulation's bits), then
    mjpc_hip_inverse_batch and mjpc_hip_inverse_fd on those rows with everything downloaded, then mjpc_hip_direct_assemble: bit for bit.  And
    the value call gives the derivative call's costs, velocities and accelerations."""
    c = dc.window_case(name)
    m, T = c["model"], c["T"]
    nq, nv, sp = m["nq"], m["nv"], c["spec"]
    b = window_backend(c)
    o = derivatives(b, c)
    assert not o["failure"].any(), o["failure"]
    v = value(b, c, c["Q"])
    rows = ed.window(m, c["Q"], ctrl=c["U"], time=c["time"])
    X, A = rows["x"][0], rows["a"][0]
    assert np.array_equal(v["velocity"][0], X[:, nq:nq + nv]) and np.array_equal(v["acceleration"][0], A)
    assert np.array_equal(o["dvdq0"], rows["dvdq0"]) and np.array_equal(o["dvdq1"], rows["dvdq1"])
    check_rows(name, v["velocity"][0], v["acceleration"][0], o["dvdq0"], o["dvdq1"])
    ev = b.inverse_batch(X, c["U"], A, c["time"], mocap=c["mocap"], discrete=True)
    fd = b.inverse_fd(X, c["U"], A, c["time"], mocap=c["mocap"], discrete=True, eps=dc.MODEL_FD_EPS)
    assert np.array_equal(v["force_prediction"][0], ev["qfrc_inverse"]) and np.array_equal(v["sensor_prediction"][0], ev["residual"][:, sp.first_row:sp.first_row + sp.ns])
    for k in ("DfDq", "DfDv", "DfDa", "DsDq", "DsDv", "DsDa"):
        assert np.array_equal(o[k], fd[k]), k
    rs = ev["residual"][:, sp.first_row:sp.first_row + sp.ns] - c["y_sensor"][:, :sp.ns]
    a = b.direct_assemble(dc.settings(sp), rs, ev["qfrc_inverse"] - c["y_force"], *[fd[k] for k in ("DfDq", "DfDv", "DfDa", "DsDq", "DsDv", "DsDa")], o["dvdq0"], o["dvdq1"])
    for k in ed.OUTPUTS:
        assert np.array_equal(o[k], a[k]), k
    assert np.array_equal(v["cost"][0], o["cost"]) and np.isfinite(o["hessian_band"]).all() and o["cost"][0] > 0
    if name == "quadruped_elliptic":          # a contact force above 1 N somewhere in the window
        assert np.abs(ev["qfrc_constraint"]).max() > 1.0
    b.close()


@pytest.mark.parametrize("name", WINDOWS)
def test_three_windows_in_one_call_equal_three_calls(name):
    c = dc.window_case(name)
    m = c["model"]
    rng = np.random.default_rng(5)
    Q3 = np.stack([c["Q"]] + [np.stack([dc.dr.integrate_pos(m, q, 1e-3 * rng.standard_normal(m["nv"])) for q in c["Q"]]) for _ in range(2)])
    b = window_backend(c)
    o3 = value(b, c, Q3)
    for w in range(3):
        o1 = value(b, c, Q3[w])
        for k in o3:
            assert np.array_equal(o3[k][w], o1[k][0]), (w, k)
    assert len({o3["cost"][w, 0] for w in range(3)}) == 3
    # two identical calls
    again = derivatives(b, c); once = derivatives(b, c)
    assert all(np.array_equal(again[k], once[k]) for k in again)
    b.close()


def test_launch_boundary():
    """an engine of four workgroups per launch (40 launches of the inverse kernel for the chain's window) gives one launch's bits"""
    c = dc.window_case("chain3_euler")
    big, small = window_backend(c), window_backend(c, max_samples=4)
    a, b_ = derivatives(big, c), derivatives(small, c)
    assert all(np.array_equal(a[k], b_[k]) for k in a)
    Q3 = np.stack([c["Q"], c["Q"][::-1], c["Q"]])
    va, vb = value(big, c, Q3), value(small, c, Q3)
    assert all(np.array_equal(va[k], vb[k]) for k in va)
    big.close(); small.close()


def test_a_nan_configuration_sets_failure_and_the_call_returns():
    c = dc.window_case("chain3_euler")
    T = 5
    c5 = dc.window_case("chain3_euler", T)
    Q = c5["Q"].copy(); Q[3, 0] = np.nan
    b = window_backend(c5)
    o = derivatives(b, c5, Q=Q)
    v = value(b, c5, Q)
    # configuration 3 feeds the velocities of 3 and 4 and the accelerations of 2 and 3
    assert o["failure"][2:].all() and v["failure"][0, 2:].all() and not o["failure"][:2].any() and not v["failure"][0, :2].any()
    clean = derivatives(b, c5)
    assert not clean["failure"].any() and np.isfinite(clean["gradient"]).all()
    b.close()


def test_window_call_refusals():
    c = dc.window_case("chain3_euler")
    b = window_backend(c, max_samples=4)
    s = dc.settings(c["spec"])
    args = (None, c["U"], c["time"], c["y_sensor"], c["y_force"])
    with pytest.raises(RuntimeError, match="fd_eps <= 0"):
        b.direct_cost_derivatives(s, c["Q"], *args, eps=0.0)
    with pytest.raises(RuntimeError, match="T < 3"):
        b.direct_cost_derivatives(s, c["Q"][:2], None, c["U"][:2], c["time"][:2], c["y_sensor"][:2], c["y_force"][:2])
    with pytest.raises(RuntimeError, match="T < 3"):
        b.direct_cost(s, c["Q"][:2], None, c["U"][:2], c["time"][:2], c["y_sensor"][:2], c["y_force"][:2])
    bad = dc.settings(c["spec"]); bad.struct_size += 8
    for call in (b.direct_cost, b.direct_cost_derivatives):
        with pytest.raises(RuntimeError, match="struct_size"):
            call(bad, c["Q"], *args)
    bad = dc.settings(c["spec"]); bad.sensor_first_row = 1
    with pytest.raises(RuntimeError, match="outside the residual"):
        b.direct_cost(bad, c["Q"], *args)
    sp = c["spec"]
    bad = capi.direct_settings(sp.dim, sp.stage, sp.norm_type, sp.prm, np.zeros(len(sp.dim)), sp.noise_process, sp.h)
    with pytest.raises(RuntimeError, match="noise value <= 0"):
        b.direct_cost_derivatives(bad, c["Q"], *args)
    dp = capi.c_double_p
    cost = np.full(3, 7.0)
    q = np.ascontiguousarray(c["Q"])
    rc = b.lib.mjpc_hip_direct_cost(b.h, 0, 4, C.byref(s), 1, q.ctypes.data_as(dp), *[None] * 7, cost.ctypes.data_as(dp), *[None] * 5)
    assert rc == -1 and b"nwin < 1" in b.lib.mjpc_hip_last_error() and np.all(cost == 7.0)
    rc = b.lib.mjpc_hip_direct_cost(b.h, 1, 4, C.byref(s), 1, None, *[None] * 7, cost.ctypes.data_as(dp), *[None] * 5)
    assert rc == -1 and b"null input" in b.lib.mjpc_hip_last_error() and np.all(cost == 7.0)
    assert np.isfinite(b.direct_cost(s, c["Q"], *args)["cost"]).all()
    b.close()
    # discrete != 0 on a dense implicit integrator, exactly as mjpc_hip_inverse_fd refuses it
    from mujoco_mpc_amd.modelgen import REGISTRY
    m, task, d = REGISTRY["swimmer"]()
    sw = HipBackend(m, task, max_samples=4, max_horizon=2)
    nr, nv = task["num_residual"], m["nv"]
    s = capi.direct_settings([nr], [2], [0], [[0.0, 0.0]], [1.0], np.ones(nv), float(m["timestep"]))
    Q = np.tile(np.asarray(d["state"], float)[:m["nq"]], (3, 1))
    mocap = d["mocap"] if len(d["mocap"]) else None
    for call in (sw.direct_cost, sw.direct_cost_derivatives):
        with pytest.raises(RuntimeError, match="dense implicit integrator"):
            call(s, Q, None, None, np.zeros(3), np.zeros((3, nr)), np.zeros((3, nv)), mocap=mocap, discrete=True)
    assert np.isfinite(sw.direct_cost(s, Q, None, None, np.zeros(3), np.zeros((3, nr)), np.zeros((3, nv)), mocap=mocap, discrete=False)["cost"]).all()
    sw.close()


def test_directcost_object_owns_the_window():
    """mjpc_hip::DirectCost::Cost / CostDerivatives through the C view give the bits of the two C-ABI calls; a mask shorter than the window is
    refused"""
    from mujoco_mpc_amd import cplanner
    c = dc.window_case("sphere")
    sp, m = c["spec"], c["model"]
    b = window_backend(c)
    h = host(sp)
    h.set_window(m, c["Q"], ctrl=c["U"], time=c["time"], sensor_measurement=c["y_sensor"], force_measurement=c["y_force"], tol=dc.MODEL_FD_EPS)
    o, ref = h.cost_derivatives(b, mocap=c["mocap"]), derivatives(b, c)
    for k in ed.OUTPUTS:
        assert np.array_equal(o[k], ref[k]), k
    Q3 = np.stack([c["Q"], c["Q"][::-1], c["Q"]])
    assert np.array_equal(h.cost(b, Q3, mocap=c["mocap"])["cost"], value(b, c, Q3)["cost"])
    assert np.array_equal(h.cost(b, mocap=c["mocap"])["cost"][0], ref["cost"])
    short = host(sp); short.lib.mjpc_dc_set_mask(short.h, np.ones(len(sp.dim), np.int32).ctypes.data_as(capi.c_int_p), 1)
    short.set_window(m, c["Q"])
    with pytest.raises(cplanner.PlannerError, match="mask"):
        short.cost_derivatives(b)
    b.close()


@pytest.mark.parametrize("name", list(dc.REF_WINDOWS))
def test_model_windows_against_whole_window_references(name):
    """mjpc_hip_direct_cost_derivatives on the free sphere, the two balls and the A1 against J_ref, g_ref, H_ref of the whole window (stored
    fixtures) with the CPU-measured bars, and the directional quotient; continuous inverse dynamics, as the reference's"""
    from test_direct_cost import check_reference_window
    b = window_backend(dc.ref_case(name))
    o = check_reference_window(name, lambda c: derivatives(b, c, discrete=False))
    assert not o["failure"].any()
    c = dc.ref_case(name)
    v = value(b, c, c["Q"], discrete=False)
    assert np.array_equal(v["cost"][0], o["cost"])
    b.close()
