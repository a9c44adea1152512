"""CPU tier of the direct optimiser's window cost (csrc/direct_cost.h, mjpc_hip_direct_assemble, mjpc_hip::DirectCost): the 1-lane emulation of
the five dc_* kernels and the host mirror DirectCost::AssembleHost against tests/direct_ref.py.

The references are independent of the code under test: direct_ref.Window differentiates a whole synthetic window by centred differences (no
chain rule in it), direct_ref.assemble is the algebra in numpy's matrix products.  The bars are ten times the deviation of the emulation
from them, measured here on the CPU (direct_cases.*_MEASURED), and are shared with the GPU tier."""
import numpy as np
import pytest

import direct_cases as dc
import direct_ref as dr
import emu_direct_lib as ed
from mujoco_mpc_amd import cplanner
from mujoco_mpc_amd import derivatives as D

NAMES = list(dc.CASES)


def emulated(c, **override):
    return ed.assemble(dc.settings(c["spec"], **override), *c["inputs"])


def host(sp, **override):
    flags = dict(sp.flags); flags.update(override)
    return D.DirectCost(sp.nv, sp.nr, sp.h, sp.dim, sp.stage, sp.norm_type, sp.prm, sp.noise_sensor, sp.noise_process, sp.first_row, sp.mask, **flags)


def check_window(name, run):
    """costs, gradient, band and blocks of run(case) against the whole-window reference; shared with the GPU tier"""
    c = dc.case(name)
    o = run(c)
    assert all(np.isfinite(v).all() for v in o.values()), "an output entry was never written"
    dev = dc.deviations(o, c["ref"], c["T"], c["nv"])
    print(name, "window", {k: f"{v:.1e}" for k, v in dev.items()})
    for k, v in dev.items():
        assert v <= dc.bar(dc.WINDOW_MEASURED, name, k), (k, v)
    return o


def check_algebra(name, run):
    c = dc.algebra_case(name)
    o = run(c)
    dev = dc.deviations(o, c["ref"], c["T"], c["nv"])
    print(name, "algebra", {k: f"{v:.1e}" for k, v in dev.items()})
    for k, v in dev.items():
        assert v <= dc.bar(dc.ALGEBRA_MEASURED, name, k), (k, v)
    return o


def direction(name, gradient):
    """(|g . d - quotient|, the same for the reference's gradient) for a seeded unit direction"""
    c = dc.case(name)
    w = c["window"]
    d = np.random.default_rng(77).normal(size=w.Q.shape); d /= np.linalg.norm(d)
    q = (w.cost(w.Q + dc.DIR_EPS * d)[0] - w.cost(w.Q - dc.DIR_EPS * d)[0]) / (2 * dc.DIR_EPS)
    return abs(gradient @ d.ravel() - q), abs(c["ref"]["gradient"] @ d.ravel() - q)


# ---------------------------------------------------------------------------------------------------------------- 1-3, 5. the references
@pytest.mark.parametrize("name", NAMES)
def test_costs_gradient_band_and_blocks_against_the_whole_window_reference(name):
    c = dc.case(name)
    o = check_window(name, emulated)
    T, nv, ref = c["T"], c["nv"], c["ref"]
    # the reference's Hessian has nothing outside the band, so the band is all of it
    assert dr.outside_band(ref["H"], 3 * nv) <= 1e-12 * np.abs(ref["H"]).max()
    # the band rows in front of the first full row: leading zeros, exactly
    for R in range(3 * nv - 1):
        assert np.all(o["hessian_band"][R, :3 * nv - 1 - R] == 0.0)
    # what the two ends drop is exactly zero: configuration 0 has its own columns alone and no velocity or acceleration row, the last
    # one no next configuration and no acceleration row, neither has a force block
    st = c["spec"].row_stage()
    bs, bf = o["block_sensor"], o["block_force"]
    assert np.all(bs[0][:, :nv] == 0.0) and np.all(bs[0][:, 2 * nv:] == 0.0) and np.all(bs[0][st != dr.POS] == 0.0) and np.any(bs[0][st == dr.POS] != 0.0)
    assert np.all(bs[T - 1][:, 2 * nv:] == 0.0) and np.all(bs[T - 1][st == dr.ACC] == 0.0) and np.any(bs[T - 1][st == dr.VEL][:, :nv] != 0.0)
    assert np.all(bf[0] == 0.0) and np.all(bf[T - 1] == 0.0) and np.all(bf[1:T - 1] != 0.0)
    assert np.array_equal(o["residual_sensor"], ref["residual_sensor"]) and np.array_equal(o["residual_force"], ref["residual_force"])


@pytest.mark.parametrize("name", NAMES)
def test_dense_velocity_blocks_against_numpy_products(name):
    check_algebra(name, lambda c: ed.assemble(dc.settings(c["spec"]), *c["inputs"]))


# ---------------------------------------------------------------------------------------------------------------- a real model
def emulated_model():
    """(evaluate, differentiate) of direct_ref.ModelWindow.inputs over the emulated inverse kernel and its finite differences"""
    import emu_inverse_lib as ei
    import inverse_cases as ic
    c = ic.case(dc.MODEL)
    m, task, mocap = c["model"], c["task"], c["mocap"]

    def evaluate(X, U, A, t):
        f, _, r, fail = ei.inverse_batch(m, task, X, U, A, t, mocap=mocap, discrete=False)
        assert not fail.any()
        return f, r
    return evaluate, lambda X, U, A, t: ei.inverse_fd(m, task, X, U, A, t, mocap=mocap, discrete=False, eps=dc.MODEL_FD_EPS)


def check_model(T, evaluate, differentiate, run):
    """inverse evaluations, their finite differences and the assemble of run(settings, *inputs) against the whole-window reference of the
    3-hinge chain (independent forces and rows, centred differences over the window); shared with the GPU tier"""
    c = dc.model_case(T)
    o = run(dc.settings(c["spec"]), *c["window"].inputs(evaluate, differentiate))
    dev = dc.deviations(o, c["ref"], T, c["nv"])
    print(c["name"], "model", {k: f"{v:.1e}" for k, v in dev.items()})
    for k, v in dev.items():
        assert v <= dc.bar(dc.MODEL_MEASURED, c["name"], k), (k, v)
    d = np.random.default_rng(78).normal(size=c["window"].Q.shape); d /= np.linalg.norm(d)
    w = c["window"]
    q = (w.cost(w.Q + dc.DIR_EPS * d)[0] - w.cost(w.Q - dc.DIR_EPS * d)[0]) / (2 * dc.DIR_EPS)
    mine, reference = abs(o["gradient"] @ d.ravel() - q), abs(c["ref"]["gradient"] @ d.ravel() - q)
    print(c["name"], "direction", f"{mine:.1e}", "reference's own", f"{reference:.1e}")
    assert mine <= 10.0 * max(reference, dc.ULP)
    return o


@pytest.mark.parametrize("T", dc.MODEL_T)
def test_chain_window_from_emulated_inverse_derivatives(T):
    check_model(T, *emulated_model(), ed.assemble)


# ---------------------------------------------------------------------------------------------------------------- 4. directional check
@pytest.mark.parametrize("name", NAMES)
def test_directional_derivative_of_the_whole_window_cost(name):
    mine, reference = direction(name, emulated(dc.case(name))["gradient"])
    print(name, "direction", f"{mine:.1e}", "reference's own", f"{reference:.1e}")
    # the bar: ten times the truncation error of the check itself, measured on the reference's own gradient against the same quotient
    assert mine <= 10.0 * max(reference, dc.ULP)


# ---------------------------------------------------------------------------------------------------------------- 6. host mirror
@pytest.mark.parametrize("name", NAMES)
def test_host_mirror_gives_the_emulations_bits(name):
    for c in (dc.case(name), dc.algebra_case(name)):
        o, oh = ed.assemble(dc.settings(c["spec"]), *c["inputs"]), host(c["spec"]).assemble_host(*c["inputs"])
        for k in ed.OUTPUTS:
            assert np.array_equal(o[k], oh[k]), k


def test_two_runs_give_the_same_bits():
    c = dc.algebra_case("nv7_T4")
    a, b = emulated(c), emulated(c)
    assert all(np.array_equal(a[k], b[k]) for k in ed.OUTPUTS)


# ---------------------------------------------------------------------------------------------------------------- 8. mask, flags
@pytest.mark.parametrize("run", ["emulation", "host"])
def test_a_masked_sensor_changes_nothing(run):
    c = dc.case("nv3_T5")
    sp = c["spec"]
    f = (lambda ins: emulated(dict(c, inputs=ins))) if run == "emulation" else (lambda ins: host(sp).assemble_host(*ins))
    base = f(c["inputs"])
    rs = c["inputs"][0].copy()
    sl = slice(sp.first[1], sp.first[1] + sp.dim[1])
    rs[1, sl] += 1.0e6          # the measurement of the masked pair (t = 1, sensor 1) moved by 1e6
    moved = f((rs,) + c["inputs"][1:])
    for k in ("cost", "gradient", "hessian_band", "block_sensor", "block_force"):
        assert np.array_equal(base[k], moved[k]), k
    # and the mask does something: with the pair switched on the cost is another
    on = np.ones_like(sp.mask)
    spec_on = dr.Spec(sp.nv, sp.nr, sp.h, sp.dim, sp.stage, sp.norm_type, sp.prm, sp.noise_sensor, sp.noise_process, sp.first_row, on, **sp.flags)
    assert ed.assemble(dc.settings(spec_on), *c["inputs"])["cost"][0] > base["cost"][0]


def test_flags_switch_the_two_terms_off():
    c = dc.case("nv3_T4")
    full, no_s, no_f = emulated(c), emulated(c, sensor_flag=False), emulated(c, force_flag=False)
    assert no_s["cost"][1] == 0.0 and no_s["cost"][0] == no_s["cost"][2] == full["cost"][2]
    assert no_f["cost"][2] == 0.0 and no_f["cost"][0] == no_f["cost"][1] == full["cost"][1]
    assert np.allclose(no_s["gradient"] + no_f["gradient"], full["gradient"], rtol=1e-13, atol=0)
    assert np.allclose(no_s["hessian_band"] + no_f["hessian_band"], full["hessian_band"], rtol=1e-13, atol=1e-300)


# ---------------------------------------------------------------------------------------------------------------- 9. refusals (host)
def test_host_refusals():
    c = dc.case("nv3_T3")
    sp, ins = c["spec"], c["inputs"]

    def refused(h, arrays, what):
        with pytest.raises(cplanner.PlannerError, match=what):
            h.assemble_host(*arrays)
    refused(host(sp), [a[:2] for a in ins], "T < 3")
    bad = lambda **kw: D.DirectCost(**{**dict(nv=sp.nv, nr=sp.nr, timestep=sp.h, sensor_dim=sp.dim, sensor_stage=sp.stage, sensor_norm=sp.norm_type,      # noqa: E731
                                              sensor_norm_parameter=sp.prm, noise_sensor=sp.noise_sensor, noise_process=sp.noise_process,
                                              sensor_first_row=sp.first_row), **kw})
    refused(bad(noise_sensor=[1.0, 0.0, 1.0, 1.0]), ins, "sensor noise")
    refused(bad(noise_process=[1.0, -1.0, 1.0]), ins, "process noise")
    refused(bad(sensor_first_row=sp.nr - sp.ns + 1), ins, "outside the residual")
    refused(bad(sensor_stage=[0, 1, 3, 0]), ins, "stage")
    refused(bad(timestep=0.0), ins, "timestep")


# ---------------------------------------------------------------------------------------------------------------- the window's rows
def check_rows(name, velocity, acceleration, dvdq0, dvdq1):
    """velocities, accelerations and velocity blocks of a window_case against numpy's differentiate_pos and its centred differences over tangent
    nudges; the ends' rules exactly; shared with the GPU tier"""
    c = dc.window_case(name)
    m, Q, T, h = c["model"], c["Q"], c["T"], c["spec"].h
    V = np.zeros((T, m["nv"])); A = np.zeros_like(V)
    for t in range(1, T):
        V[t] = dr.differentiate_pos(m, Q[t - 1], Q[t], h)
    A[1:T - 1] = (V[2:] - V[1:T - 1]) / h
    rel = lambda a, b: float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())      # noqa: E731
    dev = dict(velocity=rel(velocity, V), acceleration=rel(acceleration, A), blocks=0.0)
    for t in range(1, T):
        V0, V1 = dr.velocity_blocks(m, Q[t - 1], Q[t], h)
        dev["blocks"] = max(dev["blocks"], rel(dvdq0[t], V0), rel(dvdq1[t], V1))
    print(name, "rows", {k: f"{v:.1e}" for k, v in dev.items()})
    for k, v in dev.items():
        assert v <= dc.bar(dc.ROWS_MEASURED, name, k), (k, v)
    assert not velocity[0].any() and not acceleration[0].any() and not acceleration[T - 1].any() and not dvdq0[0].any() and not dvdq1[0].any()


@pytest.mark.parametrize("name", list(dc.WINDOW_MODELS))
def test_window_rows_and_velocity_blocks(name):
    c = dc.window_case(name)
    m = c["model"]
    nq, nv = m["nq"], m["nv"]
    o = ed.window(m, c["Q"], ctrl=c["U"], time=c["time"])
    assert np.array_equal(o["x"][0][:, :nq], c["Q"]) and np.array_equal(o["u"][0], c["U"]) and np.array_equal(o["time"][0], c["time"])
    check_rows(name, o["x"][0][:, nq:nq + nv], o["a"][0], o["dvdq0"], o["dvdq1"])
    if name == "sphere":          # the quaternion block is no scaled identity: the rotation between two configurations is about 0.3 rad
        assert np.abs(o["dvdq1"][1][3:, 3:] * c["spec"].h - np.eye(3)).max() > 1e-2
    # candidate windows in one call are the single windows' rows
    Q3 = np.stack([c["Q"], c["Q"][::-1], c["Q"]])
    o3 = ed.window(m, Q3, ctrl=c["U"], time=c["time"], blocks=False)
    assert np.array_equal(o3["x"][0], o["x"][0]) and np.array_equal(o3["a"][2], o["a"][0])
    assert np.array_equal(o3["x"][1], ed.window(m, c["Q"][::-1], ctrl=c["U"], time=c["time"], blocks=False)["x"][0])


def test_chain_window_uses_the_emulated_velocity_blocks():
    """on hinges the emulated blocks are the -1/h, 1/h the chain windows above are assembled with, bit for bit"""
    c = dc.model_case(4)
    o = ed.window(c["window"].case["model"], c["window"].Q)
    h, nv = c["spec"].h, c["nv"]
    for t in range(1, 4):
        assert np.array_equal(o["dvdq0"][t], -np.eye(nv) / h) and np.array_equal(o["dvdq1"][t], np.eye(nv) / h)
    X, A = c["window"].rows(c["window"].Q)
    assert np.array_equal(o["x"][0], X) and np.array_equal(o["a"][0], A)


# ---------------------------------------------------------------------------------------------------------------- the window calls, emulated
def emulated_derivatives(c, Q=None, discrete=False):
    """mjpc_hip_direct_cost_derivatives stage by stage in the emulation: dc_window_kernel and dc_vblock_kernel, the inverse kernel and its
    finite differences (tests/emu_inverse_lib.py), dc_residual_kernel, the five assemble kernels; plus the value call's tail on the same rows
    (cost_value) and the evaluations' constraint forces and warning bits"""
    import emu_inverse_lib as ei
    m, task, sp, T = c["model"], c["task"], c["spec"], c["T"]
    s = dc.settings(sp)
    rows = ed.window(m, c["Q"] if Q is None else Q, ctrl=c["U"], time=c["time"])
    X, A = rows["x"][0], rows["a"][0]
    f, fc, r, fail = ei.inverse_batch(m, task, X, c["U"], A, c["time"], mocap=c["mocap"], discrete=discrete)
    fd = ei.inverse_fd(m, task, X, c["U"], A, c["time"], mocap=c["mocap"], discrete=discrete, eps=dc.MODEL_FD_EPS, centered=c.get("centered", False))
    val = ed.value(s, T, sp.nv, r, f, c["y_sensor"], c["y_force"])
    o = ed.assemble(s, val["rs"][0], val["rf"][0], *[fd[k] for k in ("DfDq", "DfDv", "DfDa", "DsDq", "DsDv", "DsDa")], rows["dvdq0"], rows["dvdq1"])
    o.update(cost_value=val["cost"][0], failure=fail, qfrc_constraint=fc, rs=val["rs"][0], rf=val["rf"][0], residual=r, qfrc=f, dvdq1=rows["dvdq1"])
    return o


def check_reference_window(name, run):
    """run(case) -> the derivative call's outputs, against the stored whole-window reference of a model case: costs, gradient, band, blocks,
    the directional quotient; shared with the GPU tier"""
    c = dc.ref_case(name)
    o = run(c)
    T, nv, w = c["T"], c["nv"], c["window"]
    dev = dc.deviations(o, c["ref"], T, nv)
    print(name, "reference window", {k: f"{v:.1e}" for k, v in dev.items()})
    for k, v in dev.items():
        assert v <= dc.bar(dc.REF_MEASURED, name, k), (k, v)
    assert dr.outside_band(c["ref"]["H"], 3 * nv) <= 1e-12 * np.abs(c["ref"]["H"]).max()
    d = np.random.default_rng(79).normal(size=(T, nv)); d /= np.linalg.norm(d)
    q = (w.cost(w.plus(w.Q, dc.DIR_EPS * d))[0] - w.cost(w.plus(w.Q, -dc.DIR_EPS * d))[0]) / (2 * dc.DIR_EPS)
    mine, reference = abs(o["gradient"] @ d.ravel() - q), abs(c["ref"]["gradient"] @ d.ravel() - q)
    print(name, "direction", f"{mine:.1e}", "reference's own", f"{reference:.1e}")
    assert mine <= 10.0 * max(reference, dc.ULP)
    return o


@pytest.mark.parametrize("name", list(dc.REF_WINDOWS))
def test_model_windows_against_whole_window_references(name):
    """the free sphere (quaternion dofs), the two balls and the A1 (elliptic contacts): the emulated derivative call against J_ref, g_ref, H_ref
    of the whole window.  No state of the window, nor any nudged one, lies within 1e-9 of a contact margin: the reference's InvRef raises
    NearMargin otherwise, here for the window itself and at fixture time for every nudged evaluation."""
    o = check_reference_window(name, emulated_derivatives)
    c = dc.ref_case(name)
    c["window"].predictions(c["Q"])          # (NearMargin would be raised here)
    st = c["spec"].row_stage(); T, nv = c["T"], c["nv"]
    bs = o["block_sensor"]
    assert np.all(bs[0][st != dr.POS] == 0.0) and np.all(bs[0][:, :nv] == 0.0) and np.all(bs[T - 1][st == dr.ACC] == 0.0) and np.all(bs[T - 1][:, 2 * nv:] == 0.0)
    assert np.all(o["block_force"][0] == 0.0) and np.all(o["block_force"][T - 1] == 0.0)
    if c["name"] != "sphere":          # contacts: a constraint force above 1 N in the window
        assert np.abs(o["qfrc_constraint"]).max() > 1.0
    else:                              # and the sphere's quaternion blocks are no scaled identity
        assert np.abs(o["dvdq1"][1][3:, 3:] * c["spec"].h - np.eye(3)).max() > 1e-3


@pytest.mark.parametrize("name", list(dc.REF_WINDOWS) + ["chain3_euler"])
def test_derivative_call_is_its_stages_and_the_value_call_gives_its_costs(name):
    """6b and 7: the residual kernel is the subtraction of the measurements from the base evaluations (also out of a table with further
    slots per configuration), the derivative call's costs are the value call's bits, and three windows in one call are three calls"""
    import emu_inverse_lib as ei
    c = dc.ref_case(name) if name in dc.REF_WINDOWS else dc.window_case(name)
    m, task, sp, T = c["model"], c["task"], c["spec"], c["T"]
    o = emulated_derivatives(c)
    ys = c["y_sensor"][:, :sp.ns]
    assert np.array_equal(o["rs"], o["residual"][:, sp.first_row:sp.first_row + sp.ns] - ys) and np.array_equal(o["rf"], o["qfrc"] - c["y_force"])
    assert np.array_equal(o["cost_value"], o["cost"]) and not o["failure"].any()
    s = dc.settings(sp)
    E = 3          # the derivative call's table: E slots per configuration, the base first; the other slots are not to be read
    table_r = np.full((T, E, o["residual"].shape[1]), np.nan); table_r[:, 0] = o["residual"]
    table_f = np.full((T, E, sp.nv), np.nan); table_f[:, 0] = o["qfrc"]
    strided = ed.value(s, T, sp.nv, table_r.reshape(T * E, -1), table_f.reshape(T * E, -1), c["y_sensor"], c["y_force"], E=E)
    assert np.array_equal(strided["rs"][0], o["rs"]) and np.array_equal(strided["cost"][0], o["cost"])
    # three candidate windows
    rng = np.random.default_rng(6)
    Q3 = np.stack([c["Q"]] + [np.stack([dr.integrate_pos(m, q, 1e-4 * rng.standard_normal(sp.nv)) for q in c["Q"]]) for _ in range(2)])
    rows = ed.window(m, Q3, ctrl=c["U"], time=c["time"], blocks=False)
    X, A = rows["x"].reshape(3 * T, -1), rows["a"].reshape(3 * T, -1)
    f, _, r, fail = ei.inverse_batch(m, task, X, np.tile(c["U"], (3, 1)), A, np.tile(c["time"], 3), mocap=c["mocap"], discrete=False)
    three = ed.value(s, T, sp.nv, r, f, c["y_sensor"], c["y_force"])
    for w in range(3):
        one = ed.value(s, T, sp.nv, r[w * T:(w + 1) * T], f[w * T:(w + 1) * T], c["y_sensor"], c["y_force"])
        for k in three:
            assert np.array_equal(three[k][w], one[k][0]), (w, k)
    assert np.array_equal(three["cost"][0], o["cost"]) and len({three["cost"][w, 0] for w in range(3)}) == 3


def test_a_nan_configuration_sets_failure_and_the_emulated_call_returns():
    """10: configuration 3 of 5 feeds the velocities of 3 and 4 and the accelerations of 2 and 3"""
    c = dc.window_case("chain3_euler", 5)
    Q = c["Q"].copy(); Q[3, 0] = np.nan
    o = emulated_derivatives(c, Q=Q)
    assert o["failure"][2:].all() and not o["failure"][:2].any()
    assert np.isfinite(o["rs"][:2]).all() and np.isfinite(o["rf"][:2]).all()
    clean = emulated_derivatives(c)
    assert not clean["failure"].any() and np.isfinite(clean["gradient"]).all()


# ---------------------------------------------------------------------------------------------------------------- host memory check
def test_host_mirror_under_sanitizers(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "direct_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-o", exe, os.path.join(root, "tests", "host", "direct_main.cpp"), os.path.join(root, "mujoco_mpc_amd", "csrc", "planner.cc"),
                           os.path.join(root, "mujoco_mpc_amd", "csrc", "direct_norms.cc"), "-Wl,--unresolved-symbols=ignore-all", "-lpthread"])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "direct ok", run.stdout
