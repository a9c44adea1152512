"""CPU tier of the table-driven residual (MJPC_TASK_TABLE = 19): the kernel source in its 1-lane emulation, a table task against its
built-in twin on the same inputs and against the independent reference tests/table_ref.py; a fuzz over random models and random
tables; the host's validation through the host-only layout query; PARAM sources."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import emu_lib
import oracle_lib as ol
import table_ref as tr
from mujoco_mpc_amd import capi, modelgen
from mujoco_mpc_amd.modelgen import TABLE_TASKS, ResidualTable, filter_arm, particle_task
from random_models import random_model
from task_ref import TaskRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the built-in twin of every TABLE_TASKS entry
BUILTIN = dict(cartpole=modelgen.cartpole, particle=lambda: modelgen.particle(copystate=True), particle_fixed=lambda: particle_task(fixed=True),
               walker=modelgen.walker, acrobot=modelgen.acrobot, swimmer=modelgen.swimmer, fingers=modelgen.fingers,
               quadrotor=modelgen.quadrotor, quadruped_hill=modelgen.quadruped_hill, humanoid_stand=modelgen.humanoid_stand,
               shadow_hand=modelgen.shadow_hand, allegro=modelgen.allegro, op3=lambda: modelgen.op3(mode=0),
               op3_handstand=lambda: modelgen.op3(mode=1))
# tasks whose rollouts have bodies in contact (feet / forearms / a quadrotor / the fingers' target on the floor, a cube on a hand);
# the others disable contacts or have nothing to touch
CONTACT = {"walker", "fingers", "quadrotor", "quadruped_hill", "humanoid_stand", "shadow_hand", "allegro", "op3", "op3_handstand"}
NAMES = sorted(TABLE_TASKS)


def _rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-300)


def plan_inputs(name, m, d, N, seed=1):
    """the task's own H / P / spline / exploration; OP3 starts from the key of its mode; nominal = the defaults' hold controls"""
    st = d["state"].copy()
    if name.startswith("op3"):
        st[:m["nq"]] = m["key_qpos"][1 if name == "op3_handstand" else 0]
    P, H = d["P"], d["horizon"]
    kt = np.linspace(0, (H - 1) * m["timestep"], P)
    kv = np.tile(d["ctrl0"], (P, 1)) if "ctrl0" in d else np.zeros((P, m["nu"]))
    eps, sel = ol.noise(seed, 0, 0, N, P, m["nu"])
    mocap = d["mocap"] if len(d["mocap"]) else None
    return st, mocap, kt, kv, eps, sel, H


_cache = {}


def _pair(name, N=6):
    """(model, built-in task, table task, built-in plan, table plan, mocap) in the emulation, same state, knots and Philox noise"""
    if name not in _cache:
        m, tb, d = BUILTIN[name]()
        m2, tt, d2 = TABLE_TASKS[name]()
        assert tt["task_id"] == 19 and tt["num_residual"] == tb["num_residual"]
        st, mocap, kt, kv, eps, sel, H = plan_inputs(name, m, d, N)
        kw = dict(sigma=d["sigma"], noise_eps=eps, noise_sel=sel)
        a = emu_lib.plan(m, tb, st, mocap, 0.0, kt, kv, d["interp"], N, H, **kw)
        b = emu_lib.plan(m2, tt, st, mocap, 0.0, kt, kv, d["interp"], N, H, **kw)
        _cache[name] = (m, tb, tt, a, b, mocap)
    return _cache[name]


@pytest.mark.parametrize("name", NAMES)
def test_table_task_matches_its_builtin_twin(name):
    """bit-equal states / actions / times / knots (the dynamics never read the residual); residual rows, costs and returns at 1e-12
    relative to the largest magnitude; same winner; the candidates differ; contact tasks have contacts in play"""
    m, tb, tt, a, b, _ = _pair(name)
    assert not a["failure"].any() and not b["failure"].any()
    for k in ("states", "actions", "times", "knots"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("residual", "costs", "returns"):
        err = _rel(b[k], a[k])
        print(name, k, "table against built-in:", err)
        assert err < 1e-12, (k, err)
    assert np.abs(a["residual"]).max() > 0
    assert int(np.argmin(a["returns"])) == int(np.argmin(b["returns"]))
    assert np.ptp(b["returns"]) > 0
    if name in CONTACT:
        assert b["diag"][:, 1].max() >= 1


@pytest.mark.parametrize("name", NAMES)
def test_table_rows_match_the_independent_reference(name):
    """every candidate and step: the emulated kernel's table rows against table_ref on the kernel's own states at 1e-12; Allegro /
    OP3 also against task_ref.TaskRef, which restates those residuals without a table"""
    m, tb, tt, a, b, mocap = _pair(name)
    S = b["states"].reshape(-1, b["states"].shape[-1]); A = b["actions"].reshape(-1, m["nu"])
    r = tr.TableRef(m, tt).residual(S, A, mocap).reshape(b["residual"].shape)
    err = np.abs(b["residual"] - r).max((0, 1)) / (np.abs(r).max() + 1e-300)
    print(name, "table rows against table_ref:", float(err.max()), "row", int(err.argmax()))
    assert err.max() < 1e-12, (int(err.argmax()), float(err.max()))
    if name in ("allegro", "op3", "op3_handstand"):
        nq, nv = m["nq"], m["nv"]
        r2 = TaskRef(m, tb).residual(S[:, :nq], S[:, nq:nq + nv], A).reshape(b["residual"].shape)
        assert _rel(b["residual"], r2) < 1e-12


# ----------------------------------------------------------------------------------- fuzz: random models, random tables
FUZZ = [("random", s) for s in range(22)] + [("filter_arm", 0), ("particle_fixed", 0)]


def _random_table(m, rng, nparam):
    """one block per source kind the model offers (random object, random slice), then a few blocks that mix two or three terms,
    norms and a quaternion difference; written through the Python builder"""
    t = ResidualTable(m)
    objs = [("body", m["nbody"]), ("xbody", m["nbody"]), ("geom", m["ngeom"]), ("site", m["nsite"])]

    def obj():
        ty, n = objs[int(rng.integers(len(objs)))]
        return ty, int(rng.integers(n))

    makers = [lambda: t.const(rng.normal(size=int(rng.integers(1, 5)))), lambda: t.param()[0:nparam], t.qpos, t.qvel, t.ctrl,
              lambda: t.subtree_com(int(rng.integers(m["nbody"]))), lambda: t.subtree_linvel(int(rng.integers(m["nbody"])))]
    makers += [lambda f=f: f(*obj()) for f in (t.pos, t.quat, t.mat, t.xaxis, t.yaxis, t.zaxis, t.linvel, t.angvel)]
    if m["na"]:
        makers.append(t.act)
    if tr.forces_ok(m):
        makers.append(t.actuator_force)
    if m["nkey"]:
        makers.append(lambda: t.key_qpos(int(rng.integers(m["nkey"]))))
    if m["nmocap"]:
        makers += [lambda f=f: f(int(rng.integers(m["nmocap"]))) for f in (t.mocap_pos, t.mocap_quat, t.mocap_mat)]

    def piece(n=None):
        """a random slice (of n components) of a random source, randomly scaled"""
        while True:
            e = makers[int(rng.integers(len(makers)))]()
            if n is None or len(e) >= n:
                break
        k = int(rng.integers(1, min(len(e), 4) + 1)) if n is None else n
        a = int(rng.integers(0, len(e) - k + 1))
        return float(rng.choice([1.0, -1.0, 0.5, 2.0, rng.normal()])) * e[a:a + k]

    order = rng.permutation(len(makers))
    for i in order:                                       # every kind once, on its own
        e = makers[int(i)]()
        k = int(rng.integers(1, min(len(e), 4) + 1)); a = int(rng.integers(0, len(e) - k + 1))
        t.sum(-1.5 * e[a:a + k])
    for _ in range(int(rng.integers(2, 5))):              # sums of several terms
        k = int(rng.integers(1, 4))
        e = piece(k)
        for _ in range(int(rng.integers(1, 3))):
            e = e + piece(k)
        t.sum(e)
    t.zeros(int(rng.integers(1, 3)))
    for _ in range(2):
        k = int(rng.integers(1, 4))
        t.norm(piece(k) - piece(k))
    qa = t.quat(*obj())
    qb = t.mocap_quat(0) if m["nmocap"] and rng.random() < 0.5 else t.quat(*obj())
    t.subquat(qa, qb, coef=float(rng.choice([1.0, -0.5])))
    params = list(rng.normal(size=nparam))
    return t.task([(t.rows, 0, 1.0)], parameters=params)


_fuzz = {}


def _fuzz_case(kind, seed):
    """(model, defaults, table task) of a fuzz case; the table is a function of (kind, seed) alone"""
    if (kind, seed) not in _fuzz:
        rng = np.random.default_rng([77, seed, len(kind)])
        if kind == "random":
            m, _, d = random_model(seed)
        else:
            m, _, d = filter_arm() if kind == "filter_arm" else particle_task(fixed=True)
        _fuzz[(kind, seed)] = (m, d, _random_table(m, rng, nparam=3))
    return _fuzz[(kind, seed)]


@pytest.mark.parametrize("kind,seed", FUZZ)
def test_fuzz_random_tables_on_random_models(kind, seed):
    """random_model's trees (free / ball / hinge / slide joints, every geom type, a site, motors and servos), plus filter_arm for
    ACT and particle_fixed for MOCAP_*: a random table each, the emulated kernel's rows against table_ref at 1e-12 on every
    (candidate, step), no candidate failed.  test_fuzz_coverage asserts what the tables drew."""
    m, d, task = _fuzz_case(kind, seed)
    P, H, N = 4, 12, 3
    kt = np.linspace(0, (H - 1) * m["timestep"], P)
    kv = np.random.default_rng(1000 + seed).uniform(-0.5, 0.5, (P, m["nu"]))
    eps, sel = ol.noise(seed, 0, 0, N, P, m["nu"])
    mocap = None
    if m["nmocap"]:
        mocap = np.array([0.1, -0.2, 0.05, 0.8, 0.2, -0.4, 0.4])
        mocap[3:] /= np.linalg.norm(mocap[3:])
    out = emu_lib.plan(m, task, d["state"], mocap, 0.0, kt, kv, 2, N, H, sigma=(0.3, 0.0), noise_eps=eps, noise_sel=sel)
    assert not out["failure"].any()
    S = out["states"].reshape(N * H, -1); A = out["actions"].reshape(N * H, -1)
    r = tr.TableRef(m, task).residual(S, A, mocap).reshape(out["residual"].shape)
    err = np.abs(out["residual"] - r).max((0, 1)) / (np.abs(r).max() + 1e-300)
    print(kind, seed, "rows", task["num_residual"], "worst", float(err.max()), "row", int(err.argmax()))
    assert err.max() < 1e-12, (int(err.argmax()), float(err.max()))


def test_fuzz_coverage():
    """across the fuzz cases every source kind, every object type (on a frame quantity), every operation and a non-zero offset are
    drawn: the fuzz cannot pass by drawing nothing"""
    kinds, ops, offset = set(), set(), False
    for kind, seed in FUZZ:
        k, o, f = tr.kinds_used(_fuzz_case(kind, seed)[2])
        kinds |= k; ops |= o; offset |= f
    assert {k for k, _ in kinds} == set(range(21)), sorted(set(range(21)) - {k for k, _ in kinds})
    assert {ty for k, ty in kinds if k >= tr.POS} == {1, 2, 5, 6}
    assert ops == {0, 1, 2} and offset


# ----------------------------------------------------------------------------------- validation (host-only)
def _lib():
    lib = C.CDLL(capi.ENGINE_PATH)
    lib.mjpc_hip_layout_bytes.argtypes = [C.POINTER(capi.MjpcHipModel), C.POINTER(capi.MjpcHipTask), C.c_int]
    lib.mjpc_hip_last_error.restype = C.c_char_p
    return lib


def _layout(m, task, use_cache):
    lib = _lib()
    cm = capi.CModel(m, task)
    n = lib.mjpc_hip_layout_bytes(C.byref(cm.c_model), C.byref(cm.c_task), use_cache)
    return n, lib.mjpc_hip_last_error().decode()


def _base():
    """a table on the ParticleFixed model (one mocap body, key `home`, site `tip`, na = 0) with every record shape in it:
    blocks 0 SUM(2: site pos - mocap pos), 1 NORM(3: site linvel), 2 SUBQUAT(xbody quat, mocap quat), 3 SUM(2: qpos - key_qpos),
    4 SUM(2: ctrl - constants), 5 SUM(1: parameter 0), 6 SUM(1: geom z axis)"""
    m, _, _ = particle_task(fixed=True)
    t = ResidualTable(m)
    t.sum(t.pos("site", "tip") - t.mocap_pos(0), dim=2)
    t.norm(t.linvel("site", "tip"))
    t.subquat(t.quat("xbody", "pointmass"), t.mocap_quat(0))
    t.sum(t.qpos() - t.key_qpos("home"))
    t.sum(t.ctrl() - [0.25, -0.25])
    t.sum(t.param(0))
    t.sum(t.zaxis("geom", "pointmass")[2])
    return m, t.task([(12, 0, 1.0)], parameters=[0.5])


def _edit(task, ints=(), dbls=(), **fields):
    """copy of the task with int_data[i] = v for (i, v) in ints (the same for dbl_data) and other fields replaced"""
    t = dict(task)
    t["int_data"] = np.array(task["int_data"], np.int32); t["dbl_data"] = np.array(task["dbl_data"], float)
    for i, v in ints:
        t["int_data"][i] = v
    for i, v in dbls:
        t["dbl_data"][i] = v
    t.update(fields)
    return t


NB, NT = 7, 11                      # blocks and terms of _base()
BLK = lambda b: 3 + 6 * b           # noqa: E731  [op, row, dim, ncomp, first term, terms]
TRM = lambda j: 3 + 6 * NB + 4 * j  # noqa: E731  [kind, objtype, id, off]
# terms of _base(): 0 site pos, 1 mocap pos, 2 linvel, 3 quat, 4 mocap quat, 5 qpos, 6 key_qpos, 7 ctrl, 8 const, 9 param, 10 geom zaxis
REFUSALS = {
    "unknown operation": (dict(ints=[(BLK(0), 7)]), "block 0"),
    "unknown source kind": (dict(ints=[(TRM(0), 21)]), "block 0 term 0"),
    "negative source kind": (dict(ints=[(TRM(2), -1)]), "block 1 term 2"),
    "unknown object type": (dict(ints=[(TRM(0) + 1, 3)]), "block 0 term 0"),
    "site out of range": (dict(ints=[(TRM(0) + 2, 1)]), "block 0 term 0"),
    "body out of range": (dict(ints=[(TRM(3) + 2, 3)]), "block 2 term 3"),
    "geom out of range": (dict(ints=[(TRM(10) + 2, -1)]), "block 6 term 10"),
    "key out of range": (dict(ints=[(TRM(6) + 2, 1)]), "block 3 term 6"),
    "mocap out of range": (dict(ints=[(TRM(1) + 2, 1)]), "block 0 term 1"),
    "mocap quaternion out of range": (dict(ints=[(TRM(4) + 2, 2)]), "block 2 term 4"),
    "parameter out of range": (dict(ints=[(TRM(9) + 3, 1)]), "block 5 term 9"),
    "no parameters at all": (dict(num_parameter=0), "block 5 term 9"),
    "constants beyond dbl_data": (dict(ints=[(TRM(8) + 2, 12)]), "block 4 term 8"),
    "constants before dbl_data": (dict(ints=[(TRM(8) + 2, -1)]), "block 4 term 8"),
    "offset beyond the source": (dict(ints=[(TRM(0) + 3, 2)]), "block 0 term 0"),
    "negative offset": (dict(ints=[(TRM(5) + 3, -1)]), "block 3 term 5"),
    "blocks overlap": (dict(ints=[(BLK(1) + 1, 1)]), "block 1"),
    "blocks leave a gap": (dict(ints=[(BLK(1) + 1, 3)]), "block 1"),
    "blocks end before num_residual": (dict(num_residual=13, dim_norm_residual=np.array([13], np.int32)), "num_residual"),
    "blocks run past num_residual": (dict(num_residual=11, dim_norm_residual=np.array([11], np.int32)), "block 6"),
    "empty block": (dict(ints=[(BLK(5) + 2, 0), (BLK(5) + 3, 0)]), "block 5"),
    "SUM with ncomp != dim": (dict(ints=[(BLK(0) + 3, 3)]), "block 0"),
    "NORM of two rows": (dict(ints=[(BLK(1) + 2, 2)]), "block 1"),
    "NORM without components": (dict(ints=[(BLK(1) + 3, 0)]), "block 1"),
    "NORM over too many components": (dict(ints=[(BLK(1) + 3, 17)]), "block 1"),
    "SUBQUAT of a position": (dict(ints=[(TRM(3), 13)]), "block 2 term 3"),
    "SUBQUAT with an offset": (dict(ints=[(TRM(4) + 3, 1)]), "block 2 term 4"),
    "SUBQUAT with two rows": (dict(ints=[(BLK(2) + 2, 2)]), "block 2"),
    "terms out of order": (dict(ints=[(BLK(3) + 4, 6)]), "block 3"),
    "ACT without activation states": (dict(ints=[(TRM(5), 4)]), "block 3 term 5"),
    "num_int shorter than the header claims": (dict(num_int=3 + 6 * NB + 4 * NT - 1), "num_int"),
    "num_int shorter than the header": (dict(num_int=2), "num_int"),
    "num_dbl shorter than the header claims": (dict(num_dbl=NT - 1), "num_dbl"),
    "too many blocks": (dict(ints=[(1, 65)]), "65 blocks"),
    "too many terms": (dict(ints=[(2, 257)]), "257 terms"),
    "unknown version": (dict(ints=[(0, 2)]), "version"),
}


def test_base_table_is_accepted_and_runs():
    m, task = _base()
    I = [int(x) for x in task["int_data"]]
    assert I[:3] == [1, NB, NT] and len(I) == 3 + 6 * NB + 4 * NT and task["num_residual"] == 12
    assert [I[TRM(j)] for j in range(NT)] == [13, 8, 19, 14, 9, 2, 7, 5, 0, 1, 18]
    n, _ = _layout(m, task, 1)
    assert n > 0
    out = emu_lib.plan(m, task, np.array([0.05, -0.1, 0.3, 0.2]), np.array([0.25, 0, 0.01, 1, 0, 0, 0.0]), 0.0, np.array([0.0]),
                       np.array([[0.5, -0.5]]), 0, 1, 3, sigma=(0.0, 0.0))
    r = out["residual"][0, 0]
    np.testing.assert_allclose(r[:2], [0.05 - 0.25, -0.1], rtol=0, atol=1e-15)
    np.testing.assert_allclose(r[2], np.hypot(0.3, 0.2), rtol=1e-15)
    np.testing.assert_allclose(r[3:6], 0, atol=1e-15)
    np.testing.assert_allclose(r[6:8], [0.05 - 1.0, -0.1 - 2.0], rtol=1e-15)
    np.testing.assert_allclose(r[8:10], [0.5 - 0.25, -0.5 + 0.25], rtol=1e-15)
    assert r[10] == 0.5 and r[11] == 1.0


@pytest.mark.parametrize("rule", sorted(REFUSALS))
def test_bad_table_is_refused_by_the_layout_query(rule):
    edit, names = REFUSALS[rule]
    m, task = _base()
    for use_cache in (1, 0):
        n, msg = _layout(m, _edit(task, **edit), use_cache)
        assert n < 0, rule
        assert "residual table" in msg and names in msg, (rule, msg)


@pytest.mark.parametrize("name", NAMES)
def test_table_tasks_are_accepted_and_add_no_per_candidate_array(name):
    """direct flavour (no task block in LDS): exactly the built-in twin's bytes; cached flavour: at most the growth of the task
    block (4 bytes per int, 8 per double, 16 of rounding) more"""
    m, tb, _ = BUILTIN[name]()
    m2, tt, _ = TABLE_TASKS[name]()
    direct = [_layout(mm, t, 0)[0] for mm, t in ((m, tb), (m2, tt))]
    cached = [_layout(mm, t, 1)[0] for mm, t in ((m, tb), (m2, tt))]
    assert direct[0] > 0 and direct[1] == direct[0], direct
    grow = 4 * (int(tt["num_int"]) - int(tb["num_int"])) + 8 * (int(tt["num_dbl"]) - int(tb["num_dbl"]))
    assert cached[0] > 0 and 0 < cached[1] <= cached[0] + grow + 16, (cached, grow)


def test_header_names_the_table_task():
    with open(os.path.join(ROOT, "include", "mjpc_hip.h")) as f:
        h = f.read()
    assert re.search(r"MJPC_TASK_TABLE\s*=\s*19\b", h) and re.search(r"#define MJPC_HIP_ABI_VERSION 4\b", h)
    for k, name in enumerate(tr.KIND_NAMES):
        assert re.search(rf"MJPC_TBL_{name}\s*=\s*{k}\b", h), name
    for k, name in enumerate(("SUM", "NORM", "SUBQUAT")):
        assert re.search(rf"MJPC_TBL_OP_{name}\s*=\s*{k}\b", h), name


# ----------------------------------------------------------------------------------- PARAM
def test_parameters_move_exactly_the_rows_that_read_them():
    """two one-step plans on the walker table that differ only in `parameters`: rows 6 (height goal) and 8 (speed goal) move by the
    change, every other row is bit-equal"""
    m, task, d = TABLE_TASKS["walker"]()
    kt = np.array([0.0]); kv = np.full((1, m["nu"]), 0.1)
    r = []
    for prm in ([1.2, 0.0], [1.0, 0.75]):
        t = dict(task, parameters=np.array(prm, float))
        r.append(emu_lib.plan(m, t, d["state"], None, 0.0, kt, kv, 0, 1, 2, sigma=(0.0, 0.0))["residual"][0])
    moved = np.flatnonzero((r[0] != r[1]).any(0))
    assert list(moved) == [6, 8]
    np.testing.assert_allclose(r[1][:, 6] - r[0][:, 6], 0.2, rtol=0, atol=1e-15)
    np.testing.assert_allclose(r[1][:, 8] - r[0][:, 8], -0.75, rtol=0, atol=1e-15)


# ----------------------------------------------------------------------------------- the Python builder
def test_builder_checks_names_lengths_and_coverage():
    m, _, _ = particle_task(fixed=True)
    t = ResidualTable(m)
    with pytest.raises(KeyError):
        t.pos("site", "no_such_site")
    with pytest.raises(IndexError):
        t.pos("body", 99)
    with pytest.raises(ValueError):
        t.pos("site", "tip") - t.mocap_quat(0)              # 3 against 4 components
    with pytest.raises(ValueError):
        t.subquat(t.pos("site", "tip"), t.mocap_quat(0))
    with pytest.raises(ValueError):
        t.act()                                             # na = 0
    t.sum(t.pos("site", "tip")[:2] - t.mocap_pos(0)[:2])
    with pytest.raises(ValueError):
        t.task([(3, 0, 1.0)])                               # the cost table covers 3 rows, the table writes 2
    t.sum(t.param(1))
    with pytest.raises(IndexError):
        t.task([(3, 0, 1.0)], parameters=[0.5])             # parameter 1 of 1
    assert t.task([(3, 0, 1.0)], parameters=[0.5, 0.25])["task_id"] == 19
