"""Designed batches for the task-residual reference (tests/task_ref.py), shared by the CPU tier (tests/test_task_reference.py) and the
GPU tier (tests/test_gpu_task_reference.py).  TEST INFRASTRUCTURE ONLY.

Nothing is sampled from rollouts: each batch is laid out so that every branch of a residual is entered on purpose, and the tests
assert that it was.  A batch is a list of groups; a group is one task dict (mode, parameters and frozen residual state are per
task, not per state), one mocap input and a handful of states, controls and times.  Every case's distance to a point where a row
may flip on a 1-ulp difference is computed from the reference alone (TaskRef.margin); a case closer than MARGIN is redrawn, so
the tests exclude nothing.
"""
import functools
from fractions import Fraction

import numpy as np

from mujoco_mpc_amd import modelgen
from mujoco_mpc_amd.modelgen.tasks import INTERACT_WEIGHTS, select_value
from dyn_ref import DynRef
from task_ref import TaskRef, ground, frames, _t

MARGIN = 1e-6
QUADRUPED_MODES = ("quadruped", "biped", "walk", "scramble", "flip")
GROUPS, PER_GROUP = 16, 8                                   # 128 states per quadruped mode
DUTY = (0.0, 0.3, 0.75, 1.0)
PHASE_VELOCITY = (0.0, 4 * np.pi, -3.0)                      # -3: fmod's argument goes negative
ANGVEL = (0.0, 0.005, 0.5, -1.0)                             # both sides of kMinAngvel = 0.01
PLACES = dict(flat=(0.0, 0.0), ramp=(3.1, 2.5), hill=(5.0, 5.0), box=(-2.5, 0.0))
RISKS = (0.0, 0.7, -0.7, 5.0)
TRACK_MOTIONS = (0, 4, 8, 9)


def _rot_quat(rng, max_angle):
    axis = rng.standard_normal(3); axis /= np.linalg.norm(axis)
    a = rng.uniform(0, max_angle)
    return np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * axis])


def flip_bounds(D):
    """the four phase boundaries from the stored doubles, summed left to right as the reference's expressions are"""
    crouch, jump, flight, land = D[21], D[23], D[19], D[25]
    return [crouch, jump, jump + flight, jump + flight + land]


def _quadruped_task(base, mode, g, rng):
    t = dict(base)
    I = np.array(base["int_data"]).copy(); D = np.array(base["dbl_data"], float).copy(); P = np.array(base["parameters"], float).copy()
    I[-1] = mode
    exact = mode == 4 and g % 4 == 3                        # groups whose states sit ON the flip boundaries: mode_start = 0
    D[0] = 0.0 if exact else rng.uniform(0, 0.3)
    D[1:3] = rng.uniform(-1, 1, 2); D[4:6] = rng.uniform(-1, 1, 2); D[6] = rng.uniform(0, 1); D[7] = ANGVEL[g % 4]; D[8] = rng.uniform(-0.05, 0.05)
    o = rng.standard_normal(4); D[9:13] = o / np.linalg.norm(o)
    D[13] = select_value(g % 5); D[14] = rng.uniform(0, 6); D[15] = rng.uniform(0, 0.2); D[16] = PHASE_VELOCITY[g % 3]
    P[I[9]] = select_value((g // 2) % 2); P[I[10]] = select_value(g % 2)
    P[I[12]] = 0.0 if g in (7, 12) else rng.uniform(0.01, 0.1)
    P[I[13]] = DUTY[g % 4]; P[I[14]] = rng.uniform(-3.1, 3.1)
    t["int_data"], t["dbl_data"], t["parameters"] = I, D, P
    return t, exact


def _quadruped_state(m, d, mode, n, place, rng, low):
    st = d["state"].copy()
    xy = np.array(PLACES[place]) + rng.uniform(-0.8, 0.8, 2)
    st[0:2] = xy
    st[3:7] = _rot_quat(rng, 0.1 if low else 1.0)
    st[2] = rng.uniform(0.5, 1.2)
    st[7:19] += rng.uniform(-0.3, 0.3, 12); st[19:] = rng.standard_normal(m["nv"])
    return st


def _quadruped_group(m, base, d, mode, g, rng):
    places = list(PLACES)
    task, exact = _quadruped_task(base, mode, g, rng)
    D = task["dbl_data"]
    mocap = d["mocap"].copy()
    X, U, T = [], [], []
    plc = [places[(g + j) % 4] for j in range(PER_GROUP)]
    ang = 2 * np.pi * g / GROUPS                                                 # Scramble: the goal goes round the robot
    mocap[:3] = np.array([*PLACES[plc[0]], 0.3]) + np.array([2.0 * np.cos(ang), 2.0 * np.sin(ang), rng.uniform(-0.2, 0.2)]) if mode == 3 \
        else mocap[:3] + rng.uniform(-1, 1, 3)
    mocap[7:10] += rng.uniform(-0.1, 0.1, 3)
    mocap[10:14] = np.array([np.cos(0.2 * g), 0, 0, np.sin(0.2 * g)]) * 1.3      # the box turned about z, its quaternion NOT of unit length
    bounds = flip_bounds(D)
    ref = _dynref(m)
    for j in range(PER_GROUP):
        low = mode == 3 and j % 2 == 1                                           # Scramble: every other state has its feet near their targets
        st = _quadruped_state(m, d, mode, j, plc[j], rng, low)
        if low:
            f = frames(ref, m, _t(st[None, :m["nq"]]), mocap)
            st[2] = ground(m, f, np.array([[st[0], st[1], 1.0]]))[0][0] + rng.uniform(0.27, 0.36)
        X.append(st); U.append(rng.uniform(-1, 1, m["nu"]))
        if mode == 4:
            k = (g * PER_GROUP + j) % 5                                           # spread over the five phases
            edges = [0.0] + bounds + [bounds[-1] + 0.3]
            Tm = rng.uniform(edges[k], edges[k + 1])
            if exact and j < 4:
                Tm = bounds[j]                                                   # the stored double itself: T - 0 == boundary on both sides
            T.append(D[0] + Tm)
        else:
            T.append(rng.uniform(0, 1.6))
    return dict(task=task, mocap=mocap, X=np.array(X), U=np.array(U), T=np.array(T), places=plc)


_DYNREF = {}


def _dynref(m):
    """one DynRef per model object (kept alive with it)"""
    if id(m) not in _DYNREF:
        _DYNREF[id(m)] = (m, DynRef(m))
    return _DYNREF[id(m)][1]


def _fill_reference(m, groups, jac=None):
    """the reference's rows, branches and margins of each group; the Jacobians of all states in one batched call"""
    nq, nv = m["nq"], m["nv"]
    if jac is None:
        jac = _dynref(m).jacobians(_t(np.concatenate([g["X"][:, :nq] for g in groups])))
    at = 0
    for g in groups:
        n = len(g["X"])
        tr = TaskRef(m, g["task"])
        g["ref"] = tr.residual(g["X"][:, :nq], g["X"][:, nq:nq + nv], g["U"], g["T"], g["mocap"], jac={k: x[at:at + n] for k, x in jac.items()})
        g["entered"], g["margin"] = dict(tr.entered), tr.margin.copy()
        at += n
    return groups


def quadruped_batch(mode, seed=0):
    """[group dict(task, mocap, X [8, 37], U [8, 12], T [8], places, ref, entered, margin)] x 16 for one mode; a group with a case
    closer than MARGIN to a boundary is drawn again"""
    m, base, d = modelgen.quadruped()
    rng = np.random.default_rng(100 * mode + seed)
    groups = _fill_reference(m, [_quadruped_group(m, base, d, mode, g, rng) for g in range(GROUPS)])
    for g in range(GROUPS):
        for _ in range(100):
            if groups[g]["margin"].min() >= MARGIN:
                break
            groups[g] = _fill_reference(m, [_quadruped_group(m, base, d, mode, g, rng)])[0]
        else:
            raise RuntimeError("no admissible group found")
    return m, groups


def key_time(k, start, ref_time):
    """the first double at or after ref_time + k / 30 whose exact index (time - ref_time) * 30 + start is >= start + k: the product
    is rarely exact, but rounding is monotone, so every spelling of it (two roundings or one fused) lands on start + k or a few ulp
    above and floors to the same key; a double on the other side would floor to the key before on some spellings only"""
    c = ref_time + k / 30.0
    while Fraction(c - ref_time) * 30 < k:
        c = float(np.nextafter(c, np.inf))
    while Fraction(float(np.nextafter(c, -np.inf)) - ref_time) * 30 >= k:
        c = float(np.nextafter(c, -np.inf))
    return c


def tracking_batch(motion, seed=0):
    """32 states of one motion in one group: 4 each of: before the start (two of them before key 0 of the whole table, where the
    index clamps; the others read the motion stored before this one, as the reference does), ON the first key, ON an inner key, half-way between two
    keys, a random inner time, ON the second-to-last key, ON the last key, past the end.  ref_time is 0.25 (exact in binary)."""
    m, task, d = modelgen.humanoid_track(motion=motion)
    rng = np.random.default_rng(400 + motion + seed)
    task = dict(task); task["dbl_data"] = np.array([0.25])
    start, length = int(task["int_data"][1]), int(task["int_data"][2])
    ref = 0.25
    X, U, T = [], [], []
    for n in range(32):
        kind, j = n // 4, n % 4
        inner = int(rng.integers(2, length - 3))
        tm = [ref - (0.5, 1e-3, start / 30.0 + 7.0, start / 30.0 + 1e-3)[j], key_time(0, start, ref), key_time(inner, start, ref), ref + (2 * inner + 1) / 60.0,
              ref + rng.uniform(0, (length - 1) / 30.0), key_time(length - 2, start, ref), key_time(length - 1, start, ref),
              ref + (length - 1) / 30.0 + (1e-3, 1 / 30, 0.5, 5.0)[j]][kind]
        st = d["state"].copy()
        nq = m["nq"]
        st[7:nq] += 0.3 * rng.standard_normal(nq - 7); st[nq:] = rng.standard_normal(m["nv"])
        qq = st[3:7] + 0.3 * rng.standard_normal(4); st[3:7] = qq / np.linalg.norm(qq)
        X.append(st); U.append(rng.uniform(-1, 1, m["nu"])); T.append(tm)
    X, U, T = np.array(X), np.array(U), np.array(T)
    return m, [dict(task=task, mocap=d["mocap"].copy(), X=X, U=U, T=T)]


def _humanoid_states(m, d, n, rng):
    nq = m["nq"]
    X = np.tile(d["state"], (n, 1))
    X[:, 7:nq] += 0.3 * rng.standard_normal((n, nq - 7)); X[:, nq:] = rng.standard_normal((n, m["nv"]))
    qq = X[:, 3:7] + 0.4 * rng.standard_normal((n, 4)); X[:, 3:7] = qq / np.linalg.norm(qq, axis=-1, keepdims=True)
    X[:, :2] += rng.uniform(-0.5, 0.5, (n, 2)); X[:, 2] += rng.uniform(0.0, 0.3, n)
    return X


def walk_batch(seed=0):
    """64 states: 56 random ones; 4 lying on the side with the joints at zero (the model is mirror-symmetric, so the feet coincide
    in the plane and the support segment's half length goes negative); 4 with the root's x axis straight up and the joints at zero
    (the summed forward vector is exactly (0, 0): mju_normalize's guard, forward = (1, 0))"""
    m, task, d = modelgen.humanoid_walk()
    rng = np.random.default_rng(600 + seed)
    nq = m["nq"]
    X = _humanoid_states(m, d, 64, rng)
    X[56:60, 3:7] = [np.sqrt(0.5), np.sqrt(0.5), 0.0, 0.0]; X[56:60, 7:nq] = 0.0
    X[60:64, 3:7] = [0.5, -0.5, -0.5, -0.5]; X[60:64, 7:nq] = 0.0
    U = rng.uniform(-1, 1, (64, m["nu"]))
    return m, [dict(task=task, mocap=None, X=X, U=U, T=np.zeros(64))]


INTERACT_PAIRS = (("hand_right", (0.01, 0.02, -0.03), "chair", (0.1, 0.3, 0.2)), ("pelvis", (0.0, 0.0, -0.05), "chair", (0.0, 0.0, 0.17)),
                  ("foot_left", (0.05, 0.0, 0.0), -1, (0.0, 0.0, 0.0)), (-1, (0.0, 0.0, 0.0), -1, (0.0, 0.0, 0.0)),
                  ("head", (0.0, 0.0, 0.1), "lower_arm_left", (0.1, 0.0, 0.0)))
INTERACT_FACING = ("none", "target", "above")


def interact_batch(seed=0):
    """the four modes' weight rows x (no facing target, a target, the target straight above the torso) x 8 states; three active
    contact pairs, one with only its first body chosen and one with none.  `above`: root at the origin of the plane with the identity
    quaternion, so the torso's inertial frame sits at body_ipos exactly and the target minus it is exactly (0, 0): n < mjMINVAL"""
    groups = []
    rng = np.random.default_rng(700 + seed)
    for mode in range(4):
        for facing in INTERACT_FACING:
            m, _, d = modelgen.humanoid_interact()
            torso = m["names"]["body"]["torso"]
            target = dict(none=None, target=tuple(rng.uniform(-2, 2, 2)), above=tuple(np.asarray(m["body_ipos"], float)[torso][:2]))[facing]
            m, task, d = modelgen.humanoid_interact(contact_pairs=INTERACT_PAIRS, facing_target=target)
            task = dict(task); task["weight"] = np.array(INTERACT_WEIGHTS[mode], float)
            X = _humanoid_states(m, d, 8, rng)
            if facing == "above":
                X[:, 0:2] = 0.0; X[:, 3:7] = [1.0, 0.0, 0.0, 0.0]
            groups.append(dict(task=task, mocap=None, X=X, U=rng.uniform(-1, 1, (8, m["nu"])), T=np.zeros(8), mode=mode, facing=facing))
    return m, groups


@functools.lru_cache(maxsize=None)
def designed(name):
    """name: quadruped_<mode>, tracking_<motion>, walk, interact -> (model, groups); each group also carries the reference's rows
    `ref` [n, nr], the branches `entered` and the margins `margin` [n], computed once and shared by the tests (do not modify)"""
    if name.startswith("quadruped_"):
        m, groups = quadruped_batch(QUADRUPED_MODES.index(name[10:]))
    elif name.startswith("tracking_"):
        m, groups = tracking_batch(int(name[9:]))
    else:
        m, groups = dict(walk=walk_batch, interact=interact_batch)[name]()
    if "ref" not in groups[0]:
        same = all(g["X"].shape[1] == groups[0]["X"].shape[1] for g in groups)
        groups = _fill_reference(m, groups) if same else groups
    for g in groups:
        assert g["margin"].min() >= MARGIN                                        # 0 rows excluded: every case is clear of every boundary
    return m, groups


DESIGNED = [f"quadruped_{x}" for x in QUADRUPED_MODES] + [f"tracking_{k}" for k in TRACK_MOTIONS] + ["walk", "interact"]


# ----------------------------------------------------------------------------------- small plans
def plan_task(name):
    """(model, task, defaults) of the small plans: one per quadruped mode (a mid-table gait, mode entered at the plan's start) and
    per humanoid task"""
    if name.startswith("quadruped_"):
        mode = QUADRUPED_MODES.index(name[10:])
        m, base, d = modelgen.quadruped()
        rng = np.random.default_rng(900 + mode)
        task, _ = _quadruped_task(base, mode, 5, rng)                             # group 5 of _quadruped_task: duty ratio 0.3, |angvel| 0.005
        task["dbl_data"][13] = select_value(1 + mode % 4); task["dbl_data"][0] = 0.0        # a moving gait; the mode starts with the plan
        task["dbl_data"][16] = 4 * np.pi
        return m, task, d
    if name.startswith("tracking_"):
        return modelgen.humanoid_track(motion=int(name[9:]))
    if name == "walk":
        return modelgen.humanoid_walk()
    m, task, d = modelgen.humanoid_interact(contact_pairs=INTERACT_PAIRS, facing_target=(1.0, 0.5))
    return m, task, d


PLANS = [f"quadruped_{x}" for x in QUADRUPED_MODES] + ["tracking_0", "walk", "interact"]


def plan_inputs(m, d, N, H, seed=7):
    """the task's own P and spline, zero nominal, explicit Philox noise"""
    import oracle_lib as ol
    P = d["P"]
    kt = np.linspace(0, (H - 1) * m["timestep"], P); kv = np.zeros((P, m["nu"]))
    eps, sel = ol.noise(seed, 0, 0, N, P, m["nu"])
    mocap = d.get("mocap")
    mocap = mocap if mocap is not None and len(mocap) else None
    return dict(state=d["state"], mocap=mocap, time=0.0, knot_times=kt, knot_values=kv, interp=d["interp"], sigma=d["sigma"], eps=eps, sel=sel)


def rollout_reference(m, task, mocap, out, skip_below=1e-9):
    """TaskRef rows on a plan's own states, actions and times (arrays [N, H, .]); rows of cases whose reference margin is under
    skip_below are marked: returns (rows, keep [N, H] bool, TaskRef)"""
    nq, nv = m["nq"], m["nv"]
    S = out["states"].reshape(-1, out["states"].shape[-1]); A = out["actions"].reshape(-1, m["nu"]); T = out["times"].reshape(-1)
    tr = TaskRef(m, task)
    r = tr.residual(S[:, :nq], S[:, nq:nq + nv], A, T, mocap).reshape(out["residual"].shape)
    keep = (tr.margin >= skip_below).reshape(out["times"].shape)
    return r, keep, tr
