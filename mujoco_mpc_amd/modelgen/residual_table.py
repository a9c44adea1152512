"""Table-driven residuals (MJPC_TASK_TABLE = 19, include/mjpc_hip.h): a task's residual written as a list of blocks of linear
terms over named sources, so that a task needs no device code of its own.

    t = ResidualTable(model)
    t.sum(t.ctrl())                                              # nu rows
    t.sum(t.pos("xbody", "torso")[2] - t.param(0))               # one row: torso height - goal
    t.sum(t.pos("site", "tip") - t.mocap_pos(0), dim=2)          # xy only
    t.norm(t.pos("site", "a") - t.pos("site", "b"))              # one row: a distance
    t.subquat(t.quat("body", "goal"), t.quat("body", "cube"))    # three rows
    task = t.task(terms, parameters=..., traces=...)             # the make_task dict with task_id = 19

A source call returns an `Expr` (a linear combination of sources, all of one length) that can be sliced (`[2]`, `[:2]`, `[7:23]`),
scaled, negated, added and subtracted; a number or a sequence on the other side of `+` / `-` becomes a constant.  Objects are named
through model["names"] (an integer id is taken as it is); the object types are "body" (the inertial frame, MuJoCo's
objtype="body"), "xbody", "geom" and "site".

`TABLE_TASKS` restates registry tasks as tables: name -> generator returning the usual (model, task, defaults), same model, cost
table, parameters, traces and defaults as the built-in task, only the residual comes from a table.  They are not in REGISTRY.
"""
from __future__ import annotations

import numpy as np

from . import tasks as T
from .tasks import OBJ_BODY, OBJ_GEOM, OBJ_SITE, OBJ_XBODY, make_task

TASK_TABLE = 19
TBL_VERSION = 1
OP_SUM, OP_NORM, OP_SUBQUAT = 0, 1, 2
(SRC_CONST, SRC_PARAM, SRC_QPOS, SRC_QVEL, SRC_ACT, SRC_CTRL, SRC_ACTUATOR_FORCE, SRC_KEY_QPOS, SRC_MOCAP_POS, SRC_MOCAP_QUAT,
 SRC_MOCAP_MAT, SRC_SUBTREE_COM, SRC_SUBTREE_LINVEL, SRC_POS, SRC_QUAT, SRC_MAT, SRC_XAXIS, SRC_YAXIS, SRC_ZAXIS, SRC_LINVEL,
 SRC_ANGVEL) = range(21)
# late kinds (include/mjpc_hip.h): they need the converged solve and exist in the one-step calls only; a rollout writes their rows as 0.0
SRC_QACC, SRC_LINACC, SRC_ANGACC, SRC_ACCELEROMETER, SRC_GYRO, SRC_VELOCIMETER, SRC_TOUCH = range(21, 28)
ZONES = {"sphere": 2, "capsule": 3, "ellipsoid": 4, "cylinder": 5, "box": 6}
_ZONE_SIZES = {2: 1, 3: 2, 4: 3, 5: 2, 6: 3}          # how many of size[3] the shape reads (MuJoCo's size conventions)
MAX_BLOCKS, MAX_TERMS, MAX_NORM = 64, 256, 16
_OBJ = {"body": OBJ_BODY, "xbody": OBJ_XBODY, "geom": OBJ_GEOM, "site": OBJ_SITE}
_OBJ_NAMES = {OBJ_BODY: "body", OBJ_XBODY: "body", OBJ_GEOM: "geom", OBJ_SITE: "site"}
_FRAME_LEN = {SRC_POS: 3, SRC_QUAT: 4, SRC_MAT: 9, SRC_XAXIS: 3, SRC_YAXIS: 3, SRC_ZAXIS: 3, SRC_LINVEL: 3, SRC_ANGVEL: 3, SRC_LINACC: 3, SRC_ANGACC: 3,
              SRC_ACCELEROMETER: 3, SRC_GYRO: 3, SRC_VELOCIMETER: 3}


class Expr:
    """sum of coef * source[off : off + n]; terms = [(coef, kind, objtype, id, off, constant values or None)]"""

    __array_ufunc__ = None        # a numpy scalar on the left of * / + / - defers to the methods below

    def __init__(self, terms, n):
        self.terms, self.n = list(terms), int(n)

    def __len__(self):
        return self.n

    def __getitem__(self, key):
        if isinstance(key, slice):
            a, b, step = key.indices(self.n)
            if step != 1 or b <= a:
                raise ValueError("a source is sliced by a non-empty contiguous range")
        else:
            a = int(key) + (self.n if int(key) < 0 else 0)
            b = a + 1
            if not 0 <= a < self.n:
                raise IndexError(f"component {key} of a source of length {self.n}")
        return Expr([(c, k, ty, i, off + a, v) for c, k, ty, i, off, v in self.terms], b - a)

    def _other(self, other):
        if isinstance(other, Expr):
            if other.n != self.n:
                raise ValueError(f"lengths differ: {self.n} and {other.n}")
            return other
        v = np.asarray(other, float).ravel()
        if v.size == 1 and self.n > 1:
            v = np.full(self.n, float(v[0]))
        if v.size != self.n:
            raise ValueError(f"a constant of length {v.size} beside a source of length {self.n}")
        return Expr([(1.0, SRC_CONST, 0, 0, 0, v)], self.n)

    def __add__(self, other):
        return Expr(self.terms + self._other(other).terms, self.n)

    def __sub__(self, other):
        return self + (-self._other(other))

    def __radd__(self, other):
        return self._other(other) + self

    def __rsub__(self, other):
        return self._other(other) - self

    def __neg__(self):
        return self * -1.0

    def __mul__(self, s):
        return Expr([(c * float(s), k, ty, i, off, v) for c, k, ty, i, off, v in self.terms], self.n)

    __rmul__ = __mul__


class ResidualTable:
    def __init__(self, model: dict):
        self.m = model
        self.blocks = []          # (op, dim, ncomp, [terms])
        self.rows = 0

    # ---- sources
    def _id(self, objtype, name):
        ty = _OBJ[objtype] if isinstance(objtype, str) else int(objtype)
        kind = _OBJ_NAMES[ty]
        i = self.m["names"][kind][name] if isinstance(name, str) else int(name)
        count = {"body": self.m["nbody"], "geom": self.m["ngeom"], "site": self.m["nsite"]}[kind]
        if not 0 <= i < count:
            raise IndexError(f"{kind} {name}: id {i} out of range ({count})")
        return ty, i

    def _src(self, kind, n, ty=0, i=0):
        if n < 1:
            raise ValueError("the model has no such quantity (length 0)")
        return Expr([(1.0, kind, ty, i, 0, None)], n)

    def const(self, values):
        v = np.asarray(values, float).ravel()
        return Expr([(1.0, SRC_CONST, 0, 0, 0, v)], v.size)

    def param(self, i=None):
        """parameters[i], or the whole parameter vector to slice (needs the parameter count: pass `num_parameter=` to task())"""
        e = Expr([(1.0, SRC_PARAM, 0, 0, 0, None)], 1 << 20)
        return e if i is None else e[int(i)]

    def qpos(self): return self._src(SRC_QPOS, self.m["nq"])
    def qvel(self): return self._src(SRC_QVEL, self.m["nv"])
    def act(self): return self._src(SRC_ACT, self.m["na"])
    def ctrl(self): return self._src(SRC_CTRL, self.m["nu"])
    def actuator_force(self): return self._src(SRC_ACTUATOR_FORCE, self.m["nu"])

    def key_qpos(self, key):
        k = self.m["names"]["key"][key] if isinstance(key, str) else int(key)
        if not 0 <= k < self.m["nkey"]:
            raise IndexError(f"key {key} out of range ({self.m['nkey']})")
        return self._src(SRC_KEY_QPOS, self.m["nq"], 0, k)

    def _mocap(self, kind, n, i):
        if not 0 <= int(i) < self.m["nmocap"]:
            raise IndexError(f"mocap body {i} out of range ({self.m['nmocap']})")
        return self._src(kind, n, 0, int(i))

    def mocap_pos(self, i=0): return self._mocap(SRC_MOCAP_POS, 3, i)
    def mocap_quat(self, i=0): return self._mocap(SRC_MOCAP_QUAT, 4, i)
    def mocap_mat(self, i=0): return self._mocap(SRC_MOCAP_MAT, 9, i)
    def subtree_com(self, body): return self._src(SRC_SUBTREE_COM, 3, 0, self._id("body", body)[1])
    def subtree_linvel(self, body): return self._src(SRC_SUBTREE_LINVEL, 3, 0, self._id("body", body)[1])

    def _frame(self, kind, objtype, name):
        ty, i = self._id(objtype, name)
        return self._src(kind, _FRAME_LEN[kind], ty, i)

    def pos(self, objtype, name): return self._frame(SRC_POS, objtype, name)
    def quat(self, objtype, name): return self._frame(SRC_QUAT, objtype, name)
    def mat(self, objtype, name): return self._frame(SRC_MAT, objtype, name)
    def xaxis(self, objtype, name): return self._frame(SRC_XAXIS, objtype, name)
    def yaxis(self, objtype, name): return self._frame(SRC_YAXIS, objtype, name)
    def zaxis(self, objtype, name): return self._frame(SRC_ZAXIS, objtype, name)
    def linvel(self, objtype, name): return self._frame(SRC_LINVEL, objtype, name)
    def angvel(self, objtype, name): return self._frame(SRC_ANGVEL, objtype, name)

    # ---- late sources: a block that uses one may otherwise only hold late sources, constants and parameters, and is a sum or a norm
    def qacc(self): return self._src(SRC_QACC, self.m["nv"])
    def linacc(self, objtype, name): return self._frame(SRC_LINACC, objtype, name)
    def angacc(self, objtype, name): return self._frame(SRC_ANGACC, objtype, name)
    def accelerometer(self, site): return self._frame(SRC_ACCELEROMETER, "site", site)
    def gyro(self, site): return self._frame(SRC_GYRO, "site", site)
    def velocimeter(self, site): return self._frame(SRC_VELOCIMETER, "site", site)

    def touch(self, site, shape, size):
        """sum of the normal forces of the contacts of the site's body inside the zone `shape` ("sphere", "capsule", "ellipsoid",
        "cylinder", "box") of MuJoCo's `size` around the site"""
        ty, i = self._id("site", site)
        z = ZONES[shape] if isinstance(shape, str) else int(shape)
        if z not in _ZONE_SIZES:
            raise ValueError(f"unknown touch zone shape {shape}")
        v = np.zeros(3); sz = np.asarray(size, float).ravel()
        if sz.size < _ZONE_SIZES[z] or sz.size > 3:
            raise ValueError(f"a {shape} zone reads {_ZONE_SIZES[z]} sizes, got {sz.size}")
        v[:sz.size] = sz
        if not np.all(v[:_ZONE_SIZES[z]] > 0):
            raise ValueError("touch zone sizes must be positive")
        return Expr([(1.0, SRC_TOUCH, z, i, 0, v)], 1)

    # ---- blocks (each appends rows behind the ones before it)
    def _cut(self, expr, dim):
        if not isinstance(expr, Expr):
            raise TypeError("a block takes an expression of sources")
        if dim is not None:
            expr = expr[:int(dim)]
        if expr.n >= 1 << 20:
            raise ValueError("slice the parameter vector: param(i) or param()[a:b]")
        return expr

    def _add(self, op, dim, ncomp, terms):
        if any(t[1] >= SRC_QACC for t in terms):
            if op == OP_SUBQUAT or any(t[1] < SRC_QACC and t[1] not in (SRC_CONST, SRC_PARAM) for t in terms):
                raise ValueError("a late block (acceleration / touch sources) is a sum or a norm of late sources, constants and parameters only")
        self.blocks.append((op, int(dim), int(ncomp), list(terms)))
        self.rows += int(dim)
        return self

    def sum(self, expr, dim=None):
        """rows = the expression's components (the first `dim` of them)"""
        e = self._cut(expr, dim)
        return self._add(OP_SUM, e.n, e.n, e.terms)

    def zeros(self, n):
        """n rows of zeros (a block without terms)"""
        return self._add(OP_SUM, n, n, [])

    def norm(self, expr, dim=None):
        """one row: the Euclidean norm of the expression's (first `dim`) components"""
        e = self._cut(expr, dim)
        if not 1 <= e.n <= MAX_NORM:
            raise ValueError(f"a norm over {e.n} components (1 .. {MAX_NORM})")
        return self._add(OP_NORM, 1, e.n, e.terms)

    def subquat(self, a, b, coef=1.0):
        """three rows: coef * mju_subQuat(a, b); a and b are quat(...) or mocap_quat(...)"""
        for e in (a, b):
            if not (isinstance(e, Expr) and e.n == 4 and len(e.terms) == 1 and e.terms[0][1] in (SRC_QUAT, SRC_MOCAP_QUAT) and e.terms[0][4] == 0
                    and e.terms[0][0] == 1.0):
                raise ValueError("subquat takes two whole quaternion sources")
        ta, tb = a.terms[0], b.terms[0]
        return self._add(OP_SUBQUAT, 3, 4, [(float(coef),) + ta[1:], (1.0,) + tb[1:]])

    # ---- the task
    def encode(self, num_parameter=0):
        """(int_data, dbl_data) as include/mjpc_hip.h describes them"""
        nterm = sum(len(b[3]) for b in self.blocks)
        if not 1 <= len(self.blocks) <= MAX_BLOCKS or nterm > MAX_TERMS:
            raise ValueError(f"{len(self.blocks)} blocks / {nterm} terms (caps {MAX_BLOCKS} / {MAX_TERMS})")
        ints = [TBL_VERSION, len(self.blocks), nterm]
        recs, coefs, pool = [], [], []
        row = 0
        for op, dim, ncomp, terms in self.blocks:
            ints += [op, row, dim, ncomp, len(coefs), len(terms)]
            row += dim
            for c, kind, ty, i, off, v in terms:
                need = 4 if op == OP_SUBQUAT else ncomp
                if kind == SRC_CONST:
                    ty, i = int(v.size), nterm + len(pool)
                    pool += [float(x) for x in v]
                if kind == SRC_TOUCH:      # the zone's size[3] goes to the constant pool, the record's off is its address
                    off = nterm + len(pool)
                    pool += [float(x) for x in v]
                if kind == SRC_PARAM and off + need > num_parameter:
                    raise IndexError(f"parameters [{off}, {off + need}) of {num_parameter}")
                coefs.append(float(c)); recs += [kind, ty, i, off]
        return np.array(ints + recs, np.int32), np.array(coefs + pool, float)

    def task(self, terms, parameters=(), risk=0.0, traces=()):
        """terms: the cost table, (dim, norm, weight, [norm parameters]) per term, covering the table's rows"""
        if sum(t[0] for t in terms) != self.rows:
            raise ValueError(f"the cost terms cover {sum(t[0] for t in terms)} residual rows, the table writes {self.rows}")
        ints, dbls = self.encode(len(parameters))
        return make_task(TASK_TABLE, terms, parameters=parameters, risk=risk, traces=traces, int_data=list(ints), dbl_data=list(dbls))

    def measurement(self, parameters=(), traces=()):
        """a task whose rows are only sensors (the estimators' measurement model, mujoco_mpc_amd/estimators.py): the cost table is one
        quadratic term of weight 0 over all rows"""
        return self.task([(self.rows, 0, 0.0, [])], parameters=parameters, traces=traces)


# ---------------------------------------------------------------------------------------- registry tasks restated as tables
def _cost_of(task):
    """(terms, parameters, risk, traces) of a make_task dict: the twin keeps the built-in task's cost table"""
    terms, p = [], 0
    for k in range(int(task["num_term"])):
        n = int(task["num_norm_parameter"][k])
        terms.append((int(task["dim_norm_residual"][k]), int(task["norm"][k]), float(task["weight"][k]), [float(x) for x in task["norm_parameter"][p:p + n]]))
        p += n
    traces = [(int(a), int(b)) for a, b in zip(task["trace_objtype"], task["trace_objid"])]
    return dict(terms=terms, parameters=[float(x) for x in task["parameters"]], risk=float(task["risk"]), traces=traces)


def _twin(gen, fill, **kw):
    m, task, d = gen(**kw)
    t = ResidualTable(m)
    fill(t, m, [int(x) for x in task["int_data"]])
    return m, t.task(**_cost_of(task)), d


def cartpole():
    """cartpole.cc:36-49; cos(q_pole) - 1 is the z component of the pole's z axis minus 1 (the hinge turns about y)"""
    def fill(t, m, I):
        t.sum(t.zaxis("xbody", "pole_1")[2] - 1.0)
        t.sum(t.qpos()[0] - t.param(0))
        t.sum(t.qvel()[1])
        t.sum(t.ctrl()[0])
    return _twin(T.cartpole, fill)


def particle():
    """rollout_test.cc:40-60: the residual copies the state"""
    def fill(t, m, I):
        t.sum(t.qpos()); t.sum(t.qvel())
    return _twin(T.particle, fill, copystate=True)


def particle_fixed():
    """particle.cc:68-73: tip - mocap goal (xy), tip velocity (xy), control"""
    def fill(t, m, I):
        t.sum(t.pos("site", "tip") - t.mocap_pos(0), dim=2)
        t.sum(t.linvel("site", "tip"), dim=2)
        t.sum(t.ctrl())
    return _twin(T.particle_task, fill, fixed=True)


def walker():
    """walker.cc:39-57"""
    def fill(t, m, I):
        t.sum(t.ctrl())
        t.sum(t.pos("xbody", "torso")[2] - t.param(0))
        t.sum(t.zaxis("xbody", "torso")[2] - 1.0)
        t.sum(t.subtree_linvel("torso")[0] - t.param(1))
    return _twin(T.walker, fill)


def acrobot():
    """acrobot.cc:34-49: target - tip (z, x), joint velocities, control"""
    def fill(t, m, I):
        d = t.pos("site", "target") - t.pos("site", "tip")
        t.sum(d[2]); t.sum(d[0]); t.sum(t.qvel()[:2]); t.sum(t.ctrl()[0])
    return _twin(T.acrobot, fill)


def swimmer():
    """swimmer.cc:33-46: control, nose - target in the plane"""
    def fill(t, m, I):
        t.sum(t.ctrl())
        t.sum(t.pos("geom", "nose") - t.mocap_pos(0), dim=2)
    return _twin(T.swimmer, fill)


def fingers():
    """fingers.cc:31-62: finger - object (framepos of the bodies), distances of the object's sites to their targets, control"""
    def fill(t, m, I):
        t.sum(t.pos("body", I[0]) - t.pos("body", I[2]))
        t.sum(t.pos("body", I[1]) - t.pos("body", I[2]))
        for k in range(3):
            t.norm(t.pos("site", I[3 + k]) - t.pos("site", I[6 + k]))
        t.sum(t.ctrl())
    return _twin(T.fingers, fill)


def quadrotor():
    """quadrotor.cc:37-60: position - goal, linear and angular velocity, control - hover thrust; the last two declared rows are
    never written by the reference (zeros here)"""
    def fill(t, m, I):
        g = float(np.sqrt(np.sum(np.asarray(m["gravity"], float) ** 2)))
        thrust = (float(m["body_mass"][0]) + float(m["body_mass"][1])) * g / m["nu"]
        t.sum(t.pos("body", I[0]) - t.mocap_pos(0))
        t.sum(t.linvel("body", I[0]))
        t.sum(t.angvel("body", I[0]))
        t.sum(t.ctrl() - thrust)
        t.zeros(2)
    return _twin(T.quadrotor, fill)


def quadruped_hill():
    """quadruped.cc:726-768: trunk height over the feet - goal, trunk - goal position, trunk - goal orientation (matrices), control"""
    def fill(t, m, I):
        feet = 0.25 * (t.pos("site", I[1]) + t.pos("site", I[2]) + t.pos("site", I[3]) + t.pos("site", I[4]))
        t.sum(t.pos("xbody", I[0])[2] - feet[2] - t.param(0))
        t.sum(t.pos("xbody", I[0]) - t.mocap_pos(0))
        t.sum(t.mat("xbody", I[0]) - t.mocap_mat(0))
        t.sum(t.ctrl())
    return _twin(T.quadruped_hill, fill)


def humanoid_stand():
    """stand.cc:41-94: head height over the feet - goal, capture point against the feet (norm, xy), com velocity xy, joint
    velocities, control"""
    def fill(t, m, I):
        feet = 0.25 * (t.pos("site", I[0]) + t.pos("site", I[1]) + t.pos("site", I[2]) + t.pos("site", I[3]))
        t.sum(t.pos("body", I[4])[2] - feet[2] - t.param(0))
        t.norm(feet - t.subtree_com(I[5]) - 0.2 * t.subtree_linvel(I[5]), dim=2)
        t.sum(t.subtree_linvel(I[5]), dim=2)
        t.sum(t.qvel()[6:])
        t.sum(t.ctrl())
    return _twin(T.humanoid_stand, fill)


def _hand(gen, width):
    def fill(t, m, I):
        site, cube, goal, key = I
        t.sum(t.pos("body", cube) - t.pos("site", site))
        t.subquat(t.quat("body", goal), t.quat("body", cube))
        t.sum(t.linvel("body", cube))
        t.sum(t.actuator_force())
        t.sum(t.qpos()[7:7 + width] - t.key_qpos(key)[7:7 + width])
        t.sum(t.qvel()[6:6 + width])
    return _twin(gen, fill)


def shadow_hand():
    """hand.cc:37-84 (26-wide slices)"""
    return _hand(T.shadow_hand, 26)


def allegro():
    """allegro.cc:36-77 (16-wide slices)"""
    return _hand(T.allegro, 16)


def op3(mode=0):
    """op3/stand.cc:34-152, the rows of the mode (0 Stand, 1 Handstand)"""
    def fill(t, m, I):
        mode_, head, lf, rf, lh, rh, torso, body = I
        nu = m["nu"]
        z = [0.0, 0.0, 1.0]
        feet = 0.5 * (t.pos("site", lf) + t.pos("site", rf))
        if mode_ == 0:
            t.sum(t.pos("site", head)[2] - feet[2] - t.param(0))
            support = feet
        else:
            t.sum(feet[2] - 0.5 * (t.pos("site", lh)[2] - t.pos("site", rh)[2]) - t.param(0))
            support = 0.5 * (t.pos("site", lh) + t.pos("site", rh))
        t.norm(support - t.subtree_com(body) - 0.05 * t.subtree_linvel(body), dim=2)
        t.sum(t.subtree_linvel(body), dim=2)
        t.sum(t.ctrl() - t.key_qpos(mode_)[7:7 + nu])
        if mode_ == 0:
            t.sum(0.1 * (t.zaxis("site", rf) - z)); t.sum(0.1 * (t.zaxis("site", lf) - z))
            t.sum(t.zaxis("site", torso)[2] - 1.0)
            t.zeros(6)
        else:
            t.sum(0.1 * (t.yaxis("site", rh) - z)); t.sum(0.1 * (t.yaxis("site", lh) + z))
            t.sum(0.1 * (t.zaxis("site", rf) + z)); t.sum(0.1 * (t.zaxis("site", lf) + z))
            t.sum(t.zaxis("site", torso)[2] + 1.0)
        t.sum(t.qvel()[6:])
    return _twin(T.op3, fill, mode=mode)


def op3_handstand():
    return op3(mode=1)


TABLE_TASKS = dict(cartpole=cartpole, particle=particle, particle_fixed=particle_fixed, walker=walker, acrobot=acrobot, swimmer=swimmer,
                   fingers=fingers, quadrotor=quadrotor, quadruped_hill=quadruped_hill, humanoid_stand=humanoid_stand,
                   shadow_hand=shadow_hand, allegro=allegro, op3=op3, op3_handstand=op3_handstand)
