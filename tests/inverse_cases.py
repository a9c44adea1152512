"""Cases and bars of the inverse-dynamics tests (TEST INFRASTRUCTURE ONLY), shared by the CPU tier (tests/test_inverse.py, the emulation)
and the GPU tier (tests/test_gpu_inverse.py): the models, tables and states of tests/late_cases.py, five rows each, with a seeded
acceleration per row.

The bars: ten times the largest deviation of the EMULATION from tests/inv_ref.py (residual rows: tests/acc_ref.py through
tests/late_checks.py) relative to max(1, |entry|), measured on the CPU (tests/test_inverse.py prints each figure), shared by both tiers.
Never derived from device output.  A measured 0.0 is a bit-equal case: its bar is 0.
"""
import functools
import math

import numpy as np

import late_cases as lc

KINEMATIC = list(lc.KINEMATIC)
CONTACT = list(lc.TOUCH)
CASES = KINEMATIC + CONTACT
ROWS = 5
DAMPED = "chain3_euler"                     # the round trip's model with damping for the continuous / discrete comparison

# measured on the CPU: emulation against inv_ref, relative to max(1, |entry|); bars = ten times that
# forces: qfrc_inverse and qfrc_constraint against inv_ref; residual: the rows against acc_ref at the given acceleration
FORCE_MEASURED = {"chain3_euler": 3.2e-16, "chain3_implicitfast": 4.1e-16, "sphere": 1.5e-15, "filter_arm": 3.7e-16, "particle_imu": 1.4e-17,
                  "twoball_elliptic": 1.1e-15, "twoball_pyramidal": 5.3e-15, "quadruped_elliptic": 2.8e-13, "quadruped_pyramidal": 2.4e-13}
RESIDUAL_MEASURED = {"chain3_euler": 2.7e-15, "chain3_implicitfast": 2.8e-15, "sphere": 8.9e-15, "filter_arm": 7.2e-16, "particle_imu": 0.0,
                     "twoball_elliptic": 8.1e-16, "twoball_pyramidal": 2.8e-16, "quadruped_elliptic": 2.4e-14, "quadruped_pyramidal": 6.3e-14}
# round trip (discrete = 1 at a forward step's (v' - v) / h): qfrc_inverse against DynRef's actuator force, qfrc_constraint against
# A a_d - (tau - c) and the emulated forward step's own, the QACC rows against the reference's converted acceleration.  Bounded by the forward solver's convergence at con_cases.TOLERANCE: the elliptic cases stop at a gradient of 1e-6
ROUNDTRIP_MEASURED = {"chain3_euler": 3.1e-15, "chain3_implicitfast": 4.0e-15, "sphere": 1.1e-13, "filter_arm": 9.3e-15, "particle_imu": 5.6e-17,
                      "twoball_elliptic": 2.1e-06, "twoball_pyramidal": 1.7e-13, "quadruped_elliptic": 1.5e-06, "quadruped_pyramidal": 2.1e-13}
# FD blocks at FD_EPS, one-sided and centred, T = 1 (chain3_euler: and T = 3): the six blocks against the same differences over the
# references, measured on the block itself (not divided back by eps); FD_MASS: DfDa against DynRef.mass_matrix and the QACC block of DsDa
# against the identity on the contact-free models
FD_MEASURED = {"chain3_euler": 7.1e-09, "chain3_implicitfast": 5.3e-09, "sphere": 2.1e-08, "filter_arm": 6.9e-09, "particle_imu": 0.0,
               "twoball_elliptic": 1.7e-07, "twoball_pyramidal": 9.8e-08, "quadruped_elliptic": 5.7e-08, "quadruped_pyramidal": 5.7e-08}
ZOO_MEASURED = 4.3e-13                   # forces of con_cases' zoo, whose actuators include two site transmissions (tests/test_inverse.py::zoo_case)
HUMANOID_SPILL_MEASURED = 7.2e-13         # forces of the humanoid at the spill flavour's capacity (tests/test_inverse.py::humanoid_spill_case)
FD_MASS_MEASURED = {"chain3_euler": 2.7e-10, "chain3_implicitfast": 4.5e-10, "sphere": 2.4e-09, "filter_arm": 2.8e-10, "particle_imu": 8.2e-11}


def bar(table, key):
    return 10 * table[key]


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(model, task, mocap, X, U, T, A, contact, late): `late` is late_cases' own dict cut to the same rows (for late_checks)"""
    contact = name in CONTACT
    c = dict(lc.touch(name) if contact else lc.kinematic(name))
    n = len(c["X"])
    idx = np.arange(ROWS) % n                                  # (the two-ball cases have four states: the fifth row is the first again, with its own acceleration)
    c["X"] = np.array(c["X"])[idx]; c["U"] = np.array(c["U"])[idx]; c["T"] = np.array(c["T"])[idx]
    rng = np.random.default_rng(1000 + CASES.index(name))
    A = rng.uniform(-2.0, 2.0, (ROWS, c["model"]["nv"]))
    A[0] = 0.0                                                 # one row at rest in acceleration
    return dict(model=c["model"], task=c["task"], mocap=c["mocap"], X=c["X"], U=c["U"], T=c["T"], A=A, contact=contact, late=c)


# ---------------------------------------------------------------------------------------------------------------- references
def ref_residual(c, X, U, A):
    """the residual rows [n, nr] an inverse evaluation of case c must report at (X, U) and the continuous acceleration A: the early and
    late blocks of late_cases' table from tests/acc_ref.py (through late_checks), the QACC rows A themselves"""
    import late_checks as lk
    m = c["model"]; late = dict(c["late"]); late["X"] = np.asarray(X, float); late["U"] = np.asarray(U, float)
    n, nv = len(late["X"]), m["nv"]
    res = np.zeros((n, c["task"]["num_residual"]))
    if c["contact"]:
        res[:, :nv] = A
        res[:, nv:] = touch_rows(c, late["X"], np.asarray(A, float))
    else:
        res[:, late["rows"]["qacc"]] = A
        want, _, _ = lk.kinematic_want(late, res)
        for k, w in want.items():
            res[:, late["rows"][k]] = np.asarray(w, float).reshape(n, -1)
    return res


def touch_rows(c, X, A):
    """late_checks.touch_want's rows (one per zone, then |t0 + t1 - 1|) for many states at once: acc_ref.TouchRef's rule with the
    kinematics and Jacobians of DynRef taken for the whole batch in one pass (TouchRef takes them state by state: 0.2 s each on the A1)"""
    from acc_ref import EDGE, NearZone, TouchRef, in_zone
    from dyn_ref import _t
    m = c["model"]; nq, nv = m["nq"], m["nv"]
    ref = _TOUCH_REFS.get(id(m)) or _TOUCH_REFS.setdefault(id(m), TouchRef(m, c["late"]["zones"]))
    con, dyn = ref.con, ref.con.dyn
    q, v = X[:, :nq], X[:, nq:nq + nv]
    fk = dyn.fk(_t(q)); jac = dyn.jacobians(_t(q))
    xpos, xmat, xipos = fk["xpos"].numpy(), fk["xmat"].numpy(), fk["xipos"].numpy()
    sx, sR = fk["site_xpos"].numpy(), fk["site_xmat"].numpy()
    Jp, Jr = jac["Jp"].numpy(), jac["Jr"].numpy()
    out = np.zeros((len(X), len(ref.zones) + 1))
    for i in range(len(X)):
        r = con.rows(q[i], v[i], xpos[i], xmat[i], xipos[i], Jp[i], Jr[i])
        F, _ = con.force(r, r["J"] @ A[i] - r["aref"])
        cons = ref.contacts(xpos[i], xmat[i])
        groups = r["groups"][len(r["groups"]) - len(cons):] if cons else []
        assert len(cons) == r["ncon"] and all(g[0] in ("ell", "pyr", "pos") for g in groups)
        normal = [float(F[k0:k0 + n].sum()) if kind == "pyr" else float(F[k0]) for kind, k0, n, _ in groups]
        for z, (site, shape, size) in enumerate(ref.zones):
            body = int(m["site_bodyid"][site]); tot = 0.0
            for k, (g1, g2, pos) in enumerate(cons):
                if body not in (int(m["geom_bodyid"][g1]), int(m["geom_bodyid"][g2])) or not normal[k] > 0:
                    continue
                inside, edge = in_zone(shape, sR[i, site].T @ (pos - sx[i, site]), size)
                if edge < EDGE:
                    raise NearZone(f"state {i}: a contact point is {edge:.1e} from a zone boundary")
                if inside:
                    tot += normal[k]
            out[i, z] = tot
        out[i, -1] = abs(out[i, 0] + out[i, 1] - 1.0)
    return out


_TOUCH_REFS = {}


def qacc_rows(c):
    return slice(0, c["model"]["nv"]) if c["contact"] else c["late"]["rows"]["qacc"]


def split_table(c, table):
    """(X, U, T, A) of the nudged table rows [state | ctrl | time | qacc]"""
    m = c["model"]; ds, nu = m["nq"] + m["nv"] + m["na"], m["nu"]
    return table[:, :ds], table[:, ds:ds + nu], table[:, ds + nu], table[:, ds + nu + 1:]


def fd_blocks_of(f, s, nv, T, eps, centered):
    """the six blocks from evaluations f [T * E, nv], s [T * E, nr] of a nudged table: the differences the kernels take, in numpy"""
    E = 1 + (6 if centered else 3) * nv
    out = {}
    for bi, bn in enumerate("qva"):
        for y, key in ((f, "Df"), (s, "Ds")):
            blk = np.zeros((T, y.shape[1], nv))
            for t in range(T):
                for j in range(nv):
                    col = bi * nv + j
                    if centered:
                        blk[t, :, j] = (y[t * E + 1 + 2 * col] - y[t * E + 2 + 2 * col]) / (2 * eps)
                    else:
                        blk[t, :, j] = (y[t * E + 1 + col] - y[t * E]) / eps
            out[key + "D" + bn] = blk
    return out


BLOCKS = ("DfDq", "DfDv", "DfDa", "DsDq", "DsDv", "DsDa")
FD_EPS = 1e-6


@functools.lru_cache(maxsize=None)
def fd_reference(name, centered, T=1, first=1):
    """dict(the six blocks, M [T, nv, nv], table) for rows [first, first + T) of the case: differences over inv_ref (forces) and
    ref_residual on the nudged table, which is rebuilt here in numpy from the documented rule and must equal the kernels' bit for bit"""
    import inv_ref as ir
    import transition_mirror as tm
    c = case(name); m = c["model"]; nv = m["nv"]
    sl = slice(first, first + T)
    table = nudged_table(m, c["X"][sl], c["U"][sl], c["T"][sl], c["A"][sl], FD_EPS, centered, tm.dofmap(m))
    X, U, _, A = split_table(c, table)
    ref = ir.InvRef(m)
    w = ir.evaluate(ref, m, X, U, A)
    out = fd_blocks_of(w["qfrc_inverse"], ref_residual(c, X, U, A), nv, T, FD_EPS, centered)
    E = 1 + (6 if centered else 3) * nv
    out["M"] = w["M"][::E]; out["table"] = table
    return out


def _normalize4(q):
    n = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    if n < 1e-15:
        return np.array([1.0, 0, 0, 0])
    return q / n if abs(n - 1) > 1e-15 else q.copy()


def _quat_nudge(q, ax, cs, sn):
    """transition_fd.h's fd_quat_nudge, operation for operation"""
    w, x, y, z = _normalize4(np.asarray(q, float))
    if ax == 0:
        r = [w * cs + -(x * sn), w * sn + x * cs, y * cs + z * sn, z * cs + -(y * sn)]
    elif ax == 1:
        r = [w * cs + -(y * sn), x * cs + -(z * sn), w * sn + y * cs, z * cs + x * sn]
    else:
        r = [w * cs + -(z * sn), x * cs + y * sn, y * cs + -(x * sn), w * sn + z * cs]
    return _normalize4(np.array(r))


def nudged_table(m, X, U, T, A, eps, centered, dofmap):
    """rows [state | ctrl | time | qacc] of mjpc_hip_inverse_fd's evaluation table (csrc/inverse_fd.h), restated in numpy"""
    nq, nv, na, nu = m["nq"], m["nv"], m["na"], m["nu"]; ds = nq + nv + na
    E = 1 + (6 if centered else 3) * nv
    cs, sn = math.cos(0.5 * eps), math.sin(0.5 * eps)          # the host's libm, as the engine's entry point
    rows = []
    for t in range(len(X)):
        for s in range(E):
            x = np.array(X[t], float); a = np.array(A[t], float)
            if s > 0:
                c, sgn = ((s - 1) >> 1, -1.0 if (s - 1) & 1 else 1.0) if centered else (s - 1, 1.0)
                if c < nv:
                    qa, ax = dofmap[c]
                    if ax < 0:
                        x[qa] = x[qa] + sgn * eps
                    else:
                        x[qa:qa + 4] = _quat_nudge(X[t][qa:qa + 4], ax, cs, sgn * sn)
                elif c < 2 * nv:
                    x[nq + c - nv] = x[nq + c - nv] + sgn * eps
                else:
                    a[c - 2 * nv] = a[c - 2 * nv] + sgn * eps
            rows.append(np.concatenate([x, np.asarray(U[t], float).reshape(nu), [T[t]], a]))
    return np.array(rows)
