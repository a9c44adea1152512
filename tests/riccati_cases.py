"""Inputs of the iLQG backward-pass tests (TEST INFRASTRUCTURE ONLY), shared by the CPU tier (emulation, host C++, mirror) and the GPU tier."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ilqg_backward_pass_lqr.json")
# (nd, nu, T): a single control; T = 2 is a single step; the filter_arm dimensions (na > 0); the A1; the humanoid (no multiple of 16 or 64)
SHAPES = [(2, 1, 3), (4, 1, 8), (4, 2, 2), "filter_arm", (36, 12, 5), (54, 21, 4)]
REG_TYPES = [0, 1, 2, 3]
OUT_KEYS = ("k", "K", "Vx", "Vxx", "Qx", "Qu", "Qxx", "Qxu", "Quu", "dV")


def shape(s):
    if s == "filter_arm":
        import transition_cases as tc
        import transition_mirror as tm
        m, task, _ = tc.model("filter_arm")
        dd = tm.dims(m, task)
        return 2 * dd["nv"] + dd["na"], dd["nu"], 5
    return s


def trajectory(nd, nu, T, seed=0, box=0.6):
    """A, B unit normals scaled by 1 / sqrt(nd); cost Hessians J'J / nr of a random Jacobian with more rows than columns (positive definite);
    actions inside +-0.5 and limits +-box: with box 0.6 some controls clamp and some stay free"""
    rng = np.random.default_rng(7000 + 131 * nd + 17 * nu + T + 1000 * seed)
    n = nd + nu; nr = n + 2
    A = rng.standard_normal((T - 1, nd, nd)) / np.sqrt(nd); B = rng.standard_normal((T - 1, nd, nu)) / np.sqrt(nd)
    J = rng.standard_normal((T, nr, n))
    Hm = np.einsum("tri,trj->tij", J, J) / nr
    g = rng.standard_normal((T, n))
    c = dict(A=A, B=B, cx=np.ascontiguousarray(g[:, :nd]), cu=np.ascontiguousarray(g[:, nd:]), cxx=np.ascontiguousarray(Hm[:, :nd, :nd]),
             cxu=np.ascontiguousarray(Hm[:, :nd, nd:]), cuu=np.ascontiguousarray(Hm[:, nd:, nd:]))
    c["cu"][T - 1] = 0.0; c["cxu"][T - 1] = 0.0; c["cuu"][T - 1] = 0.0          # the terminal knot has no control
    c["actions"] = rng.uniform(-0.5, 0.5, (T, nu))
    c["action_limits"] = np.tile([-box, box], (nu, 1)).astype(float)
    return c


def lqr():
    """the reference's fixture: (inputs as trajectory()'s, expected dict, tolerance)"""
    with open(GOLDEN) as f:
        gd = json.load(f)
    n, m, T = gd["n"], gd["m"], gd["T"]
    A = np.array(gd["A"], float); B = np.array(gd["B"], float).reshape(n, m); u = np.array(gd["u"], float).reshape(T - 1, m)
    x = np.zeros((T, n)); x[0] = gd["x0"]
    for t in range(T - 1):
        x[t + 1] = A @ x[t] + B @ u[t]
    c = dict(A=np.tile(A, (T - 1, 1, 1)), B=np.tile(B, (T - 1, 1, 1)), cx=x.copy(), cu=np.vstack([u, np.zeros((1, m))]), cxx=np.tile(np.eye(n), (T, 1, 1)),
             cxu=np.zeros((T, n, m)), cuu=np.tile(np.eye(m), (T, 1, 1)), actions=np.vstack([u, np.zeros((1, m))]),
             action_limits=np.array(gd["action_limits"], float))
    c["cuu"][T - 1] = 0.0
    exp = dict(Vx=np.array(gd["Vx"]).reshape(T, n), Vxx=np.array(gd["Vxx"]).reshape(T, n, n), K=np.array(gd["feedback_gain"]).reshape(T - 1, m, n),
               k=np.array(gd["action_improvement"]).reshape(T - 1, m))
    return c, exp, gd["tolerance"], gd["regularization"]


def failing_knot(nd=4, nu=2, T=6, knot=2, depth=10.0):
    """a trajectory whose cuu at `knot` is -depth I, with B = 0 and cxu = 0 there: Quu = -depth I, so under control regularisation the step
    at that knot fails exactly while regularization <= depth.  From (1, 1) with factor 2: 1, 2 and 8 fail, 64 passes"""
    c = trajectory(nd, nu, T, seed=3)
    c["cuu"][knot] = -depth * np.eye(nu); c["cxu"][knot] = 0.0; c["B"][knot] = 0.0
    return c, knot


def boxqp_problem(n, seed):
    """the issue's draw order"""
    rng = np.random.default_rng(100 * n + seed)
    M = rng.standard_normal((n, n))
    H = M @ M.T + n * np.eye(n)
    g = 3 * n * rng.standard_normal(n)
    lower = -rng.uniform(0.2, 1, n)
    upper = rng.uniform(0.2, 1, n)
    return H, g, lower, upper
