"""Record the bit patterns that tests/test_row_broadcast_bits.py pins: outputs of the register L^T D L hooks (tests/hip/ldl_hooks.hip)
and of small rollouts, as uint64 views of the doubles, into tests/golden/row_broadcast/bits.npz.

Run it on the GPU with the libraries of the commit whose bits are to be kept (the parent of a change that must not move them):
    python tools/record_ldl_bits.py [output.npz]
The test imports the case lists and runners below, so recorder and test always feed the same inputs.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "row_broadcast", "bits.npz")

LDL_NS = (18, 27, 33)
LDL_SEEDS = 8

# (key, generator, generator kwargs, debug knobs, candidates, steps, spline points, sigma)
ROLLOUT_CASES = (
    ("quadruped", "quadruped", {}, (), 8, 12, 3, 0.04),                               # in contact from step 0: Newton iterations, elliptic cones, cone job
    ("quadruped_dense_tier", "quadruped", {}, (("tier", "B"),), 8, 12, 3, 0.04),      # two candidates per CU
    ("quadruped_dense_factor", "quadruped", {}, (("dense_factor", "1"),), 8, 12, 3, 0.04),   # dense elimination order
    ("humanoid_track", "humanoid_track", {}, (), 4, 8, 3, 0.15),
    ("shadow_hand", "shadow_hand", {}, (), 4, 6, 3, 0.1),
    ("swimmer_implicit", "swimmer", {"integrator": 2}, (), 4, 10, 3, 0.3),            # LU path of the full implicit integrator
)


def dof_parents(n):
    """elimination-tree parents of the model with n dofs (csrc/model.h DofTree<n>)"""
    from mujoco_mpc_amd.modelgen import humanoid_track, quadruped, shadow_hand
    m = (quadruped() if n == 18 else (humanoid_track() if n == 27 else shadow_hand()))[0]
    par = [int(p) for p in m["dof_parentid"]]
    if n == 33:
        par[9] = 8          # the cube's free joint is the hub above the wrist
    return par


def ldl_system(n, tree, seed, par):
    """seeded SPD matrix and right-hand side; tree = 1: the pattern of the joint-space inertia (ancestors only), tree = 0: full"""
    rng = np.random.default_rng(1000 * n + 10 * seed + tree)
    A = np.zeros((n, n))
    if tree:
        for i in range(n):
            a = i
            while a >= 0:
                A[i, a] = A[a, i] = rng.normal()
                a = par[a]
    else:
        A = rng.normal(size=(n, n))
        A = A + A.T
    A[np.arange(n), np.arange(n)] = np.abs(A).sum(1) + 1.0       # SPD by diagonal dominance, pattern kept
    return np.ascontiguousarray(A), rng.normal(size=n)


def load_hooks(path=None):
    import __graft_entry__ as g
    lib = C.CDLL(path or g.TESTHOOKS_SO)
    dp = C.POINTER(C.c_double)
    lib.mjpc_hip_debug_ldl.argtypes = [C.c_int, C.c_int, dp, dp, dp, C.c_int]
    return lib


def run_ldl(lib, n, tree, par):
    """(LDL_SEEDS, 2 n) uint64: fused and split factor + solve of every seeded system"""
    dp = C.POINTER(C.c_double)
    outs = np.zeros((LDL_SEEDS, 2 * n))
    for seed in range(LDL_SEEDS):
        A, b = ldl_system(n, tree, seed, par)
        rc = lib.mjpc_hip_debug_ldl(n, tree, A.ctypes.data_as(dp), b.ctypes.data_as(dp), outs[seed].ctypes.data_as(dp), 0)
        if rc != 0:
            raise RuntimeError(f"mjpc_hip_debug_ldl({n}, {tree}) returned {rc}")
    return outs.view(np.uint64)


def run_rollout(case, set_knob):
    """returns / failure / winner's states of one small plan, as uint64 (failure as int32); set_knob(name, value) sets a debug knob"""
    from mujoco_mpc_amd import modelgen
    from mujoco_mpc_amd.planner import HipBackend
    key, gen, gkw, knobs, N, H, P, sigma = case
    m, task, d = getattr(modelgen, gen)(**gkw)
    for name, value in knobs:
        set_knob(name, value)
    kt = np.linspace(0, (H - 1) * m["timestep"], P)
    kv = np.tile(np.asarray(d["ctrl0"], dtype=float), (P, 1)) if "ctrl0" in d else np.zeros((P, m["nu"]))
    mocap = d["mocap"] if d.get("mocap") is not None and len(d["mocap"]) else None
    be = HipBackend(m, task, max_samples=N, max_horizon=H)
    out = be.plan(state=d["state"], mocap=mocap, time=0.0, knot_times=kt, knot_values=kv, interpolation=2, num_trajectory=N,
                  horizon=H, sigma=(sigma, 0.0), seed=0x5EED, stream=3)
    dense_used = be.dense_tier()[1]
    be.close()
    return dict(returns=out["returns"].view(np.uint64).copy(), failure=out["failure"].astype(np.int32),
                states=np.ascontiguousarray(out["states"]).view(np.uint64).copy(), winner=np.int64(out["winner"])), dense_used


def main():
    from mujoco_mpc_amd import capi
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    rec = {}
    lib = load_hooks()
    for n in LDL_NS:
        par = dof_parents(n)
        for tree in (0, 1):
            rec[f"ldl_{n}_{tree}"] = run_ldl(lib, n, tree, par)
    for case in ROLLOUT_CASES:
        touched = []

        def set_knob(name, value):
            touched.append(name)
            capi.debug_set(name, value)
        try:
            r, dense_used = run_rollout(case, set_knob)
        finally:
            for name in touched:
                capi.debug_set(name, None)
        for k, v in r.items():
            rec[f"rollout_{case[0]}_{k}"] = v
        print(f"{case[0]}: winner {int(r['winner'])} failures {int(r['failure'].astype(bool).sum())} dense tier used {dense_used} "
              f"returns {r['returns'].view(np.float64)[:3]}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **rec)
    print(f"wrote {path}: {len(rec)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
