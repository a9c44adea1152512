"""Record the bit patterns that tests/test_gpu_presolve_split_bits.py pins: small plans that walk every path of the pre-solve
window (contact rows, their Jacobian and impedance on the owner wave; smooth dynamics, inertia and contact-free rows on the other
three, csrc/core.h), as uint64 views of the doubles, into tests/golden/presolve_split/bits.npz.

Run it on the GPU with the library of the commit whose bits are to be kept (the parent of a change that must not move them):
    python tools/record_presolve_bits.py [output.npz]
The test imports the case list and the runner below, so recorder and test always feed the same inputs.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "presolve_split", "bits.npz")

# (key, generator, generator kwargs, model overrides, debug knobs, candidates, steps, spline points, sigma, lift of the root body [m])
CASES = (
    # the A1 dropped from 2 cm: steps with ncon = 0 (a wave with an empty share still posts its flag), then the feet touch down one
    # after the other
    ("a1_drop", "quadruped", {}, {}, (), 8, 12, 3, 0.04, 0.02),
    # the A1 standing (the headline's start): 8 contacts in its first 12 steps
    ("a1_stand", "quadruped", {}, {}, (), 8, 12, 3, 0.04, 0.0),
    # the A1 pressed into the floor, trunk, thighs and calves touch as well: the headline's 14 contacts and more, odd counts, several
    # 64-lane trips of Jacobian elements for either wave
    ("a1_pressed", "quadruped", {}, {}, (), 4, 12, 3, 0.04, -0.15),
    # contact buffer too small for the standing A1 (4 to 6 contacts in these steps): WARN_CONTACTFULL
    ("a1_contactfull", "quadruped", {}, {"nconmax": 4}, (), 4, 6, 3, 0.04, 0.0),
    # row buffer too small (36 to 42 rows in these steps): WARN_CNSTRFULL, raised by the contact rows' layout, which cuts ncon back
    ("a1_cnstrfull", "quadruped", {}, {"nefcmax": 40}, (), 4, 6, 3, 0.04, 0.0),
    # pyramidal cones, 27 dofs: 2 (dim - 1) rows per contact
    ("humanoid_pyramidal", "humanoid_track", {}, {}, (), 4, 8, 3, 0.15, 0.0),
    # every geom of the A1 with condim 1: one row per contact, no friction rows in the contact pass
    ("a1_frictionless", "quadruped", {}, {"geom_condim": 1}, (), 4, 10, 3, 0.04, 0.0),
    # connect equalities: the contact-free rows wait for the com-based quantities
    ("linkage_connect", "linkage", {}, {}, (), 4, 12, 3, 0.3, 0.0),
    # activation states (na > 0): act_dot and the force from the activation
    ("filter_arm_stateful", "filter_arm", {}, {}, (), 4, 12, 3, 0.3, 0.0),
    # 9 dofs: the generic-nv kernel
    ("walker_generic_nv", "walker", {}, {}, (), 4, 12, 3, 0.5, 0.0),
    # the spill flavour: rows, contacts and the efc vectors in the HBM slab
    ("a1_spill", "quadruped", {}, {}, (("spill", "all"),), 4, 10, 3, 0.04, 0.0),
    # the dense tier: two candidates per CU
    ("a1_dense_tier", "quadruped", {}, {}, (("tier", "B"),), 8, 12, 3, 0.04, 0.0),
)
KEYS = ("returns", "failure", "states", "winner", "sum_iter")


def run_case(case, set_knob):
    """dict(returns, failure, states, winner, sum_iter as recorded; diag [N, 4] int32: summed Newton iterations, most contacts, most
    rows, warnings of every candidate; dense_used, spill_bytes); set_knob(name, value) sets a debug knob"""
    from mujoco_mpc_amd import modelgen
    from mujoco_mpc_amd.planner import HipBackend
    key, gen, gkw, over, knobs, N, H, P, sigma, lift = case
    m, task, d = getattr(modelgen, gen)(**gkw)
    m = dict(m)
    for name, value in over.items():
        m[name] = np.full_like(np.asarray(m[name]), value) if np.ndim(m[name]) else value
    for name, value in knobs:
        set_knob(name, value)
    state = np.array(d["state"], dtype=float)
    state[2] += lift
    kt = np.linspace(0, (H - 1) * m["timestep"], P)
    kv = np.tile(np.asarray(d["ctrl0"], dtype=float), (P, 1)) if "ctrl0" in d else np.zeros((P, m["nu"]))
    mocap = d["mocap"] if d.get("mocap") is not None and len(d["mocap"]) else None
    be = HipBackend(m, task, max_samples=N, max_horizon=H)
    out = be.plan(state=state, mocap=mocap, time=0.0, knot_times=kt, knot_values=kv, interpolation=2, num_trajectory=N,
                  horizon=H, sigma=(sigma, 0.0), seed=0x5EED, stream=3)
    diag = be.fetch_all(N, H, P)["diag"].copy()
    dense_used, spill_bytes = be.dense_tier()[1], be.spill_bytes()
    be.close()
    return dict(returns=out["returns"].view(np.uint64).copy(), failure=out["failure"].astype(np.int32),
                states=np.ascontiguousarray(out["states"]).view(np.uint64).copy(), winner=np.int64(out["winner"]),
                sum_iter=diag[:, 0].astype(np.int64).view(np.uint64).copy(), diag=diag, dense_used=dense_used, spill_bytes=spill_bytes)


def main():
    from mujoco_mpc_amd import capi
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    rec = {}
    for case in CASES:
        touched = []

        def set_knob(name, value):
            touched.append(name)
            capi.debug_set(name, value)
        try:
            r = run_case(case, set_knob)
        finally:
            for name in touched:
                capi.debug_set(name, None)
        for k in KEYS:
            rec[f"{case[0]}_{k}"] = r[k]
        rec[f"{case[0]}_diag"] = r["diag"]
        print(f"{case[0]}: winner {int(r['winner'])} failure {r['failure'].tolist()} dense tier used {r['dense_used']} slab bytes {r['spill_bytes']} Newton iterations "
              f"{r['diag'][:, 0].tolist()} most contacts {r['diag'][:, 1].tolist()} most rows {r['diag'][:, 2].tolist()} "
              f"returns {r['returns'].view(np.float64)[:3]}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **rec)
    print(f"wrote {path}: {len(rec)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
