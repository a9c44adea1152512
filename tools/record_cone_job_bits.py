"""Record the bit patterns that tests/test_gpu_cone_job_bits.py pins: small plans on the models whose Newton iterates post the cone-block
job to the worker waves (csrc/solver_reg.h, worker_job), as uint64 views of the doubles, into tests/golden/cone_job/bits.npz.

Run it on the GPU with the library of the commit whose bits are to be kept (the parent of a change that must not move them):
    python tools/record_cone_job_bits.py [output.npz]
The test imports the case list and the runner below, so recorder and test always feed the same inputs.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "cone_job", "bits.npz")

# (key, generator, generator kwargs, candidates, steps, spline points, sigma, lift of the root body [m], plans in one process)
CASES = (
    # 33 dofs, the direct flavour: the cube on the palm and a finger, rows of 8 to 14 columns (beyond the 10 a worker keeps in
    # registers).  Only 2 contacts in these 6 steps: far fewer than 128 (contact, row) pairs, see quadruped_pressed for those
    ("hand_elliptic", "shadow_hand", {"cone": 1}, 4, 6, 3, 0.1, 0.0, 1),
    # 18 dofs with condim-6 contacts and dims below 6 next to them (floor: 3): the thin box pinched by the two fingers
    ("fingers_condim6", "fingers", {"noslip_iterations": 0, "grasp": True}, 4, 10, 3, 0.04, 0.0, 1),
    # the A1 dropped from 4 cm: steps without a contact (nefc = 0: nothing is built, the workers are only released), the first
    # touch-down, steps whose iterates go back and forth between having and not having a contact in its cone zone
    ("quadruped_drop", "quadruped", {}, 4, 30, 3, 0.04, 0.04, 1),
    # the A1 pressed 15 cm into the floor: trunk, thighs and calves touch as well, 24 contacts of 6 to 9 dofs each, i.e. more than 128
    # (contact, row) pairs, so worker 0 has a second pass (which reads LDS) behind its first (from registers)
    ("quadruped_pressed", "quadruped", {}, 4, 20, 3, 0.04, -0.15, 1),
    # the headline flavour, three plans in one process: the same bits every time
    ("quadruped_repeat", "quadruped", {}, 8, 12, 3, 0.04, 0.0, 3),
)
KEYS = ("returns", "failure", "states", "winner")


def run_case(case):
    """list (one entry per plan of the process) of dict(returns, failure, states, winner as recorded; diag [N, 4] int32: summed Newton
    iterations, most contacts, most rows, warnings of every candidate)"""
    from mujoco_mpc_amd import modelgen
    from mujoco_mpc_amd.planner import HipBackend
    key, gen, gkw, N, H, P, sigma, lift, plans = case
    m, task, d = getattr(modelgen, gen)(**gkw)
    state = np.array(d["state"], dtype=float)
    state[2] += lift
    kt = np.linspace(0, (H - 1) * m["timestep"], P)
    kv = np.tile(np.asarray(d["ctrl0"], dtype=float), (P, 1)) if "ctrl0" in d else np.zeros((P, m["nu"]))
    mocap = d["mocap"] if d.get("mocap") is not None and len(d["mocap"]) else None
    be = HipBackend(m, task, max_samples=N, max_horizon=H)
    outs = []
    for _ in range(plans):
        out = be.plan(state=state, mocap=mocap, time=0.0, knot_times=kt, knot_values=kv, interpolation=2, num_trajectory=N,
                      horizon=H, sigma=(sigma, 0.0), seed=0x5EED, stream=3)
        diag = be.fetch_all(N, H, P)["diag"]
        outs.append(dict(returns=out["returns"].view(np.uint64).copy(), failure=out["failure"].astype(np.int32),
                         states=np.ascontiguousarray(out["states"]).view(np.uint64).copy(), winner=np.int64(out["winner"]),
                         diag=diag.copy()))
    be.close()
    return outs


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    rec = {}
    for case in CASES:
        outs = run_case(case)
        r = outs[0]
        for o in outs[1:]:
            for k in KEYS:
                if not np.array_equal(o[k], r[k]):
                    raise RuntimeError(f"{case[0]}: {k} differs between two plans of one process")
        for k in KEYS:
            rec[f"{case[0]}_{k}"] = r[k]
        print(f"{case[0]}: winner {int(r['winner'])} failures {int(r['failure'].astype(bool).sum())} Newton iterations {r['diag'][:, 0].tolist()} "
              f"most contacts {r['diag'][:, 1].tolist()} returns {r['returns'].view(np.float64)[:3]}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **rec)
    print(f"wrote {path}: {len(rec)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
