"""Generates tests/golden/mjcf/tasks.npz: what the MJCF subset loader (modelgen/mjcf.py) reads from the reference's task files,
so that tests/test_mjcf_loader.py checks the hand-authored generators (modelgen/tasks.py) against them without the reference tree.

Per task file: the parsed task information (custom numerics and text, cost terms, trace sensors, sensors, keyframes), the
builder's options and bodies (name, position, mocap flag) and, for the files the tests compile, the compiled model arrays.
Only what the loader derives is stored, never the files themselves.  Regenerate from a checkout of the reference project:
    python tests/golden/make_mjcf_fixtures.py PATH/TO/mujoco_mpc
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "mjcf", "tasks.npz")     # beside, not among, the plan-step fixtures

# task file (relative to mjpc/): (includes that exist upstream only as patches against dm_control / menagerie and are dropped,
# compile the model).  missing_ok None = the humanoid is read from its patch and agent_timestep overrides the time step
# (mjpc/agent.cc), the way the agent loads a complete task.
FILES = {
    "test/testdata/particle_task.xml": (None, True),
    "tasks/humanoid/stand/task.xml": (None, True),
    "tasks/humanoid/walk/task.xml": (None, True),
    "tasks/humanoid/tracking/task.xml": (None, True),
    "tasks/fingers/task.xml": (None, True),
    "tasks/humanoid/interact/task.xml": (("humanoid_modified.xml",), True),
    "tasks/cartpole/task.xml": (("cartpole_modified.xml",), False),
    "tasks/quadruped/task_flat.xml": (("a1_modified.xml",), False),
    "tasks/swimmer/task.xml": (("swimmer_modified.xml",), False),
    "tasks/quadrotor/task.xml": (("quadrotor_modified.xml", "gates.xml"), False),
    "tasks/particle/task_timevarying.xml": (("particle_modified.xml",), False),
}
_LONG = 16      # float lists longer than this (keyframes) are slices of one float64 pool, shorter ones stay in the JSON


def _encode(obj, arrays, pool):
    if isinstance(obj, np.ndarray):
        name = f"a{len(arrays)}"; arrays[name] = obj
        return {"__array__": name}
    if isinstance(obj, dict):
        assert all(isinstance(k, str) for k in obj), list(obj)
        return {k: _encode(v, arrays, pool) for k, v in obj.items()}
    if isinstance(obj, tuple):
        return {"__tuple__": [_encode(v, arrays, pool) for v in obj]}
    if isinstance(obj, list):
        if len(obj) > _LONG and all(type(v) is float for v in obj):
            pool.extend(obj)
            return {"__floats__": [len(pool) - len(obj), len(obj)]}
        return [_encode(v, arrays, pool) for v in obj]
    if isinstance(obj, np.generic):
        return obj.item()
    return obj


def _decode(obj, z):
    if isinstance(obj, dict):
        if "__array__" in obj:
            return z[obj["__array__"]]
        if "__floats__" in obj:
            start, n = obj["__floats__"]
            return z["pool"][start:start + n].tolist()
        if "__tuple__" in obj:
            return tuple(_decode(v, z) for v in obj["__tuple__"])
        return {k: _decode(v, z) for k, v in obj.items()}
    if isinstance(obj, list):
        return [_decode(v, z) for v in obj]
    return obj


def load(path=FIXTURE):
    """{task file: dict(info, opt, bodies=[dict(name, pos, mocap)], model (None where not compiled))}"""
    with np.load(path) as z:
        return _decode(json.loads(str(z["meta"])), z)


def parse(ref, rel):
    sys.path.insert(0, ROOT)
    from mujoco_mpc_amd.modelgen import mjcf
    mjpc = os.path.join(ref, "mjpc")
    missing, compiled = FILES[rel]
    if missing is None:
        def reader(p):
            if os.path.basename(p) == "humanoid_modified.xml":       # exists upstream only as dm_control's file + this patch
                return mjcf.read_patch_new_file(os.path.join(mjpc, "tasks/humanoid/humanoid.xml.patch"))
            with open(p) as f:
                return f.read()
        b, info = mjcf.parse_mjcf(os.path.join(mjpc, rel), reader=reader)
        b.opt["timestep"] = info["numeric"].get("agent_timestep", [b.opt["timestep"]])[0]
    else:
        b, info = mjcf.parse_mjcf(os.path.join(mjpc, rel), missing_ok=missing)
    bodies = [dict(name=bd.name, pos=tuple(float(x) for x in bd.pos), mocap=bool(bd.mocap)) for bd in b.bodies]
    return dict(info=info, opt=dict(b.opt), bodies=bodies, model=b.compile() if compiled else None)


def main(ref):
    arrays, pool = {}, []
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    meta = {rel: _encode(parse(ref, rel), arrays, pool) for rel in FILES}
    np.savez_compressed(FIXTURE, meta=np.array(json.dumps(meta)), pool=np.array(pool, dtype=np.float64), **arrays)
    print(f"wrote {FIXTURE}: {len(FILES)} task files, {len(arrays)} arrays, {os.path.getsize(FIXTURE)} bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
