"""Generates tests/golden/mjcf/allegro_op3.npz: what the Allegro and OP3 task files of the reference say about the two tasks, so that
tests/test_registry_allegro_op3.py checks the hand-authored generators (modelgen/tasks.py allegro() / op3()) against them without the
reference tree.

Per task: what the MJCF subset loader (modelgen/mjcf.py) reads from task.xml (custom numerics and text, cost terms, trace sensors,
sensors, keyframes) with the robot file dropped (it exists upstream only as a patch against menagerie), the <option> attributes, and
the facts the robot patch adds (lines starting with "+": position gain, palm pose, sites, foot boxes, trace sensors, removed joints).
Only derived values are stored, never the files themselves.  Regenerate from a checkout of the reference project:
    python tests/golden/make_allegro_op3_fixtures.py PATH/TO/mujoco_mpc
"""
import os
import re
import sys
import xml.etree.ElementTree as ET

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_mjcf_fixtures as mf  # noqa: E402  (helpers only: its FILES list stays as it is)

FIXTURE = os.path.join(HERE, "mjcf", "allegro_op3.npz")
TASKS = {"allegro": ("tasks/allegro/task.xml", "tasks/allegro/right_hand.xml.patch", "right_hand_modified.xml"),
         "op3": ("tasks/op3/task.xml", "tasks/op3/op3.xml.patch", "op3_modified.xml")}


def _floats(s):
    return [float(x) for x in s.split()]


def _added(patch_text):
    """the XML elements a patch adds (its '+' lines, without the file header), as (tag, attributes)"""
    out = []
    for line in patch_text.splitlines():
        if line.startswith("+") and not line.startswith("+++"):
            for m in re.finditer(r"<(\w+)\s([^<>]*?)/?>", line[1:]):
                out.append((m.group(1), dict(re.findall(r'(\w+)="([^"]*)"', m.group(2)))))
    return out


def _removed_joints(patch_text):
    """joints the patch comments out: '+ <!-- <joint name=... -->' lines"""
    return [m.group(1) for line in patch_text.splitlines() if line.startswith("+") and "<!--" in line
            for m in re.finditer(r'<joint name="(\w+)"', line)]


def parse(ref, name):
    from mujoco_mpc_amd.modelgen import mjcf
    mjpc = os.path.join(ref, "mjpc")
    task_rel, patch_rel, robot = TASKS[name]
    b, info = mjcf.parse_mjcf(os.path.join(mjpc, task_rel), missing_ok=(robot,))
    option = ET.parse(os.path.join(mjpc, task_rel)).getroot().find("option")
    with open(os.path.join(mjpc, patch_rel)) as f:
        patch = f.read()
    added = [(t, a) for t, a in _added(patch) if "<!--" not in t]
    out = dict(info=info, option=dict(option.attrib) if option is not None else {},
               bodies=[dict(name=bd.name, pos=tuple(float(x) for x in bd.pos), mocap=bool(bd.mocap)) for bd in b.bodies],
               sites={a["name"]: tuple(_floats(a.get("pos", "0 0 0"))) for t, a in added if t == "site"},
               traces=[(a["objtype"], a["objname"]) for t, a in added if t == "framepos" and a.get("name", "").startswith("trace")],
               removed_joints=_removed_joints(patch))
    if name == "allegro":
        palm = [a for t, a in added if t == "body" and a.get("name") == "palm"][0]
        out["palm"] = dict(pos=tuple(_floats(palm["pos"])), quat=tuple(_floats(palm["quat"])))
        out["kp"] = [float(a["kp"]) for t, a in added if t == "position"][0]
    else:
        feet = []
        for line in patch.splitlines():          # the foot boxes are context lines (' '), next to the added foot sites
            m = re.search(r'<geom class="foot" pos="([^"]+)" size="([^"]+)"', line)
            if m:
                feet.append((tuple(_floats(m.group(1))), tuple(_floats(m.group(2)))))
        out["feet"] = feet
        out["removed_actuators"] = re.findall(r'^-\s*<position name="(\w+)"', patch, re.M)
    return out


def load(path=FIXTURE):
    """{"allegro": dict(...), "op3": dict(...)} as parse() returned it"""
    return mf.load(path)


def main(ref):
    sys.path.insert(0, mf.ROOT)
    arrays, pool = {}, []
    meta = {name: mf._encode(parse(ref, name), arrays, pool) for name in TASKS}
    import json
    np.savez_compressed(FIXTURE, meta=np.array(json.dumps(meta)), pool=np.array(pool, dtype=np.float64), **arrays)
    print(f"wrote {FIXTURE}: {len(TASKS)} tasks, {os.path.getsize(FIXTURE)} bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
