"""What the late rows of a step must be (TEST INFRASTRUCTURE ONLY): the expected rows of tests/late_cases.py's tables from the references
of tests/acc_ref.py, given the residual of whatever ran the step (the emulation on the CPU tier, the engine on the GPU tier).  The
acceleration is read from the step's own QACC rows; the QACC rows themselves are compared with M⁻¹(f − c) on the models without active
constraints."""
import numpy as np

from acc_ref import EDGE, AccRef, NearZone, TouchRef

G = np.array([0.0, 0.0, 9.81])


def dev(got, want):
    got, want = np.asarray(got, float), np.asarray(want, float)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))) if got.size else 0.0


def _split(m, X):
    nq, nv = m["nq"], m["nv"]
    return X[:, :nq], X[:, nq:nq + nv], X[:, nq + nv:]


def kinematic_want(c, res):
    """{block: expected rows} for late_cases.kinematic(name) and the residual `res` [n, nr] of its rows"""
    m, rows = c["model"], c["rows"]
    q, v, act = _split(m, c["X"])
    ref = AccRef(m)
    qacc = res[:, rows["qacc"]]
    sid = m["names"]["site"][c["site"]]
    fr = ref.frame("site", sid, q, v, qacc)
    want = dict(qpos=q, qvel=v, accelerometer=ref.local(fr, "linacc"), gyro=ref.local(fr, "angvel"), velocimeter=ref.local(fr, "linvel"),
                linacc_site=fr["linacc"], angacc_site=fr["angacc"])
    for ty, b in c["frames"]:
        f2 = ref.frame(ty, m["names"]["body"][b] if isinstance(b, str) else int(b), q, v, qacc)
        want[f"linacc_{ty}"] = f2["linacc"]; want[f"angacc_{ty}"] = f2["angacc"]
    want["norm"] = np.linalg.norm(2.0 * want["accelerometer"] - G, axis=1)[:, None]
    want["mixed"] = (0.5 * qacc[:, 0] - want["gyro"][:, 2] + 1.0)[:, None]
    smooth = ref.qacc_smooth(q, v, act, c["U"])
    return want, smooth, fr["R"]


def kinematic_deviation(c, res):
    """(largest deviation of the late and early blocks from the reference at the step's own qacc, deviation of qacc from M⁻¹(f − c),
    the site's rotation matrices)"""
    want, smooth, R = kinematic_want(c, res)
    worst = max(dev(res[:, c["rows"][k]], w) for k, w in want.items())
    return worst, dev(res[:, c["rows"]["qacc"]], smooth), R


def touch_want(c, res):
    """per state: the reference's dict (acc_ref.TouchRef) at the step's own qacc, plus `rows` = the expected late rows behind the qacc
    block (one per zone, then the norm row |t0 + t1 − 1|).  Raises NearZone when a contact point is within EDGE of a zone boundary."""
    m, nv = c["model"], c["nv"]
    ref = TouchRef(m, c["zones"])
    q, v, _ = _split(m, c["X"])
    out = []
    for i in range(len(c["X"])):
        r = ref(q[i], v[i], res[i, :nv])
        if r["near"] < EDGE:
            raise NearZone(f"state {i}: a contact point is {r['near']:.1e} from a zone boundary")
        r["rows"] = np.concatenate([r["touch"], [abs(r["touch"][0] + r["touch"][1] - 1.0)]])
        out.append(r)
    return out


def touch_deviation(c, res):
    """largest |row − reference| / max(1, |force|) over the states, and the references"""
    refs = touch_want(c, res)
    nv = c["nv"]
    worst = max(dev(res[i, nv:], r["rows"]) for i, r in enumerate(refs))
    return worst, refs


def touch_coverage(refs, airborne=()):
    """every state has an included and an excluded contact across its zones, except the ones listed as airborne for a zone"""
    for i, r in enumerate(refs):
        n = len(r["forces"])
        inc = any(len(z) > 0 for z in r["included"]); exc = any(len(z) < n for z in r["included"])
        assert n > 0 and inc and exc, f"state {i}: {n} contacts, included {r['included']}"
    for i, z in airborne:
        assert refs[i]["touch"][z] == 0.0 and len(refs[i]["included"][z]) == 0, f"state {i}: zone {z} is not in the air"
