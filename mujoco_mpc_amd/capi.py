"""ctypes mirror of include/mjpc_hip.h and loader for the in-tree HIP engine `libmjpc_hip.so`.

The engine is the product path: `load_engine()` raises if the shared library is missing — there is
no CPU fallback (the CPU oracle under oracle/ is test infrastructure and is never imported here).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ENGINE_PATH = os.path.join(_HERE, "csrc", "libmjpc_hip.so")

c_double_p = C.POINTER(C.c_double)
c_int_p = C.POINTER(C.c_int)

_MODEL_INT_SIZES = ["nq", "nv", "nu", "na", "nbody", "njnt", "ngeom", "nsite", "nmocap", "nuserdata", "nkey", "nexclude", "ntendon", "nwrap", "nmesh", "nmeshvert", "nhfield", "nhfielddata"]
_OPTIONAL_TENDON = ("tendon_stiffness", "tendon_damping", "tendon_lengthspring", "tendon_frictionloss", "tendon_solref_fri", "tendon_solimp_fri")
_OPTIONAL_EQ = ("eq_type", "eq_obj1id", "eq_obj2id", "eq_active0", "eq_data", "eq_solref", "eq_solimp")
_OPTIONAL_ACT = ("actuator_dyntype", "actuator_actadr", "actuator_actlimited", "actuator_dynprm", "actuator_actrange")
_OPTION_DEFAULTS = dict(enableflags=0, solver=2, integrator=0, noslip_iterations=0, neq=0, unsupported=0)
_OPTIONAL_MESH = ("nmesh", "nmeshvert", "geom_dataid", "mesh_vertadr", "mesh_vertnum", "mesh_vert", "nhfield", "nhfielddata", "hfield_nrow",
                  "hfield_ncol", "hfield_adr", "hfield_size", "hfield_data")
_MODEL_INT_ARRAYS_BODY = ["body_parentid", "body_rootid", "body_weldid", "body_mocapid", "body_jntnum", "body_jntadr",
                          "body_dofnum", "body_dofadr"]
_MODEL_DBL_ARRAYS_BODY = ["body_pos", "body_quat", "body_ipos", "body_iquat", "body_mass", "body_subtreemass",
                          "body_inertia", "body_invweight0"]


class MjpcHipModel(C.Structure):
    _fields_ = (
        [("struct_size", C.c_int)] + [(n, C.c_int) for n in _MODEL_INT_SIZES]
        + [("timestep", C.c_double), ("gravity", C.c_double * 3), ("impratio", C.c_double),
           ("tolerance", C.c_double), ("ls_tolerance", C.c_double), ("cone", C.c_int), ("iterations", C.c_int),
           ("ls_iterations", C.c_int), ("disableflags", C.c_int), ("enableflags", C.c_int), ("solver", C.c_int), ("integrator", C.c_int),
           ("noslip_iterations", C.c_int), ("neq", C.c_int), ("unsupported", C.c_int), ("meaninertia", C.c_double),
           ("density", C.c_double), ("viscosity", C.c_double), ("wind", C.c_double * 3),
           ("nconmax", C.c_int), ("nefcmax", C.c_int)]
        + [(n, c_int_p) for n in _MODEL_INT_ARRAYS_BODY]
        + [(n, c_double_p) for n in _MODEL_DBL_ARRAYS_BODY]
        + [("jnt_actfrclimited", c_int_p), ("jnt_actfrcrange", c_double_p), ("body_gravcomp", c_double_p)]
        + [(n, c_int_p) for n in ["jnt_type", "jnt_qposadr", "jnt_dofadr", "jnt_bodyid", "jnt_limited"]]
        + [(n, c_double_p) for n in ["jnt_pos", "jnt_axis", "jnt_stiffness", "jnt_range", "jnt_margin",
                                     "jnt_solref", "jnt_solimp", "qpos0", "qpos_spring"]]
        + [(n, c_int_p) for n in ["dof_bodyid", "dof_jntid", "dof_parentid"]]
        + [(n, c_double_p) for n in ["dof_armature", "dof_damping", "dof_frictionloss", "dof_invweight0",
                                     "dof_solref", "dof_solimp"]]
        + [(n, c_int_p) for n in ["geom_type", "geom_contype", "geom_conaffinity", "geom_condim", "geom_bodyid",
                                  "geom_group", "geom_priority"]]
        + [(n, c_double_p) for n in ["geom_size", "geom_pos", "geom_quat", "geom_friction", "geom_solmix",
                                     "geom_solref", "geom_solimp", "geom_margin", "geom_gap", "geom_rbound"]]
        + [("exclude_signature", c_int_p)]
        + [(n, c_int_p) for n in ["eq_type", "eq_obj1id", "eq_obj2id", "eq_active0"]] + [(n, c_double_p) for n in ["eq_data", "eq_solref", "eq_solimp"]]
        + [("site_bodyid", c_int_p), ("site_pos", c_double_p), ("site_quat", c_double_p)]
        + [(n, c_int_p) for n in ["actuator_trntype", "actuator_trnid", "actuator_ctrllimited", "actuator_forcelimited", "actuator_biastype"]]
        + [(n, c_double_p) for n in ["actuator_gainprm", "actuator_biasprm", "actuator_gear", "actuator_gear6", "actuator_ctrlrange",
                                     "actuator_forcerange"]]
        + [(n, c_int_p) for n in ["actuator_dyntype", "actuator_actadr", "actuator_actlimited"]]
        + [(n, c_double_p) for n in ["actuator_dynprm", "actuator_actrange"]]
        + [(n, c_int_p) for n in ["tendon_adr", "tendon_num", "tendon_limited", "wrap_objid"]]
        + [(n, c_double_p) for n in ["wrap_prm", "tendon_range", "tendon_margin", "tendon_solref_lim", "tendon_solimp_lim",
                                     "tendon_invweight0", "tendon_stiffness", "tendon_damping", "tendon_lengthspring",
                                     "tendon_frictionloss", "tendon_solref_fri", "tendon_solimp_fri"]]
        + [(n, c_int_p) for n in ["geom_dataid", "mesh_vertadr", "mesh_vertnum"]] + [("mesh_vert", c_double_p)]
        + [(n, c_int_p) for n in ["hfield_nrow", "hfield_ncol", "hfield_adr"]] + [("hfield_size", c_double_p), ("hfield_data", c_double_p)]
        + [("key_qpos", c_double_p), ("key_mpos", c_double_p)]
        + [("actuator_refsite", c_int_p), ("noslip_tolerance", C.c_double)]
    )


class MjpcHipTask(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int), ("task_id", C.c_int), ("num_residual", C.c_int), ("num_term", C.c_int), ("num_trace", C.c_int),
        ("dim_norm_residual", c_int_p), ("norm", c_int_p), ("num_norm_parameter", c_int_p),
        ("weight", c_double_p), ("norm_parameter", c_double_p), ("risk", C.c_double),
        ("num_parameter", C.c_int), ("parameters", c_double_p),
        ("trace_objtype", c_int_p), ("trace_objid", c_int_p),
        ("num_int", C.c_int), ("int_data", c_int_p), ("num_dbl", C.c_int), ("dbl_data", c_double_p),
    ]


class MjpcHipPlanInput(C.Structure):
    _fields_ = [
        ("state", c_double_p), ("mocap", c_double_p), ("userdata", c_double_p), ("time", C.c_double),
        ("knot_times", c_double_p), ("knot_values", c_double_p), ("num_spline_points", C.c_int),
        ("interpolation", C.c_int), ("num_trajectory", C.c_int), ("horizon", C.c_int),
        ("candidate_offset", C.c_int), ("num_local", C.c_int), ("noise_exploration", C.c_double * 2),
        ("noise_eps", c_double_p), ("noise_sel", c_int_p), ("seed", C.c_uint64), ("stream", C.c_uint64),
        ("noise_std", c_double_p), ("nominal_index", C.c_int),
        ("candidate_knots", c_double_p), ("xfrc_std", C.c_double), ("xfrc_rate", C.c_double),
    ]


class MjpcHipPlanOutput(C.Structure):
    _fields_ = [
        ("returns", c_double_p), ("failure", c_int_p), ("winner", C.c_int), ("winner_return", C.c_double),
        ("states", c_double_p), ("actions", c_double_p), ("times", c_double_p), ("residual", c_double_p),
        ("costs", c_double_p), ("trace", c_double_p), ("winner_knots", c_double_p),
        ("noise_compute_time_us", C.c_double), ("rollouts_compute_time_us", C.c_double),
    ]


def _dp(a):
    return a.ctypes.data_as(c_double_p) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(c_int_p) if a is not None else None


class CModel:
    """Owns contiguous numpy copies and the ctypes structs that point into them."""

    def __init__(self, model: dict, task: dict):
        self.model = model
        self.task = task
        self._keep = []
        m = MjpcHipModel()
        for name, ctype in MjpcHipModel._fields_:
            if name == "struct_size":
                m.struct_size = C.sizeof(MjpcHipModel)
                continue
            if name in _OPTION_DEFAULTS and name not in model:        # mjOption fields added later: MuJoCo's defaults
                v = _OPTION_DEFAULTS[name]
            elif name in _OPTIONAL_TENDON and name not in model:       # models built before these fields existed: no passive tendon forces
                nt = int(model["ntendon"])
                v = (np.tile([0.02, 1.0], nt) if name == "tendon_solref_fri" else np.tile([0.9, 0.95, 0.001, 0.5, 2.0], nt) if name == "tendon_solimp_fri"
                     else np.zeros(nt * (2 if name == "tendon_lengthspring" else 1)))
            elif name in ("density", "viscosity", "wind") and name not in model:      # models built before fluid forces existed
                v = (0.0, 0.0, 0.0) if name == "wind" else 0.0
            elif name in ("jnt_actfrclimited", "jnt_actfrcrange") and name not in model:      # models built before the joint-level force clamp existed
                v = np.zeros(int(model["njnt"]) * (2 if name == "jnt_actfrcrange" else 1))
            elif name == "body_gravcomp" and name not in model:       # models built before gravity compensation existed
                v = np.zeros(int(model["nbody"]))
            elif name == "actuator_gear6" and name not in model:      # models built before site transmissions existed
                v = np.zeros(6 * int(model["nu"]))
            elif name == "actuator_refsite" and name not in model:    # models built before reference sites existed: none
                v = -np.ones(int(model["nu"]))
            elif name == "noslip_tolerance" and name not in model:
                v = 1e-6
            elif name in _OPTIONAL_EQ and name not in model:            # models built before equality constraints existed: none
                v = np.zeros(0)
            elif name in _OPTIONAL_ACT and name not in model:           # models built before activation states existed: none
                nu_ = int(model["nu"])
                v = -np.ones(nu_) if name == "actuator_actadr" else np.zeros(nu_ * (2 if name == "actuator_actrange" else 1))
            elif name in _OPTIONAL_MESH and name not in model:        # ... no meshes
                v = -np.ones(int(model["ngeom"])) if name == "geom_dataid" else (0 if name in ("nmesh", "nmeshvert", "nhfield", "nhfielddata") else np.zeros(0))
            else:
                v = model[name]
            if ctype is c_double_p:
                arr = np.ascontiguousarray(np.asarray(v, dtype=np.float64).ravel())
                if arr.size == 0:
                    arr = np.zeros(1)
                self._keep.append(arr); setattr(m, name, _dp(arr))
            elif ctype is c_int_p:
                arr = np.ascontiguousarray(np.asarray(v, dtype=np.int32).ravel())
                if arr.size == 0:
                    arr = np.zeros(1, np.int32)
                self._keep.append(arr); setattr(m, name, _ip(arr))
            elif name in ("gravity", "wind"):
                setattr(m, name, (C.c_double * 3)(*[float(x) for x in v]))
            elif ctype is C.c_int:
                setattr(m, name, int(v))
            else:
                setattr(m, name, float(v))
        self.c_model = m
        self.c_task = self.make_task(task)

    def make_task(self, task: dict) -> MjpcHipTask:
        t = MjpcHipTask()
        for name, ctype in MjpcHipTask._fields_:
            if name == "struct_size":
                t.struct_size = C.sizeof(MjpcHipTask)
                continue
            v = task[name]
            if ctype is c_double_p:
                arr = np.ascontiguousarray(np.asarray(v, dtype=np.float64).ravel())
                if arr.size == 0:
                    arr = np.zeros(1)
                self._keep.append(arr); setattr(t, name, _dp(arr))
            elif ctype is c_int_p:
                arr = np.ascontiguousarray(np.asarray(v, dtype=np.int32).ravel())
                if arr.size == 0:
                    arr = np.zeros(1, np.int32)
                self._keep.append(arr); setattr(t, name, _ip(arr))
            elif ctype is C.c_int:
                setattr(t, name, int(v))
            else:
                setattr(t, name, float(v))
        return t

    @property
    def dim_state(self):
        return self.model["nq"] + self.model["nv"] + self.model["na"]


def make_plan_input(cm: CModel, state, mocap, time, knot_times, knot_values, interpolation, num_trajectory, horizon,
                    sigma=(0.1, 0.0), noise_eps=None, noise_sel=None, seed=0, stream=0, candidate_offset=0,
                    num_local=None, userdata=None, noise_std=None, nominal_index=0, candidate_knots=None, xfrc_std=0.0, xfrc_rate=0.0):
    keep = []

    def arr(x, n=None):
        a = np.ascontiguousarray(np.asarray(x if x is not None else np.zeros(max(n or 1, 1)), dtype=np.float64).ravel())
        if a.size == 0:
            a = np.zeros(1)
        keep.append(a)
        return a
    inp = MjpcHipPlanInput()
    inp.state = _dp(arr(state)); inp.mocap = _dp(arr(mocap, 7 * cm.model["nmocap"]))
    inp.userdata = _dp(arr(userdata, cm.model["nuserdata"])); inp.time = float(time)
    kt = arr(knot_times); kv = arr(knot_values)
    inp.knot_times = _dp(kt); inp.knot_values = _dp(kv)
    inp.num_spline_points = int(len(np.asarray(knot_times).ravel())); inp.interpolation = int(interpolation)
    inp.num_trajectory = int(num_trajectory); inp.horizon = int(horizon)
    inp.candidate_offset = int(candidate_offset)
    inp.num_local = int(num_trajectory if num_local is None else num_local)
    inp.noise_exploration = (C.c_double * 2)(float(sigma[0]), float(sigma[1]))
    if noise_eps is not None:
        inp.noise_eps = _dp(arr(noise_eps))
    if noise_sel is not None:
        s = np.ascontiguousarray(np.asarray(noise_sel, dtype=np.int32)); keep.append(s); inp.noise_sel = _ip(s)
    inp.seed = int(seed); inp.stream = int(stream)
    if noise_std is not None:
        inp.noise_std = _dp(arr(noise_std))
    inp.nominal_index = int(nominal_index)
    if candidate_knots is not None:
        inp.candidate_knots = _dp(arr(candidate_knots))
    inp.xfrc_std = float(xfrc_std); inp.xfrc_rate = float(xfrc_rate)
    inp._keep = keep
    return inp


class MjpcHipRiccatiSettings(C.Structure):
    """include/mjpc_hip.h: the iLQG backward pass's settings (ilqg/settings.h, plus the regularisation factor)"""
    _fields_ = [("struct_size", C.c_int), ("regularization_type", C.c_int), ("action_limits", C.c_int), ("max_regularization_iterations", C.c_int),
                ("min_regularization", C.c_double), ("max_regularization", C.c_double), ("regularization_factor", C.c_double)]


def riccati_settings(regularization_type=0, action_limits_on=1, max_regularization_iterations=5, min_regularization=1.0e-6, max_regularization=1.0e6,
                     regularization_factor=2.0):
    s = MjpcHipRiccatiSettings()
    s.struct_size = C.sizeof(MjpcHipRiccatiSettings)
    s.regularization_type = int(regularization_type); s.action_limits = int(action_limits_on)
    s.max_regularization_iterations = int(max_regularization_iterations)
    s.min_regularization = float(min_regularization); s.max_regularization = float(max_regularization); s.regularization_factor = float(regularization_factor)
    return s


class MjpcHipDirectSettings(C.Structure):
    """include/mjpc_hip.h: the sensors, noises and settings of the direct optimiser's window cost"""
    _fields_ = [("struct_size", C.c_int), ("num_sensor", C.c_int), ("sensor_first_row", C.c_int), ("num_sensor_rows", C.c_int),
                ("sensor_dim", c_int_p), ("sensor_stage", c_int_p), ("sensor_norm", c_int_p), ("sensor_norm_parameter", c_double_p),
                ("noise_sensor", c_double_p), ("noise_process", c_double_p), ("sensor_mask", c_int_p),
                ("sensor_flag", C.c_int), ("force_flag", C.c_int), ("time_scaling_sensor", C.c_int), ("time_scaling_force", C.c_int),
                ("first_step_position_sensors", C.c_int), ("last_step_position_sensors", C.c_int), ("last_step_velocity_sensors", C.c_int),
                ("timestep", C.c_double)]


def direct_settings(sensor_dim, sensor_stage, sensor_norm, sensor_norm_parameter, noise_sensor, noise_process, timestep, sensor_first_row=0,
                    sensor_mask=None, sensor_flag=True, force_flag=True, time_scaling_sensor=True, time_scaling_force=True,
                    first_step_position_sensors=True, last_step_position_sensors=False, last_step_velocity_sensors=False):
    """MjpcHipDirectSettings over contiguous copies of the arrays (kept alive on the struct).  sensor_norm_parameter [num_sensor, 2] = {p, q};
    sensor_mask [T, num_sensor] or None (every sensor on).  The defaults of the flags are the reference's (direct/direct.h)."""
    keep = []

    def ints(x):
        a = np.ascontiguousarray(np.asarray(x, dtype=np.int32).ravel()); keep.append(a)
        return (a if a.size else np.zeros(1, np.int32)).ctypes.data_as(c_int_p)

    def dbls(x):
        a = np.ascontiguousarray(np.asarray(x, dtype=np.float64).ravel()); keep.append(a)
        return (a if a.size else np.zeros(1)).ctypes.data_as(c_double_p)
    s = MjpcHipDirectSettings()
    s.struct_size = C.sizeof(MjpcHipDirectSettings)
    dim = np.asarray(sensor_dim, dtype=np.int64).ravel()
    s.num_sensor = int(dim.size); s.sensor_first_row = int(sensor_first_row); s.num_sensor_rows = int(dim.sum())
    s.sensor_dim = ints(sensor_dim); s.sensor_stage = ints(sensor_stage); s.sensor_norm = ints(sensor_norm)
    s.sensor_norm_parameter = dbls(sensor_norm_parameter); s.noise_sensor = dbls(noise_sensor); s.noise_process = dbls(noise_process)
    if sensor_mask is not None:
        s.sensor_mask = ints(sensor_mask)
    s.sensor_flag = int(bool(sensor_flag)); s.force_flag = int(bool(force_flag))
    s.time_scaling_sensor = int(bool(time_scaling_sensor)); s.time_scaling_force = int(bool(time_scaling_force))
    s.first_step_position_sensors = int(bool(first_step_position_sensors)); s.last_step_position_sensors = int(bool(last_step_position_sensors))
    s.last_step_velocity_sensors = int(bool(last_step_velocity_sensors))
    s.timestep = float(timestep)
    s._keep = keep
    return s


class MjpcHipFeedbackPolicy(C.Structure):
    """include/mjpc_hip.h: the feedback policy of mjpc_hip_plan_feedback (iLQG's ActionRollouts / FeedbackRollouts)"""
    _fields_ = [("struct_size", C.c_int), ("mode", C.c_int), ("T", C.c_int), ("representation", C.c_int),
                ("times", c_double_p), ("states", c_double_p), ("actions", c_double_p), ("feedback_gain", c_double_p),
                ("action_improvement", c_double_p), ("action_step", c_double_p), ("feedback_scaling", c_double_p), ("use_feedback", C.c_int)]


FEEDBACK_INDEXED, FEEDBACK_TIME = 0, 1


def make_feedback_policy(times, states, actions, feedback_gain, action_step, feedback_scaling, action_improvement=None, mode=FEEDBACK_INDEXED,
                         representation=1, use_feedback=True):
    """MjpcHipFeedbackPolicy over contiguous copies of the arrays (kept alive on the struct)."""
    keep = []

    def arr(x):
        a = np.ascontiguousarray(np.asarray(x, dtype=np.float64).ravel())
        keep.append(a)
        return _dp(a)
    p = MjpcHipFeedbackPolicy()
    p.struct_size = C.sizeof(MjpcHipFeedbackPolicy)
    p.mode = int(mode); p.T = int(len(np.asarray(times).ravel())); p.representation = int(representation)
    p.times = arr(times); p.states = arr(states); p.actions = arr(actions); p.feedback_gain = arr(feedback_gain)
    if action_improvement is not None:
        p.action_improvement = arr(action_improvement)
    p.action_step = arr(action_step); p.feedback_scaling = arr(feedback_scaling)
    p.use_feedback = 1 if use_feedback else 0
    p._keep = keep
    return p


_engine = None


def load_engine():
    """Load libmjpc_hip.so (HIP engine).  Fails loudly when it has not been built."""
    global _engine
    if _engine is not None:
        return _engine
    if not os.path.exists(ENGINE_PATH):
        raise RuntimeError(f"HIP engine not built: {ENGINE_PATH} missing (run `python -c 'import __graft_entry__ as g; g.build()'`)")
    lib = C.CDLL(ENGINE_PATH)
    lib.mjpc_hip_create.restype = C.c_void_p
    lib.mjpc_hip_create.argtypes = [C.POINTER(MjpcHipModel), C.POINTER(MjpcHipTask), C.c_int, C.c_int, C.c_int]
    lib.mjpc_hip_destroy.argtypes = [C.c_void_p]
    lib.mjpc_hip_destroy.restype = None
    lib.mjpc_hip_set_task.argtypes = [C.c_void_p, C.POINTER(MjpcHipTask)]
    lib.mjpc_hip_plan.argtypes = [C.c_void_p, C.POINTER(MjpcHipPlanInput), C.POINTER(MjpcHipPlanOutput)]
    lib.mjpc_hip_plan_async.argtypes = [C.c_void_p, C.POINTER(MjpcHipPlanInput)]
    lib.mjpc_hip_plan_fetch.argtypes = [C.c_void_p, C.POINTER(MjpcHipPlanOutput)]
    lib.mjpc_hip_get_candidate.argtypes = [C.c_void_p, C.c_int, C.POINTER(MjpcHipPlanOutput)]
    lib.mjpc_hip_plan_mixed_async.argtypes = [C.c_void_p, C.POINTER(MjpcHipPlanInput), C.c_int]
    lib.mjpc_hip_plan_mixed.argtypes = [C.c_void_p, C.POINTER(MjpcHipPlanInput), C.c_int, C.POINTER(MjpcHipPlanOutput)]
    lib.mjpc_hip_noise_history_reset.argtypes = [C.c_void_p]
    lib.mjpc_hip_plan_feedback_async.argtypes = [C.c_void_p, C.POINTER(MjpcHipPlanInput), C.POINTER(MjpcHipFeedbackPolicy)]
    lib.mjpc_hip_plan_feedback.argtypes = [C.c_void_p, C.POINTER(MjpcHipPlanInput), C.POINTER(MjpcHipFeedbackPolicy), C.POINTER(MjpcHipPlanOutput)]
    lib.mjpc_hip_feedback_resample_time_us.argtypes = [C.c_void_p]; lib.mjpc_hip_feedback_resample_time_us.restype = C.c_double
    lib.mjpc_hip_sample_gradient.argtypes = [C.c_void_p, C.c_int, c_int_p, c_double_p, c_double_p]
    lib.mjpc_hip_step_batch.argtypes = [C.c_void_p, C.c_int] + [c_double_p] * 5 + [c_double_p, c_double_p, c_int_p]
    lib.mjpc_hip_transition_fd.argtypes = [C.c_void_p, C.c_int] + [c_double_p] * 5 + [C.c_double, C.c_int, C.c_int] + [c_double_p] * 4 + [c_int_p]
    lib.mjpc_hip_inverse_batch.argtypes = [C.c_void_p, C.c_int] + [c_double_p] * 6 + [C.c_int] + [c_double_p] * 3 + [c_int_p]
    lib.mjpc_hip_inverse_fd.argtypes = [C.c_void_p, C.c_int] + [c_double_p] * 6 + [C.c_int, C.c_double, C.c_int] + [c_double_p] * 6 + [c_int_p]
    lib.mjpc_hip_unscented_moments.argtypes = ([C.c_void_p, c_double_p, c_double_p, C.c_double, c_double_p, c_double_p, C.c_double] + [c_double_p] * 4
                                               + [C.c_int, C.c_int] + [c_double_p] * 6 + [c_int_p])
    lib.mjpc_hip_linearize_step.argtypes = [C.c_void_p, c_double_p, c_double_p, C.c_double, c_double_p, c_double_p, C.c_double, C.c_int] + [c_double_p] * 4 + [c_int_p]
    lib.mjpc_hip_cost_derivatives.argtypes = [C.c_void_p, C.c_int] + [c_double_p] * 3 + [C.c_int, C.c_int] + [c_double_p] * 6
    lib.mjpc_hip_trajectory_gradient.argtypes = [C.c_void_p, C.c_int] + [c_double_p] * 6 + [C.c_double, C.c_int] + [c_double_p] * 5 + [c_int_p]
    lib.mjpc_hip_ilqg_backward_pass.argtypes = [C.c_void_p] + [C.c_int] * 3 + [c_double_p] * 9 + [C.POINTER(MjpcHipRiccatiSettings)] + [c_double_p] * 12 + [c_int_p]
    lib.mjpc_hip_trajectory_ilqg.argtypes = ([C.c_void_p, C.c_int] + [c_double_p] * 6 + [C.c_double, C.c_int, C.POINTER(MjpcHipRiccatiSettings)]
                                             + [c_double_p] * 12 + [c_int_p, c_int_p])
    lib.mjpc_hip_riccati_layout_bytes.argtypes = [C.c_int, C.c_int, c_int_p]
    lib.mjpc_hip_direct_cost.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(MjpcHipDirectSettings), C.c_int] + [c_double_p] * 13 + [c_int_p]
    lib.mjpc_hip_direct_cost_derivatives.argtypes = ([C.c_void_p, C.c_int, C.POINTER(MjpcHipDirectSettings), C.c_double, C.c_int, C.c_int] + [c_double_p] * 25
                                                     + [c_int_p])
    lib.mjpc_hip_direct_assemble.argtypes = [C.c_void_p] + [C.c_int] * 3 + [C.POINTER(MjpcHipDirectSettings)] + [c_double_p] * 19
    lib.mjpc_hip_get_knots.argtypes = [C.c_void_p, c_double_p]
    lib.mjpc_hip_get_frame.argtypes = [C.c_void_p] + [c_double_p] * 5
    lib.mjpc_hip_kernel_time.argtypes = [C.c_void_p, c_double_p, c_double_p]
    lib.mjpc_hip_device_ptrs.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    lib.mjpc_hip_get_all_candidates.argtypes = [C.c_void_p] + [c_double_p] * 7 + [c_int_p]
    lib.mjpc_hip_get_traces.argtypes = [C.c_void_p, c_double_p]
    lib.mjpc_hip_lds_bytes.argtypes = [C.c_void_p]
    lib.mjpc_hip_layout_bytes.argtypes = [C.POINTER(MjpcHipModel), C.POINTER(MjpcHipTask), C.c_int]
    lib.mjpc_hip_set_fetch_mode.argtypes = [C.c_void_p, C.c_int]
    lib.mjpc_hip_dense_tier.argtypes = [C.c_void_p, c_int_p]
    lib.mjpc_hip_debug_dense_capacity.argtypes = [C.c_void_p, c_int_p, c_int_p, c_int_p]; lib.mjpc_hip_debug_dense_capacity.restype = None
    lib.mjpc_hip_debug_spill.argtypes = [C.c_void_p, c_int_p]
    lib.mjpc_hip_debug_spill_layout.argtypes = [C.POINTER(MjpcHipModel), C.POINTER(MjpcHipTask), c_int_p, c_int_p]
    lib.mjpc_hip_multi_create.restype = C.c_void_p
    lib.mjpc_hip_multi_create.argtypes = [C.POINTER(MjpcHipModel), C.POINTER(MjpcHipTask), C.c_int, C.c_int, C.c_int, c_int_p]
    lib.mjpc_hip_multi_destroy.argtypes = [C.c_void_p]
    lib.mjpc_hip_multi_destroy.restype = None
    lib.mjpc_hip_multi_set_task.argtypes = [C.c_void_p, C.POINTER(MjpcHipTask)]
    lib.mjpc_hip_multi_plan.argtypes = [C.c_void_p, C.POINTER(MjpcHipPlanInput), C.POINTER(MjpcHipPlanOutput)]
    lib.mjpc_hip_multi_get_candidate.argtypes = [C.c_void_p, C.c_int, C.POINTER(MjpcHipPlanOutput)]
    lib.mjpc_hip_multi_get_knots.argtypes = [C.c_void_p, c_double_p]
    lib.mjpc_hip_multi_get_traces.argtypes = [C.c_void_p, c_double_p]
    lib.mjpc_hip_multi_num_devices.argtypes = [C.c_void_p]
    lib.mjpc_hip_multi_engine.restype = C.c_void_p
    lib.mjpc_hip_multi_engine.argtypes = [C.c_void_p, C.c_int]
    lib.mjpc_hip_last_error.restype = C.c_char_p
    lib.mjpc_hip_version.restype = C.c_int
    # a stale library next to a newer ctypes layout must not get as far as reading pointers out of the wrong offsets
    if lib.mjpc_hip_version() != ABI_VERSION:
        raise RuntimeError(f"{ENGINE_PATH}: ABI revision {lib.mjpc_hip_version()}, these bindings are revision {ABI_VERSION}: rebuild the engine")
    for what, ctype in (("model", MjpcHipModel), ("task", MjpcHipTask), ("plan_input", MjpcHipPlanInput), ("plan_output", MjpcHipPlanOutput),
                        ("feedback_policy", MjpcHipFeedbackPolicy)):
        n = getattr(lib, "mjpc_hip_sizeof_" + what)()
        if n != C.sizeof(ctype):
            raise RuntimeError(f"{ENGINE_PATH}: sizeof {what} struct is {n} in the library, {C.sizeof(ctype)} in capi.py: rebuild the engine")
    lib.mjpc_hip_debug_set.argtypes = [C.c_char_p, C.c_char_p]
    lib.mjpc_hip_debug_set.restype = None
    _engine = lib
    return lib


def debug_set(name: str, value=None):
    """Engine diagnostics knob (include/mjpc_hip_debug.h), read when an engine is created; value None clears it."""
    load_engine().mjpc_hip_debug_set(name.encode(), None if value is None else str(value).encode())


ABI_VERSION = 4            # MJPC_HIP_ABI_VERSION of include/mjpc_hip.h

# late table sources and touch zone shapes of MJPC_TASK_TABLE (include/mjpc_hip.h; modelgen.ResidualTable builds them)
(MJPC_TBL_QACC, MJPC_TBL_LINACC, MJPC_TBL_ANGACC, MJPC_TBL_ACCELEROMETER, MJPC_TBL_GYRO, MJPC_TBL_VELOCIMETER, MJPC_TBL_TOUCH) = range(21, 28)
MJPC_ZONE_SPHERE, MJPC_ZONE_CAPSULE, MJPC_ZONE_ELLIPSOID, MJPC_ZONE_CYLINDER, MJPC_ZONE_BOX = 2, 3, 4, 5, 6

EXPORTED_SYMBOLS = [
    "mjpc_hip_sizeof_model", "mjpc_hip_sizeof_task", "mjpc_hip_sizeof_plan_input", "mjpc_hip_sizeof_plan_output", "mjpc_hip_debug_set",
    "mjpc_hip_create", "mjpc_hip_destroy", "mjpc_hip_set_task", "mjpc_hip_plan", "mjpc_hip_plan_async",
    "mjpc_hip_plan_fetch", "mjpc_hip_get_candidate", "mjpc_hip_kernel_time", "mjpc_hip_device_ptrs",
    "mjpc_hip_last_error", "mjpc_hip_version", "mjpc_hip_get_knots", "mjpc_hip_get_frame",
    "mjpc_hip_get_traces", "mjpc_hip_get_all_candidates", "mjpc_hip_lds_bytes", "mjpc_hip_layout_bytes", "mjpc_hip_set_fetch_mode", "mjpc_hip_dense_tier", "mjpc_hip_debug_dense_capacity",
    "mjpc_hip_debug_spill", "mjpc_hip_debug_spill_layout",
    "mjpc_hip_plan_mixed_async", "mjpc_hip_plan_mixed", "mjpc_hip_noise_history_reset", "mjpc_hip_sample_gradient",
    "mjpc_hip_plan_feedback_async", "mjpc_hip_plan_feedback", "mjpc_hip_feedback_resample_time_us", "mjpc_hip_sizeof_feedback_policy",
    "mjpc_hip_step_batch", "mjpc_hip_transition_fd", "mjpc_hip_inverse_batch", "mjpc_hip_inverse_fd", "mjpc_hip_unscented_moments", "mjpc_hip_linearize_step", "mjpc_hip_cost_derivatives", "mjpc_hip_trajectory_gradient",
    "mjpc_hip_ilqg_backward_pass", "mjpc_hip_trajectory_ilqg", "mjpc_hip_riccati_layout_bytes", "mjpc_hip_direct_assemble", "mjpc_hip_direct_cost", "mjpc_hip_direct_cost_derivatives",
    "mjpc_hip_multi_create", "mjpc_hip_multi_destroy", "mjpc_hip_multi_set_task", "mjpc_hip_multi_plan", "mjpc_hip_multi_get_candidate",
    "mjpc_hip_multi_get_knots", "mjpc_hip_multi_get_traces", "mjpc_hip_multi_num_devices", "mjpc_hip_multi_engine",
]
